"""tests/spectral_ref.py (numpy float64 from the definition, no torch.stft)
against the references the spectral GPU tests already rest on --
tests/distance_ref.py and tests/stft_loss_ref.py, torch.stft restatements that
tests/golden/make_golden_distance.py and make_stft_loss_check.py check against
the reference's own modules -- at 1e-12 relative, on a handful of the shapes of
tests/test_gpu_spectral_edges.py's sweep; the gradient-support helper against a
brute-force float64 autograd gradient; and the clamp condition on every
multires gradient case of that sweep.  No GPU."""
import numpy as np
import pytest
import torch

from tests import distance_ref as D
from tests import spectral_ref as S
from tests import stft_loss_ref as R

TIGHT = 1e-12


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_geometry_mirrors_the_kernels():
    """kConc = max(1, 1024 / n); kTile = kConc x 4 up to n = 1024, x 2 above."""
    assert [S.conc_of(n) for n in S.SCALES] == [16, 8, 4, 2, 1, 1, 1]
    assert [S.tile_of(n) for n in S.SCALES] == [64, 32, 16, 8, 4, 2, 2]
    assert S.seam_counts(64) == [3, 15, 16, 17, 63, 64, 65, 129]
    assert S.seam_counts(64, mag=True) == [3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 257]
    assert S.seam_counts(2048) == [1, 2, 3, 5]
    assert max(t for n in S.SCALES for _, t in S.seam_lengths(n, mag=True)) == 9215      # 9 frames at n = 4096
    assert (257, 4096) in S.seam_lengths(64, mag=True)
    for n in S.SCALES:
        assert all(t > n // 2 for _, t in S.seam_lengths(n, mag=True))


@pytest.mark.parametrize("n,rows,t_len", [(64, 3, 47), (64, 1, 33), (128, 3, 1055), (512, 1, 383), (1024, 3, 767),
                                          (2048, 1, 1535), (2048, 1, 1025), (4096, 3, 3071)])
def test_magnitudes_and_distance_match_distance_ref(n, rows, t_len):
    value, target = S.synth(rows, t_len, 40 + n)
    want = D.stft_mag(torch.from_numpy(target).double()[None], n).numpy()
    got = S.magnitudes(target, n)
    assert got.shape == want.shape == (rows, n // 2 + 1, S.frame_count(t_len, n // 4))
    assert np.abs(got - want).max() <= TIGHT * np.abs(want).max()
    t64, v64 = torch.from_numpy(target).double()[None], torch.from_numpy(value).double()[None]
    for eps in (1e-7, 1.0):
        (lin, log), = S.distance_terms(target, value, (n,), eps)
        (wlin, wlog), = D.distance_terms(t64, v64, (n,), eps)
        assert rel(lin, wlin) <= TIGHT and rel(log, wlog) <= TIGHT
        assert rel(S.distance(target, value, (n,), eps), D.distance(t64, v64, (n,), eps)) <= TIGHT
        assert rel(S.v1_loss(target, value, (n,), eps), float(R.v1_distance(t64, v64, (n,), eps))) <= TIGHT


def test_multi_scale_distance_is_the_sum_of_its_terms():
    value, target = S.synth(3, 2111, 5)
    t64, v64 = torch.from_numpy(target).double()[None], torch.from_numpy(value).double()[None]
    scales = (256, 64, 2048, 64)
    terms = S.distance_terms(target, value, scales, 1e-7)
    for (lin, log), (wlin, wlog) in zip(terms, D.distance_terms(t64, v64, scales, 1e-7)):
        assert rel(lin, wlin) <= TIGHT and rel(log, wlog) <= TIGHT
    assert terms[1] == terms[3]
    assert rel(S.distance(target, value, scales, 1e-7), sum(a + b for a, b in terms)) <= TIGHT


@pytest.mark.parametrize("res,rows,t_len", [
    (((64, 5, 37),), 3, 300), (((64, 70, 37),), 3, 300),              # hop > win
    (((128, 32, 127),), 1, 300), (((256, 7, 3),), 1, 200),            # odd n - win
    (((64, 16, 64),), 3, 33), (((64, 16, 64),), 1, 34),               # the pads cover the whole signal
    ((S.FORK_4096,), 1, 2049), (S.MIXED_8, 3, S.MIXED_8_T)])
def test_multires_terms_match_stft_loss_ref(res, rows, t_len):
    pred, target = S.synth(rows, t_len, 60 + t_len)
    got = S.mr_terms(pred, target, res)
    want = R.mr_terms(torch.from_numpy(pred).double(), torch.from_numpy(target).double(), res)
    assert len(got) == len(want) == len(res)
    for (sc, mag), (wsc, wmag), (n, hop, win) in zip(got, want, res):
        assert rel(sc, wsc) <= TIGHT and rel(mag, wmag) <= TIGHT, (n, hop, win)
        if n <= 256:                                                   # the O(n^2) DFT from the definition
            dsc, dmag = R.dft_terms(pred, target, n, hop, win)
            assert rel(sc, dsc) <= TIGHT and rel(mag, dmag) <= TIGHT, (n, hop, win)
    wsc, wmag = R.mr_loss(torch.from_numpy(pred).double(), torch.from_numpy(target).double(), res)
    sc, mag = S.mr_loss(pred, target, res)
    assert rel(sc, wsc) <= TIGHT and rel(mag, wmag) <= TIGHT


def test_an_impulse_fills_every_bin_with_its_window_sample():
    """|STFT| of a unit impulse: frames that one padded position reaches hold the
    window's sample there in every bin; frames that none reaches hold exact zeros."""
    n, t_len = 64, 300
    idx, w = S.padded_index(t_len, n), S.window(n, n)
    seen = 0
    for p in (0, 1, n // 2, t_len - 1, t_len - 2, 150):
        x = np.zeros((1, t_len))
        x[0, p] = 1.0
        m = S.magnitudes(x, n)[0]
        for f in range(m.shape[1]):
            js = np.nonzero(idx[f * 16:f * 16 + n] == p)[0]
            if len(js) == 0:
                assert not m[:, f].any()
            elif len(js) == 1:
                assert np.abs(m[:, f] - w[js[0]]).max() <= 1e-15
                seen += 1
    assert seen >= 10


# ------------------------------------------------------------------ the gradient's support
def _burst(rows, t_len, burst, seed, gain=1.0):
    full, target = S.synth(rows, t_len, seed)
    value = np.zeros_like(full)
    value[:, burst[0]:burst[1]] = gain * full[:, burst[0]:burst[1]]
    assert value[:, burst[0]:burst[1]].all()
    return value, target


BURSTS = {"left": (0, 5), "left1": (1, 3), "right": (295, 300), "right1": (297, 299), "middle": (140, 150)}


@pytest.mark.parametrize("geometry", [(64, 16, 64), (64, 5, 37), (64, 70, 37), (128, 32, 127), (256, 7, 3)])
@pytest.mark.parametrize("where", list(BURSTS))
def test_support_is_where_the_float64_gradient_is_nonzero(geometry, where):
    """Brute force: torch.stft + autograd in float64.  V1 (|V| = 0 has gradient 0)
    on its own geometry, multires (the clamp has gradient 0 under it) on all;
    the multires burst is loud enough that no burst-seeing frame sits under the
    clamp, so the gradient is nonzero on all of the support."""
    n, hop, win = geometry
    t_len, burst = 300, BURSTS[where]
    want = S.support(burst, t_len, n, hop, win)
    assert want[burst[0]:burst[1]].all() or hop > win
    value, target = _burst(2, t_len, burst, 11, gain=100.0)
    t64 = torch.from_numpy(target).double()

    def mr(v):
        sc, mag = R.mr_loss(v, t64, (geometry,))
        return (sc + mag,)
    _, (g,) = R.grad_of(mr, value, torch.float64)
    for row in g.numpy():
        assert np.array_equal(row != 0, want), np.nonzero((row != 0) != want)[0]
    if (hop, win) == (n // 4, n):
        value, _ = _burst(2, t_len, burst, 11)
        _, (g,) = R.grad_of(lambda v: (R.v1_distance(t64[None], v[None], (n,), 1e-7),), value, torch.float64)
        for row in g.numpy():
            assert np.array_equal(row != 0, want)


def test_support_of_a_broadband_value_leaves_the_gaps_of_a_long_hop():
    n, hop, win = 64, 70, 37
    t_len = 300
    want = S.support((0, t_len), t_len, n, hop, win)
    assert 0 < want.sum() < t_len                                      # hop > win: some samples belong to no frame
    pred, target = S.synth(1, t_len, 12)
    t64 = torch.from_numpy(target).double()
    _, (g,) = R.grad_of(lambda v: (sum(R.mr_loss(v, t64, ((n, hop, win),))),), pred, torch.float64)
    assert np.array_equal(g.numpy()[0] != 0, want)
    assert S.support((0, t_len), t_len, 64, 16, 64).all()


# ------------------------------------------------------------------ the clamp condition
def test_no_gradient_case_has_a_bin_in_the_clamp_band():
    """sqrt(max(power, 1e-7)) has a step in its derivative at the clamp.  No bin
    of the value or the target of any multires gradient case has float64 power
    inside [0.5e-7, 2e-7], so an fp32 run (power error about 1e-6 relative) puts
    every bin on the side of the step that float64 does."""
    cases = S.multires_gradient_cases()
    assert len({c[0] for c in cases}) == len(cases)
    for name, res, rows, t_len in cases:
        pred, target = S.multires_inputs(name)
        assert pred.shape == target.shape == (rows, t_len) and pred.dtype == np.float32
        assert S.in_clamp_band(pred, res) == 0, name
        assert S.in_clamp_band(target, res) == 0, name


def test_the_clamp_band_is_not_vacuous():
    """The band catches what it is meant to: an input built to sit at the clamp."""
    n = 64
    x = np.zeros((1, 300))
    x[0, 150] = np.sqrt(1e-7)                                          # frames hold power w[j]^2 1e-7 in every bin
    assert S.in_clamp_band(x, ((n, 16, n),)) > 0
