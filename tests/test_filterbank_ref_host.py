"""tests/filterbank_ref.py against what the repository already trusts, on the
CPU: the oracle's expressions that tests/test_gpu_edges.py uses, the
reference's own PQMF and resampler fixtures, the streaming identity the cached
synthesis relies on, and the unit-impulse closed forms that
tests/test_gpu_filterbank.py holds the kernels to."""
import numpy as np
import pytest

from oracle.rave_oracle import conv1d, get_padding, pqmf_filters, reverse_half
from tests import filterbank_ref as F


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def rel(a, b):
    """test_oracle_golden.py's measure: max-abs error over max(1, max|b|)."""
    return maxabs(a, b) / max(1.0, float(np.abs(b).max()))


@pytest.fixture(scope="module")
def filters(golden):
    from rave_amd.pqmf import kernels
    hkf, hki = kernels(golden("pqmf")["hk"])
    o_hkf, o_hki = pqmf_filters(golden("pqmf")["hk"])
    assert np.array_equal(hkf, o_hkf[:, 0]) and np.array_equal(hki, o_hki)
    assert hkf.shape == (16, 513) and hki.shape == (16, 16, 33)
    return hkf, hki


def _oracle_analysis(x, hkf, causal):
    return reverse_half(conv1d(x[:, None].astype(np.float64), hkf[:, None].astype(np.float64), None, stride=16,
                               pad=get_padding(hkf.shape[-1], causal=causal)))


def _oracle_synthesis(w, hki, causal):
    ys = conv1d(reverse_half(w.astype(np.float64)), hki.astype(np.float64), None,
                pad=get_padding(hki.shape[-1], causal=causal)) * 16
    return ys[:, ::-1, :].transpose(0, 2, 1).reshape(w.shape[0], -1)


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("frames", [1, 17, 300])
def test_analysis_equals_the_oracle_expression(filters, causal, frames):
    hkf, _ = filters
    x = np.random.default_rng(frames).standard_normal((2, 16 * frames)).astype(np.float32)
    want = _oracle_analysis(x, hkf, causal)
    pad = get_padding(513, causal=causal)[0]
    got = F.analysis(x, hkf, pad, frames, 16)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert maxabs(got, want) <= 1e-12 * np.abs(want).max()
    assert np.array_equal(F.analysis(x, hkf, pad, frames, 6), got[:, :6])


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("frames", [1, 17, 300])
def test_synthesis_equals_the_oracle_expression(filters, causal, frames):
    _, hki = filters
    w = np.random.default_rng(frames).standard_normal((2, 16, frames)).astype(np.float32)
    want = _oracle_synthesis(w, hki, causal)
    got = F.synthesis(w, hki, get_padding(33, causal=causal)[0], 0, 0, 0, None, frames)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert maxabs(got, want) <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("mode,with_noise", [(1, True), (1, False), (2, True)])
def test_synthesis_modes_equal_the_oracle_epilogue(filters, mode, with_noise):
    """x * sigmoid(amp) (+ noise) -> tanh as test_gpu_edges.py writes it, then
    the oracle's synthesis."""
    _, hki = filters
    rng = np.random.default_rng(mode)
    x = rng.standard_normal((2, 32, 45)).astype(np.float32)
    nz = (0.05 * rng.standard_normal((2, 16, 45))).astype(np.float32) if with_noise else None
    v = x[:, :16].astype(np.float64)
    if mode == 1:
        v = v * (1.0 / (1.0 + np.exp(-x[:, 16:].astype(np.float64))))
    v = np.tanh(v + (nz if with_noise else 0.0))
    want = _oracle_synthesis(v, hki, True)
    got = F.synthesis(x, hki, 32, mode, 0, 0, nz, 45)
    assert maxabs(got, want) <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ against the fixtures
@pytest.mark.parametrize("causal", [False, True])
def test_pqmf_fixtures(golden, filters, causal):
    """The bound test_oracle_golden.py holds the oracle to on the same fixtures."""
    hkf, hki = filters
    g = golden("pqmf")
    mode = "causal" if causal else "centered"
    pa, ps = get_padding(513, causal=causal)[0], get_padding(33, causal=causal)[0]
    x, bands = g["x"][:, 0], g["bands"]
    ana = F.analysis(x, hkf, pa, x.shape[-1] // 16, 16)
    assert rel(ana, g[f"analysis_{mode}"]) < 1e-5
    syn = F.synthesis(bands, hki, ps, 0, 0, 0, None, bands.shape[-1])
    assert rel(syn[:, None], g[f"synthesis_{mode}"]) < 1e-5
    rt = F.synthesis(ana, hki, ps, 0, 0, 0, None, ana.shape[-1])
    assert rel(rt[:, None], g[f"roundtrip_{mode}"]) < 1e-5
    # and the fp32 run is a run of the same thing
    assert rel(F.analysis(x, hkf, pa, x.shape[-1] // 16, 16, np.float32), g[f"analysis_{mode}"]) < 1e-5


@pytest.mark.parametrize("ratio,mode", [(2, "centered"), (3, "centered"), (2, "causal")])
def test_resampler_fixtures(golden, ratio, mode):
    """fir with rave_amd.resampler.design's taps and the stages' paddings
    (_FirStage, offline) against the reference's outputs; test_gpu_speaker.py's
    bound for the same fixtures."""
    from rave_amd.config import get_padding as stage_padding
    from rave_amd.resampler import design
    g = golden("resampler")
    r, down, up = design(48000 * ratio, 48000)
    assert r == ratio
    assert np.array_equal(down, g[f"r{ratio}_{mode}/down_w"][:, 0])
    assert np.array_equal(up, g[f"r{ratio}_{mode}/up_w"][:, 0])
    x = g["x"][:, 0]
    for taps, stride, key in ((down, ratio, "down"), (up, 1, "up")):
        pad = stage_padding(taps.shape[1], stride, causal=mode == "causal")
        t_out = (x.shape[-1] + pad[0] + pad[1] - taps.shape[1]) // stride + 1
        want = g[f"r{ratio}_{mode}/{key}"][:, 0]
        got = F.fir(x, taps, stride, pad[0], t_out)
        assert got.shape == want.shape
        assert maxabs(got, want) < 1e-5
        assert maxabs(F.fir(x, taps, stride, pad[0], t_out, np.float32), want) < 1e-5


# ------------------------------------------------------------------ streaming identity
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_streaming_blocks_equal_the_one_shot_causal_synthesis(filters, mode):
    """[32 history columns | block], pad_left 0, x_len 32 + T, frame0 = block
    start - 32, for blocks of 1, 37, 128 and 134 frames (starts 0, 1, 38, 166:
    frame0 of both parities): the concatenation is the causal one-shot call."""
    _, hki = filters
    x, noise = F.stream_signal()
    if mode == 0:
        noise = np.zeros_like(noise)
    whole = F.synthesis(x, hki, 32, mode, 0, 0, noise, F.STREAM_FRAMES)
    parts = [F.synthesis(xb, hki, 0, mode, s - F.STREAM_HIST, F.STREAM_HIST + T, nb, T)
             for s, T, xb, nb in F.stream_blocks(x, noise)]
    assert {(s - F.STREAM_HIST) % 2 for s, *_ in F.stream_blocks(x, noise)} == {0, 1}
    got = np.concatenate(parts, -1)
    assert got.shape == whole.shape
    assert maxabs(got, whole) <= 1e-12 * np.abs(whole).max()
    # the parity is what frame0 is for: without it the odd-start blocks differ
    s, T, xb, nb = F.stream_blocks(x, noise)[1]
    assert (s - F.STREAM_HIST) % 2 == 1
    wrong = F.synthesis(xb, hki, 0, mode, 0, F.STREAM_HIST + T, nb, T)
    assert maxabs(wrong, parts[1]) > 1e-3


# ------------------------------------------------------------------ impulse identities
@pytest.mark.parametrize("pad_left", [256, 512, 0])
def test_analysis_impulse_closed_form(filters, pad_left):
    hkf, _ = filters
    t_out, t_in = 40, 700
    for s in (0, 1, 255, 256, 257, 511, 512, t_in - 1):
        x = np.zeros((1, t_in), np.float32)
        x[0, s] = 1.0
        want = F.analysis_impulse(hkf, s, pad_left, t_out, 16)
        for dt in (np.float64, np.float32):
            assert np.array_equal(F.analysis(x, hkf, pad_left, t_out, 16, dt)[0], want), (s, dt)
        assert np.array_equal(F.analysis_impulse(hkf, s, pad_left, t_out, 6), want[:6])
    # the 513th tap is a row entry like any other (a zero in this prototype, so a probe filter shows it)
    probe = np.arange(16 * 513, dtype=np.float32).reshape(16, 513) + 1
    sign = np.where(np.arange(16) % 2 == 1, -1.0, 1.0)                   # frame 0 is even
    assert np.array_equal(F.analysis_impulse(probe, 0, 512, 1, 16)[:, 0], sign * probe[:, 512])
    assert np.array_equal(F.analysis_impulse(probe, 15, 512, 2, 16)[:, 1], probe[:, 511])


@pytest.mark.parametrize("pad_left,frame0", [(16, 0), (32, 7), (0, -32), (0, -31)])
def test_synthesis_impulse_closed_form(filters, pad_left, frame0):
    _, hki = filters
    t_in = 50
    xl = t_in + (32 if pad_left == 0 else 0)
    for c in (0, 1, 14, 15):
        for f in (0, 1, 31, 32, 33, xl - 1):
            x = np.zeros((1, 16, xl), np.float32)
            x[0, c, f] = 1.0
            want = F.synthesis_impulse(hki, c, f, pad_left, frame0, t_in)
            for dt in (np.float64, np.float32):
                got = F.synthesis(x, hki, pad_left, 0, frame0, xl if pad_left == 0 else 0, None, t_in, dt)[0]
                assert np.array_equal(got, want), (c, f, dt)


def test_fir_impulse_closed_form():
    rng = np.random.default_rng(0)
    for P, K, S, pad in ((1, 39, 2, 19), (2, 21, 1, 10), (3, 19, 1, 0), (1, 57, 64, 56)):
        h = rng.standard_normal((P, K)).astype(np.float32)
        t_in, t_out = 400, 30
        for s in (0, 1, K - 1, K, t_in - 1):
            x = np.zeros((1, t_in), np.float32)
            x[0, s] = 1.0
            want = F.fir_impulse(h, s, S, pad, t_out)
            for dt in (np.float64, np.float32):
                assert np.array_equal(F.fir(x, h, S, pad, t_out, dt)[0], want), (P, s, dt)


# ------------------------------------------------------------------ the fp32 runs are chains
def test_fp32_step_is_a_fused_multiply_add():
    """The fp32 step against the exactly rounded a b + c in rational arithmetic
    (nearest fp32 of the exact value), on products that cancel against c so
    that a separately rounded product would show."""
    from fractions import Fraction
    rng = np.random.default_rng(24)
    a = rng.standard_normal(500).astype(np.float32)
    b = rng.standard_normal(500).astype(np.float32)
    c = (-(a * b) * (1 + rng.integers(-3, 4, 500) * np.float32(2.0 ** -20))).astype(np.float32)
    got = F._fma(a.astype(np.float64), b.astype(np.float64), c)
    assert got.dtype == np.float32
    split = 0
    for ai, bi, ci, gi in zip(a, b, c, got):
        exact = Fraction(float(ai)) * Fraction(float(bi)) + Fraction(float(ci))
        near = np.float32(float(exact))
        cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
        best = min(abs(Fraction(float(v)) - exact) for v in cands)
        assert abs(Fraction(float(gi)) - exact) == best, (ai, bi, ci, gi)
        split += np.float32(ai * bi) + ci != gi
    assert split > 100                      # multiply-then-add is another arithmetic on these
def test_fp32_runs_hold_every_intermediate_in_fp32(filters):
    """e_ref is only worth something if the fp32 run rounds after every step:
    a float64 accumulation rounded once at the end would be far closer."""
    hkf, hki = filters
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 16 * 64)).astype(np.float32)
    r64, e = F.with_e_ref(F.analysis, x, hkf, 256, 64, 16)
    once = maxabs(r64.astype(np.float32), r64)
    assert e > 2 * once > 0
    w = rng.standard_normal((2, 32, 64)).astype(np.float32)
    r64, e = F.with_e_ref(F.synthesis, w, hki, 16, 1, 0, 0, None, 64)
    assert e > 2 * maxabs(r64.astype(np.float32), r64) > 0
    h = rng.standard_normal((2, 21)).astype(np.float32)
    r64, e = F.with_e_ref(F.fir, x, h, 1, 10, 500)
    assert e > 2 * maxabs(r64.astype(np.float32), r64) > 0
