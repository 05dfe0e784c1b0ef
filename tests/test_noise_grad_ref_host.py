"""tests/noise_grad_ref.py against float64 torch autograd on the CPU: the
closed-form backward of the noise filter stage against autograd through the
torch.fft restatement of tests/aux_ref.noise_synth (which is itself pinned to
aux_ref's numpy forward here), for the three compiled (noise_bands, target)
pairs; the closed-form AdaIN backward against autograd through aux_ref's AdaIN
with the statistics as constants, in every mode with the counters zero and
non-zero.  Agreement: 1e-12 of the gradient's max.  And the C ABI the two
kernels add: version 21, the symbols, the struct sizes and their place in
STRUCTS.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import aux_ref as R, noise_grad_ref as G


def _noise_case(nb, tgt, frames=7, n_band=3, B=2, seed=0):
    rng = np.random.default_rng(seed + 100 * nb + tgt)
    amp = rng.standard_normal((B, n_band * nb, frames)) * 3 + 4
    u = rng.uniform(0, 1, (B, frames, n_band, tgt))
    gy = rng.standard_normal((B, n_band, frames * tgt))
    return amp, u, gy, n_band


@pytest.mark.parametrize("nb,tgt", G.PAIRS)
def test_torch_restatement_is_aux_refs_forward(nb, tgt):
    amp, u, _, n_band = _noise_case(nb, tgt)
    want = R.noise_synth(amp, u, n_band, nb, tgt)
    got = G.noise_synth_torch(torch.from_numpy(amp), torch.from_numpy(u), n_band, nb, tgt).numpy()
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("nb,tgt", G.PAIRS)
def test_noise_closed_form_vs_float64_autograd(nb, tgt):
    amp, u, gy, n_band = _noise_case(nb, tgt)
    a = torch.from_numpy(amp).requires_grad_(True)
    G.noise_synth_torch(a, torch.from_numpy(u), n_band, nb, tgt).backward(torch.from_numpy(gy))
    want = a.grad.numpy()
    got = G.noise_synth_backward(gy, amp, u, n_band, nb, tgt)
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"noise backward ({nb}, {tgt}): max {top:.3e} err {err:.3e}")
    assert got.shape == amp.shape and top > 0 and err <= 1e-12 * top


def test_noise_closed_form_keeps_its_digits_at_large_amp():
    """amp in [20, 30]: 1 - s is about e^-(amp - 5), which the closed form takes
    from sigmoid(5 - amp); the fp32 run keeps a relative error of fp32 size,
    where 1 - s by subtraction would give 0 (s rounds to 1)."""
    nb, tgt = 5, 8
    _, u, gy, n_band = _noise_case(nb, tgt)
    amp = np.random.default_rng(1).uniform(20, 30, (2, n_band * nb, 7))
    want = G.noise_synth_backward(gy, amp, u, n_band, nb, tgt)
    a = torch.from_numpy(amp).requires_grad_(True)
    G.noise_synth_torch(a, torch.from_numpy(u), n_band, nb, tgt).backward(torch.from_numpy(gy))
    # float64 autograd subtracts (s (1 - s)) and still has ~1e-16 / e^-25 digits: a loose cross-check
    assert np.abs(a.grad.numpy() - want).max() <= 1e-4 * np.abs(want).max()
    got32 = G.noise_synth_backward(gy.astype(np.float32), amp.astype(np.float32), u.astype(np.float32), n_band, nb, tgt,
                                   np.float32)
    assert got32.dtype == np.float32 and np.abs(want).max() > 0
    assert np.abs(got32 - want).max() <= 1e-4 * np.abs(want).max()
    # mid-range, amp = 25: e^-20 = 2e-9 is below fp32's 2^-24 next to 1
    assert (np.float32(1) - np.float32(1) / (np.float32(1) + np.exp(-np.float32(25 - 5)))) == 0


@pytest.mark.parametrize("counters", [(0, 0), (1, 0), (0, 1), (3, 2)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_adain_closed_form_vs_float64_autograd(mode, counters):
    rng = np.random.default_rng(10 * mode + counters[0])
    B, Cc, T, MB, row0 = 3, 5, 33, 8, 2
    x = torch.from_numpy(rng.standard_normal((B, Cc, T)) * 1.7 + 0.3).requires_grad_(True)
    stats = torch.from_numpy(rng.standard_normal((4, MB, Cc)))
    stats[1], stats[3] = stats[1].abs() + 0.1, stats[3].abs() + 0.1
    gy = rng.standard_normal((B, Cc, T))
    y, st, cnt = G.adain_torch(x, stats, list(counters), mode, row0)
    y64, st64, cnt64 = R.adain(x.detach(), stats, list(counters), mode, row0)
    assert torch.equal(y.detach(), y64) and torch.equal(st, st64) and cnt == cnt64   # the same forward
    y.backward(torch.from_numpy(gy))
    want = x.grad.numpy()
    got = G.adain_backward(gy, st.numpy(), cnt, mode, row0)
    transfers = mode != 2 and cnt[0] != 0 and cnt[1] != 0
    assert transfers == G.adain_transfers(cnt, mode)
    assert transfers == {0: counters == (3, 2), 1: counters[1] != 0, 2: False}[mode]
    if transfers:
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    else:
        assert np.array_equal(got, gy) and np.array_equal(want, gy)
    got32 = G.adain_backward(gy.astype(np.float32), st.numpy().astype(np.float32), cnt, mode, row0, np.float32)
    assert got32.dtype == np.float32


def test_abi_symbols_and_struct_sizes():
    from rave_amd import _native as N
    assert N.ABI_VERSION == N.lib.rave_abi_version() == 21
    for name in ("rave_noise_synth_backward", "rave_adain_backward"):
        assert name in N.EXPORTS and hasattr(N.lib, name)
    n = N.lib.rave_struct_sizes(None, 0)
    buf = (C.c_int64 * n)()
    N.lib.rave_struct_sizes(buf, n)
    assert n == len(N.STRUCTS)
    sizes = dict(zip(N.STRUCTS, buf))
    # the forward's fields with (gy, 2 strides) and (gamp, 2 strides) for (y, 2 strides)
    assert sizes[N.NoiseBackwardArgs] == C.sizeof(N.NoiseBackwardArgs) == C.sizeof(N.NoiseArgs) + 24 == 112
    # the forward's fields without the ticket word
    assert sizes[N.AdainBackwardArgs] == C.sizeof(N.AdainBackwardArgs) == C.sizeof(N.AdainArgs) - 8 == 88
    i_n, i_a, i_l = (N.STRUCTS.index(s) for s in (N.NoiseBackwardArgs, N.AdainBackwardArgs, N.StftLossArgs))
    assert (i_n, i_a, i_l) == (n - 3, n - 2, n - 1)
    assert N.lib.rave_noise_synth_backward.argtypes[0]._type_ is N.NoiseBackwardArgs
    assert N.lib.rave_adain_backward.argtypes[0]._type_ is N.AdainBackwardArgs


def test_refusals_need_no_gpu():
    """Argument checks come before any launch, in the forward's order and with its texts."""
    from rave_amd import _native as N
    one = (C.c_float * 1)()
    p = C.cast(one, C.c_void_p)

    def noise(**kw):
        base = dict(batch=1, frames=4, n_band=3, noise_bands=5, target=8, amp=p, u=p, gy=p, gamp=p)
        base.update(kw)
        return N.lib.rave_noise_synth_backward(C.byref(N.NoiseBackwardArgs(**base)), None)

    for kw, status, text in [(dict(gy=None), N.RAVE_ERR_ARG, "null pointer"),
                             (dict(gamp=None), N.RAVE_ERR_ARG, "null pointer"),
                             (dict(amp=None), N.RAVE_ERR_ARG, "null pointer"),
                             (dict(u=None), N.RAVE_ERR_ARG, "null pointer"),
                             (dict(frames=0), N.RAVE_ERR_ARG, "empty shape"),
                             (dict(frames=0, target=7), N.RAVE_ERR_ARG, "empty shape"),
                             (dict(target=7), N.RAVE_ERR_ARG, "target must be >= 2*(noise_bands-1)"),
                             (dict(noise_bands=9, target=8), N.RAVE_ERR_ARG, "target must be >= 2*(noise_bands-1)"),
                             (dict(target=12), N.RAVE_ERR_UNSUPPORTED, "supported (noise_bands, target) are (5, 8), (5, 16), (9, 16)"),
                             (dict(noise_bands=7, target=16), N.RAVE_ERR_UNSUPPORTED, "supported (noise_bands, target)")]:
        assert noise(**kw) == status, kw
        assert text in N.lib.rave_last_error().decode(), kw

    def ada(**kw):
        base = dict(batch=3, channels=5, t_len=16, mode=0, max_batch=8, row0=0, gy=p, gx=p, stats=p, counters=p)
        base.update(kw)
        return N.lib.rave_adain_backward(C.byref(N.AdainBackwardArgs(**base)), None)

    for kw, text in [(dict(gy=None), "null pointer"), (dict(gx=None), "null pointer"), (dict(stats=None), "null pointer"),
                     (dict(counters=None), "null pointer"), (dict(t_len=0), "empty shape"), (dict(mode=3), "mode must be"),
                     (dict(row0=6), "batch exceeds the statistics buffers"), (dict(row0=-1), "batch exceeds")]:
        assert ada(**kw) == N.RAVE_ERR_ARG, kw
        assert text in N.lib.rave_last_error().decode(), kw
