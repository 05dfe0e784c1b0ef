"""Host-side checks of the differentiable spectral losses (no GPU: nothing here
launches): the new exports and struct, the argument checks of
rave_stft_loss_workspace / _forward / _backward and the table packer, the fork's
resolutions, the Python wrappers' refusals, and the CPU reference
(tests/stft_loss_ref.py) against a direct DFT evaluation of the definition."""
import ctypes as C

import numpy as np
import pytest
import torch

from rave_amd import _native as N
from tests import stft_loss_ref as R

NEW = ["rave_stft_loss_table_size", "rave_stft_loss_pack_table", "rave_stft_loss_workspace",
       "rave_stft_loss_forward", "rave_stft_loss_backward"]


def _args(rows=2, t=5000, res=((2048, 220, 1102), (4096, 441, 2205), (512, 88, 441)), kind=None, eps=1e-7):
    a = N.StftLossArgs(rows=rows, t_len=t, n_res=len(res), kind=N.STFT_LOSS_MULTIRES if kind is None else kind,
                       log_epsilon=eps)
    for i, (n, h, w) in enumerate(res[:N.STFT_MAX_SCALES]):
        a.n_fft[i], a.hop[i], a.win[i] = n, h, w
    return a


def test_exports_struct_and_abi():
    for name in NEW:
        assert name in N.EXPORTS and hasattr(N.lib, name)
    assert N.ABI_VERSION == N.lib.rave_abi_version() == 21
    n = N.lib.rave_struct_sizes(None, 0)
    buf = (C.c_int64 * n)()
    N.lib.rave_struct_sizes(buf, n)
    assert N.STRUCTS[-1] is N.StftLossArgs and buf[n - 1] == C.sizeof(N.StftLossArgs)
    # 4 + 3 * 8 + 2 ints, 8 + 7 pointers
    assert C.sizeof(N.StftLossArgs) == 4 * 30 + 8 * 15


def test_workspace_size():
    """4 floats per workgroup (rows * ceil(frames / tile), tile = 4 transforms for
    n_fft <= 1024 times 1024 / n_fft frames at once, 2 above) and rows * frames *
    win floats of windowed frame gradients per resolution."""
    rows, t = 3, 5000
    res = ((2048, 220, 1102), (4096, 441, 2205), (512, 88, 441), (64, 5, 37))
    floats = 0
    for n, hop, win in res:
        frames = 1 + t // hop
        tile = max(1, 1024 // n) * (4 if n <= 1024 else 2)
        floats += 4 * rows * -(-frames // tile) + rows * frames * win
    assert N.lib.rave_stft_loss_workspace(C.byref(_args(rows, t, res))) == 4 * floats


@pytest.mark.parametrize("why,kw", [
    ("n_fft/2 >= T", dict(t=2048)),
    ("win > n_fft", dict(res=((512, 88, 513),))),
    ("win < 1", dict(res=((512, 88, 0),))),
    ("hop < 1", dict(res=((512, 0, 441),))),
    ("n_fft no power of two", dict(res=((1000, 88, 441),))),
    ("n_fft below 64", dict(res=((32, 8, 32),))),
    ("n_fft above 4096", dict(res=((8192, 8, 32),), t=20000)),
    ("no resolution", dict(res=())),
    ("a bad kind", dict(kind=2)),
    ("V1 without a positive epsilon", dict(kind=N.STFT_LOSS_V1, eps=0.0)),
    ("no rows", dict(rows=0)),
])
def test_argument_checks(why, kw):
    a = _args(**kw)
    a.target = a.value = a.workspace = a.out = a.saved = a.grad_out = a.grad_value = 16
    for i in range(N.STFT_MAX_SCALES):
        a.tables[i] = 16
    assert N.lib.rave_stft_loss_workspace(C.byref(a)) == -1, why
    assert N.lib.rave_last_error().decode().startswith("stft_loss")
    # refused before any launch: no GPU is touched here
    assert N.lib.rave_stft_loss_forward(C.byref(a), None) == N.RAVE_ERR_ARG, why
    assert N.lib.rave_stft_loss_backward(C.byref(a), None) == N.RAVE_ERR_ARG, why


def test_too_many_resolutions():
    a = _args(res=((512, 88, 441),))
    a.n_res = N.STFT_MAX_SCALES + 1
    assert N.lib.rave_stft_loss_workspace(C.byref(a)) == -1
    assert N.lib.rave_stft_loss_forward(C.byref(a), None) == N.RAVE_ERR_ARG
    from rave_amd.distance import MultiResolutionSTFTLoss
    with pytest.raises(ValueError):
        MultiResolutionSTFTLoss([(512, 88, 441)] * (N.STFT_MAX_SCALES + 1))


def test_null_pointers_are_refused():
    a = _args()
    assert N.lib.rave_stft_loss_workspace(C.byref(a)) > 0          # pointers ignored
    with pytest.raises(ValueError):
        N.check(N.lib.rave_stft_loss_forward(C.byref(a), None), "stft_loss_forward")
    a.target = a.value = a.workspace = a.out = a.saved = 16
    for i in range(3):
        a.tables[i] = 16
    assert N.lib.rave_stft_loss_backward(C.byref(a), None) == N.RAVE_ERR_ARG      # grad_out, grad_value
    a.tables[2] = None
    assert N.lib.rave_stft_loss_forward(C.byref(a), None) == N.RAVE_ERR_ARG


def test_pack_table():
    n, win = 64, 37
    assert N.lib.rave_stft_loss_table_size(n, win) == 2 * n + win
    tab = N.pack_stft_loss_table(n, win)
    k = np.arange(n)
    np.testing.assert_array_equal(tab[0:2 * n:2], np.cos(2 * np.pi / n * k).astype(np.float32))
    np.testing.assert_array_equal(tab[1:2 * n:2], (-np.sin(2 * np.pi / n * k)).astype(np.float32))
    want = torch.hann_window(win, dtype=torch.float64).numpy()
    assert np.abs(tab[2 * n:] - want).max() <= 2 ** -24
    # win = n_fft: the window of rave_stft_pack_table
    np.testing.assert_array_equal(N.pack_stft_loss_table(256, 256)[512:], N.pack_stft_table(256)[:256])
    for bad in ((64, 65), (64, 0), (100, 50), (8192, 64)):
        assert N.lib.rave_stft_loss_table_size(*bad) == -1
        with pytest.raises(ValueError):
            N.pack_stft_loss_table(*bad)


def test_for_sample_rate():
    from rave_amd.distance import MultiResolutionSTFTLoss
    fork = ((2048, 220, 1102), (4096, 441, 2205), (512, 88, 441))
    assert MultiResolutionSTFTLoss.for_sample_rate(44100).resolutions == fork
    assert MultiResolutionSTFTLoss.for_sample_rate().resolutions == fork
    assert R.fork_resolutions() == fork


def test_wrappers_refuse_bad_inputs():
    import rave_amd
    from rave_amd.distance import AudioDistance
    loss = rave_amd.MultiResolutionSTFTLoss([(64, 5, 37)])
    x = torch.zeros(2, 300)
    with pytest.raises(ValueError, match="target is constant"):
        loss(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="target is constant"):
        AudioDistance((64,))(x[:, None].clone().requires_grad_(True), x[:, None])
    with pytest.raises(ValueError, match="float32 CUDA"):
        loss(x, x)                                       # a CPU tensor
    with pytest.raises(ValueError, match="float32 CUDA"):
        loss(x.double(), x.double())
    with pytest.raises(ValueError, match="float32 CUDA"):
        loss(x.numpy(), x.numpy())
    with pytest.raises(ValueError):
        AudioDistance((64,))(x[:, None], x[:, None].clone().requires_grad_(True))     # CPU, on the new path
    meta = torch.zeros(2, 300, device="meta")
    with pytest.raises(ValueError):
        loss(meta, meta)


def test_reference_matches_the_definition():
    """The torch.stft restatement against a direct float64 DFT of the definition
    on an odd geometry: window offset (64 - 37) // 2 = 13, 1 + 100 // 5 frames."""
    pred, target = R.synth(2, 100, 300)
    n_fft, hop, win = 64, 5, 37
    (sc, mag), = R.mr_terms(torch.from_numpy(pred).double(), torch.from_numpy(target).double(), ((n_fft, hop, win),))
    wsc, wmag = R.dft_terms(pred, target, n_fft, hop, win)
    assert R.mr_mag(torch.from_numpy(pred).double(), n_fft, hop, win).shape == (2, 21, 33)
    assert abs(float(sc) - wsc) <= 1e-12 * wsc
    assert abs(float(mag) - wmag) <= 1e-12 * wmag
    # a window as long as the FFT and an even offset
    for geo in ((64, 16, 64), (128, 7, 100)):
        (sc, mag), = R.mr_terms(torch.from_numpy(pred).double(), torch.from_numpy(target).double(), (geo,))
        wsc, wmag = R.dft_terms(pred, target, *geo)
        assert abs(float(sc) - wsc) <= 1e-12 * wsc and abs(float(mag) - wmag) <= 1e-12 * wmag
