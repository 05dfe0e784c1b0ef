"""tests/pqmf_grad_ref.py on the CPU: the adjoint identity <A x, g> = <x, A^T g>
against the forward restatements of tests/filterbank_ref.py in float64, the
float64 restatement against CPU float64 torch autograd through the oracle's
PQMF forward and inverse (oracle/torch_cpu.py's expressions, the inverse behind
the mode 1 / mode 2 head written in torch), the closed forms the GPU test
compares impulses with, and the new exports and structs (no launch).

Bound 1e-11 relative: the sums have at most 528 terms in float64, so rounding
is about 6e-14."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle.rave_oracle import get_padding
from oracle.torch_cpu import TorchCPURave
from tests import filterbank_ref as F
from tests import pqmf_grad_ref as G

REL = 1e-11


@pytest.fixture(scope="module")
def filters(golden):
    from rave_amd.pqmf import kernels
    hkf, hki = kernels(golden("pqmf")["hk"])
    assert hkf.shape == (16, 513) and hki.shape == (16, 16, 33)
    return hkf, hki


def test_exports_and_structs():
    from rave_amd import _native as N
    for name in ("rave_pqmf_synthesis_backward", "rave_pqmf_analysis_backward"):
        assert name in N.EXPORTS and hasattr(N.lib, name)
    n = N.lib.rave_struct_sizes(None, 0)
    buf = (C.c_int64 * n)()
    N.lib.rave_struct_sizes(buf, n)
    sizes = dict(zip(N.STRUCTS, buf))
    assert sizes[N.SynthesisBackwardArgs] == C.sizeof(N.SynthesisBackwardArgs) == 4 * 10 + 8 * 15
    assert sizes[N.AnalysisBackwardArgs] == C.sizeof(N.AnalysisBackwardArgs) == 4 * 8 + 8 * 6
    # refused before any launch (no GPU needed): NULL pointers
    assert N.lib.rave_pqmf_synthesis_backward(C.byref(N.SynthesisBackwardArgs()), None) == N.RAVE_ERR_ARG
    assert N.lib.rave_pqmf_analysis_backward(C.byref(N.AnalysisBackwardArgs()), None) == N.RAVE_ERR_ARG


# ------------------------------------------------------------------ the adjoint identity
@pytest.mark.parametrize("t_out", [1, 17, 129])
@pytest.mark.parametrize("n_out", [6, 16])
@pytest.mark.parametrize("pad_left", [256, 0])
def test_analysis_adjoint_identity(filters, pad_left, n_out, t_out):
    hkf, _ = filters
    rng = np.random.default_rng(1000 * t_out + n_out + pad_left)
    for t_in in (16 * t_out, max(1, 16 * (t_out - 1) + 513 - pad_left - 207)):
        x = rng.standard_normal((2, t_in))
        g = rng.standard_normal((2, n_out, t_out))
        lhs = float((F.analysis(x, hkf, pad_left, t_out, n_out) * g).sum())
        gx = G.analysis_backward(g, hkf, pad_left, t_in, n_out)
        assert gx.shape == x.shape and gx.dtype == np.float64
        rhs = float((x * gx).sum())
        assert abs(lhs - rhs) <= REL * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize("t_in", [1, 17, 129])
@pytest.mark.parametrize("pad_left,x_extra,frame0", [(16, 0, 0), (16, 0, 7), (0, 32, -32)])
def test_synthesis_adjoint_identity(filters, pad_left, x_extra, frame0, t_in):
    _, hki = filters
    rng = np.random.default_rng(1000 * t_in + pad_left + frame0 + 50)
    x_len = t_in + x_extra if x_extra else 0
    n = x_len or t_in
    x = rng.standard_normal((2, 16, n))
    g = rng.standard_normal((2, 16 * t_in))
    y = F.synthesis(x, hki, pad_left, 0, frame0, x_len, None, t_in)
    gx = G.synthesis_backward(g, None, hki, pad_left, 0, frame0, x_len, None, t_in)
    assert gx.shape == x.shape and gx.dtype == np.float64
    lhs, rhs = float((y * g).sum()), float((x * gx).sum())
    assert abs(lhs - rhs) <= REL * abs(lhs), (lhs, rhs)


# ------------------------------------------------------------------ against torch autograd
B, FRAMES = 2, 300


def _oracle_forward(x, hkf, causal, n_out):
    """CachedPQMF.forward as TorchCPURave.encode writes it."""
    k = hkf.shape[-1]
    bands = TF.conv1d(TF.pad(x[:, None], get_padding(k, causal=causal)), hkf[:, None], stride=16)
    return TorchCPURave._reverse_half(bands)[:, :n_out]


def _oracle_inverse(y, hki, causal):
    """CachedPQMF.inverse as TorchCPURave.decode writes it; y (B, 16, F) -> (B, 16 F)."""
    k = hki.shape[-1]
    y = TorchCPURave._reverse_half(y)
    y = TF.conv1d(TF.pad(y, get_padding(k, causal=causal)), hki) * 16
    y = y.flip(1)
    return y.permute(0, 2, 1).reshape(y.shape[0], -1)


def _head(x, mode, noise):
    """GeneratorV2's epilogue in torch (oracle/torch_cpu.py:122-125 with the noise added)."""
    if mode == 0:
        return x
    v = x[:, :16] * torch.sigmoid(x[:, 16:]) if mode == 1 else x
    if noise is not None:
        v = v + noise
    return torch.tanh(v)


def _close(got, want):
    want = want.detach().numpy()
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= REL * float(np.abs(want).max())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("n_out", [6, 16])
def test_analysis_backward_equals_autograd(filters, causal, n_out):
    hkf, _ = filters
    rng = np.random.default_rng(n_out + causal)
    x = torch.from_numpy(rng.standard_normal((B, 16 * FRAMES))).requires_grad_(True)
    g = rng.standard_normal((B, n_out, FRAMES))
    y = _oracle_forward(x, torch.from_numpy(hkf).double(), causal, n_out)
    want, = torch.autograd.grad(y, x, torch.from_numpy(g))
    pad = get_padding(513, causal=causal)[0]
    _close(G.analysis_backward(g, hkf, pad, 16 * FRAMES, n_out), want)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("mode,with_noise", [(0, False), (1, True), (1, False), (2, True), (2, False)])
def test_synthesis_backward_equals_autograd(filters, mode, with_noise, causal):
    _, hki = filters
    rng = np.random.default_rng(10 * mode + with_noise + 2 * causal)
    x = torch.from_numpy(rng.standard_normal((B, 32 if mode == 1 else 16, FRAMES))).requires_grad_(True)
    nz = torch.from_numpy(0.1 * rng.standard_normal((B, 16, FRAMES))).requires_grad_(True) if with_noise else None
    g = rng.standard_normal((B, 16 * FRAMES))
    y = _oracle_inverse(_head(x, mode, nz), torch.from_numpy(hki).double(), causal)
    want = torch.autograd.grad(y, [x] + ([nz] if with_noise else []), torch.from_numpy(g))
    pad = get_padding(33, causal=causal)[0]
    out = G.synthesis_backward(g, x.detach().numpy(), hki, pad, mode, 0, 0,
                               nz.detach().numpy() if with_noise else None, FRAMES)
    gx, gn = G.split(out, mode, with_noise)
    _close(gx, want[0])
    if with_noise:
        _close(gn, want[1])


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("pad_left", [256, 512, 0])
def test_analysis_backward_impulse_closed_form(filters, pad_left):
    hkf, _ = filters
    t_out, t_in = 40, 16 * 40
    for k, t in ((0, 0), (1, 0), (5, 7), (15, 39), (3, 32)):
        g = np.zeros((1, 16, t_out), np.float32)
        g[0, k, t] = 1.0
        want = G.analysis_backward_impulse(hkf, k, t, pad_left, t_in)
        for dtype in (np.float32, np.float64):
            assert np.array_equal(G.analysis_backward(g, hkf, pad_left, t_in, 16, dtype)[0], want)


@pytest.mark.parametrize("frame0", [0, 7])
@pytest.mark.parametrize("pad_left,x_extra", [(16, 0), (32, 0), (0, 32)])
def test_synthesis_backward_impulse_closed_form(filters, pad_left, x_extra, frame0):
    _, hki = filters
    t_in = 40
    x_len = t_in + x_extra if x_extra else 0
    for s in (0, 15, 16 * 17 + 3, 16 * t_in - 1):
        g = np.zeros((1, 16 * t_in), np.float32)
        g[0, s] = 1.0
        want = G.synthesis_backward_impulse(hki, s, pad_left, frame0, x_len or t_in)
        for dtype in (np.float32, np.float64):
            got = G.synthesis_backward(g, None, hki, pad_left, 0, frame0, x_len, None, t_in, dtype)[0]
            assert np.array_equal(got, want)


def test_fp32_run_is_fp32_and_saturation_gives_exact_zeros(filters):
    _, hki = filters
    rng = np.random.default_rng(40)
    x = rng.standard_normal((2, 32, 20)).astype(np.float32)
    x[:, :16, ::3] = 40.0
    x[:, 16:, ::3] = 40.0
    x[:, :16, 1::3] = -40.0
    g = rng.standard_normal((2, 320)).astype(np.float32)
    out = G.synthesis_backward(g, x, hki, 16, 1, 0, 0, None, 20, np.float32)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    assert not out[:, :, ::3].any() and out[:, :, 2::3].any()
