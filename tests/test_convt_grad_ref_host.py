"""tests/convt_grad_ref.py against float64 torch autograd and the adjoint identity
(no GPU), and the host-side refusals of the conv_transpose1d backward's C boundary."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convt_grad_ref as G
from tests.test_conv_grad_ref_host import _torch_act

CASES = [(r, act, B) for r in G.STRIDES for act in (G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE) for B in (1, 3)]


def _data(r, act, B=2, c_in=5, c_out=6, t_in=9, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c_in, t_in))
    x[0, 0, :3] = 0.0                                       # exact zeros: LeakyReLU's x <= 0 side
    w = rng.standard_normal((c_in, c_out, 2 * r))
    bias = rng.standard_normal(c_out)
    res = rng.standard_normal((B, c_out, t_in * r))
    gy = rng.standard_normal((B, c_out, t_in * r))
    alpha = rng.uniform(0.1, 3.0, c_in)
    alpha[-1] = 0.0
    return dict(x=x, w=w, bias=bias, res=res, gy=gy, alpha=alpha, r=r, act=act, slope=0.2, t_in=t_in)


def _close(a, b):
    b = np.asarray(b)
    return np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("r,act,B", CASES)
def test_reference_matches_float64_autograd(r, act, B):
    c = _data(r, act, B=B)
    x = torch.tensor(c["x"], requires_grad=True)
    w = torch.tensor(c["w"], requires_grad=True)
    bias = torch.tensor(c["bias"], requires_grad=True)
    res = torch.tensor(c["res"], requires_grad=True)
    alpha = torch.tensor(c["alpha"], requires_grad=True)
    y = F.conv_transpose1d(_torch_act(x, act, c["slope"], alpha), w, bias, stride=r, padding=r // 2) + res
    y.backward(torch.tensor(c["gy"]))
    yref = G.forward(c["x"], c["w"], c["bias"], c["alpha"], c["res"], r, act, c["slope"])
    assert yref.shape == (B, 6, c["t_in"] * r) and _close(yref, y.detach().numpy())
    flat = G.backward(c["gy"], c["x"], c["w"], c["alpha"], r, act, c["slope"])
    gx, gw, gb, ga = G.split(flat, B, 5, 6, c["t_in"], r, act)
    assert _close(gx, x.grad.numpy()) and _close(gw, w.grad.numpy()) and _close(gb, bias.grad.numpy())
    assert np.array_equal(res.grad.numpy(), c["gy"])        # the residual's gradient is gy itself
    if act == G.ACT_SNAKE:
        assert _close(ga, alpha.grad.numpy())
        assert c["alpha"][-1] == 0.0 and np.isfinite(ga).all()
    else:
        assert ga is None


@pytest.mark.parametrize("r", G.STRIDES)
def test_reference_adjoint_identity(r):
    """<gy, J dx> = <J^T gy, dx> of the linear map a -> y (bias and residual off)."""
    c = _data(r, G.ACT_SNAKE, seed=3)
    a = G.act_fwd(c["x"], c["act"], c["slope"], c["alpha"], np.float64)
    y = G.forward(a, c["w"], None, None, None, r, G.ACT_NONE, 0.2)
    flat = G.backward(c["gy"], a, c["w"], None, r, G.ACT_NONE, 0.2)
    ga = G.split(flat, *a.shape[:2], c["w"].shape[1], c["t_in"], r, G.ACT_NONE)[0]
    lhs, rhs = float((y * c["gy"]).sum()), float((a * ga).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs))


def test_with_e_ref_is_per_output():
    c = _data(4, G.ACT_SNAKE)
    r64, e = G.with_e_ref(c["gy"], c["x"], c["w"], c["alpha"], 4, c["act"], 0.2)
    assert len(r64) == 4 and len(e) == 4 and all(0 < v < 1e-4 for v in e)


# ------------------------------------------------------------------ C boundary, host side
NAMES = ("rave_conv_transpose1d_backward_workspace", "rave_conv_transpose1d_backward_data",
         "rave_conv_transpose1d_backward_weight")


def _args(N, **kw):
    a = N.ConvBackwardArgs()
    a.c_in, a.c_out, a.kernel, a.stride, a.dilation = 16, 16, 4, 2, 1
    a.transposed, a.out_shift, a.batch, a.t_in, a.t_out = 1, 1, 1, 32, 64
    a.leaky_slope = 0.2
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_and_abi():
    from rave_amd import _native as N
    for name in NAMES:
        assert name in N.EXPORTS and hasattr(N.lib, name)
    assert N.ABI_VERSION == 21 and N.lib.rave_abi_version() == 21
    assert N.ConvBackwardArgs in N.STRUCTS and C.sizeof(N.ConvBackwardArgs) == 184


def test_host_refusals():
    from rave_amd import _native as N
    fns = [getattr(N.lib, n) for n in NAMES]

    def refused(a, status, word):
        for fn in fns:
            rc = fn(C.byref(a)) if fn is fns[0] else fn(C.byref(a), None)
            text = N.lib.rave_last_error().decode()
            assert rc == status and word in text, (rc, text)

    assert N.lib.rave_conv_transpose1d_backward_workspace(C.byref(_args(N))) == 0
    refused(_args(N, transposed=0), N.RAVE_ERR_ARG, "transposed")
    refused(_args(N, kernel=3), N.RAVE_ERR_ARG, "kernel")
    refused(_args(N, kernel=8), N.RAVE_ERR_ARG, "kernel")
    refused(_args(N, pad_left=1, out_shift=0, t_in=33), N.RAVE_ERR_ARG, "pad_left")
    refused(_args(N, out_shift=0), N.RAVE_ERR_ARG, "out_shift")
    for prec in (1, 4, 5):
        refused(_args(N, precision=prec), N.RAVE_ERR_ARG, "precision")
    refused(_args(N, kernel=16, stride=8, out_shift=4, t_out=256), N.RAVE_ERR_UNSUPPORTED, "stride")
    refused(_args(N, kernel=6, stride=3, out_shift=1, t_out=96), N.RAVE_ERR_UNSUPPORTED, "stride")
    refused(_args(N, t_out=63), N.RAVE_ERR_ARG, "t_out")
    refused(_args(N, act=2), N.RAVE_ERR_ARG, "alpha")
    # a missing x where the activation's derivative or gweight needs it (dummy non-null pointers: refused before any launch)
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    rc = N.lib.rave_conv_transpose1d_backward_data(C.byref(_args(N, act=1, gy=p, weight=p, gx=p)), None)
    assert rc == N.RAVE_ERR_ARG and "needs the input x" in N.lib.rave_last_error().decode()
    rc = N.lib.rave_conv_transpose1d_backward_weight(C.byref(_args(N, gy=p, weight=p, gweight=p)), None)
    assert rc == N.RAVE_ERR_ARG and "needs the input x" in N.lib.rave_last_error().decode()
    # the non-transposed entry points keep refusing transposed = 1
    rc = N.lib.rave_conv1d_backward_data(C.byref(_args(N)), None)
    assert rc == N.RAVE_ERR_ARG and "transposed" in N.lib.rave_last_error().decode()


def test_switch_is_off_by_default_and_read_at_construction():
    from rave_amd import cc
    assert cc.ConvTranspose1d(16, 8, 8, stride=4, padding=2).differentiable is False
    cc.use_transposed_grad(True)
    try:
        on = cc.ConvTranspose1d(16, 8, 8, stride=4, padding=2)
    finally:
        cc.use_transposed_grad(False)
    assert on.differentiable is True and cc.ConvTranspose1d(16, 8, 8, stride=4, padding=2).differentiable is False
    assert torch.ops.rave_amd.conv_transpose1d_w and torch.ops.rave_amd.conv_transpose1d_backward
