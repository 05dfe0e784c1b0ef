"""tests/conv_grad_ref.py against float64 torch autograd and the adjoint identity
(no GPU), and the host-side refusals of the conv1d backward's C boundary."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_grad_ref as G

CASES = [(fam, pad, act) for fam in G.FAMILIES for pad in ("centred", "causal", "none", "tail")
         for act in (G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE)
         if not (pad == "tail" and fam[1] == 1)]


def _geometry(fam, pad, t_out):
    k, s, d = fam
    span = (k - 1) * d + 1
    pl, pr = {"centred": ((span - 1) // 2, span // 2), "causal": (span - 1, 0), "none": (0, 0), "tail": (0, 0)}[pad]
    t_in = (t_out - 1) * s + span - pl - pr
    if pad == "tail":
        t_in += s - 1                                       # columns no output reads
    return pl, pr, t_in


def _data(fam, pad, act, B=2, c_in=5, c_out=6, t_out=9, seed=0):
    k, s, d = fam
    pl, pr, t_in = _geometry(fam, pad, t_out)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c_in, t_in))
    x[0, 0, : min(3, t_in)] = 0.0                           # exact zeros: LeakyReLU's x <= 0 side
    w = rng.standard_normal((c_out, c_in, k))
    gy = rng.standard_normal((B, c_out, t_out))
    alpha = rng.uniform(0.1, 3.0, c_in)
    alpha[-1] = 0.0
    return dict(x=x, w=w, gy=gy, alpha=alpha, k=k, s=s, d=d, pl=pl, pr=pr, act=act, slope=0.2, t_in=t_in)


def _torch_act(x, act, slope, alpha):
    if act == G.ACT_LEAKY:
        return F.leaky_relu(x, slope)
    if act == G.ACT_SNAKE:
        al = alpha.reshape(1, -1, 1)
        return x + (al + 1e-9).reciprocal() * (al * x).sin().pow(2)     # modules.Snake.forward
    return x


@pytest.mark.parametrize("fam,pad,act", CASES)
def test_reference_matches_float64_autograd(fam, pad, act):
    c = _data(fam, pad, act)
    x = torch.tensor(c["x"], requires_grad=True)
    w = torch.tensor(c["w"], requires_grad=True)
    bias = torch.zeros(c["w"].shape[0], dtype=torch.float64, requires_grad=True)
    alpha = torch.tensor(c["alpha"], requires_grad=True)
    a = F.pad(_torch_act(x, act, c["slope"], alpha), (c["pl"], c["pr"]))
    y = F.conv1d(a, w, bias, stride=c["s"], dilation=c["d"])
    y.backward(torch.tensor(c["gy"]))
    yref = G.forward(c["x"], c["w"], None, c["alpha"], None, c["k"], c["s"], c["d"], c["pl"], c["pr"], act, c["slope"])
    assert np.abs(yref - y.detach().numpy()).max() < 1e-11
    flat = G.backward(c["gy"], c["x"], c["w"], c["alpha"], c["k"], c["s"], c["d"], c["pl"], c["pr"], act, c["slope"])
    gx, gw, gb, ga = G.split(flat, *c["x"].shape[:2], c["w"].shape[0], c["t_in"], c["k"], act)
    assert np.abs(gx - x.grad.numpy()).max() < 1e-11
    assert np.abs(gw - w.grad.numpy()).max() < 1e-11
    assert np.abs(gb - bias.grad.numpy()).max() < 1e-11
    if act == G.ACT_SNAKE:
        assert np.abs(ga - alpha.grad.numpy()).max() < 1e-11
    if pad == "tail":
        assert (gx[:, :, c["t_in"] - (c["s"] - 1):] == 0).all()


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_reference_adjoint_identity(fam):
    c = _data(fam, "centred", G.ACT_SNAKE, seed=3)
    a = G.act_fwd(c["x"], c["act"], c["slope"], c["alpha"], np.float64)
    y = G.forward(a, c["w"], None, None, None, c["k"], c["s"], c["d"], c["pl"], c["pr"], G.ACT_NONE, 0.2)
    flat = G.backward(c["gy"], a, c["w"], None, c["k"], c["s"], c["d"], c["pl"], c["pr"], G.ACT_NONE, 0.2)
    ga = G.split(flat, *a.shape[:2], c["w"].shape[0], c["t_in"], c["k"], G.ACT_NONE)[0]
    lhs, rhs = float((y * c["gy"]).sum()), float((a * ga).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs))


def test_with_e_ref_is_per_output():
    c = _data((3, 1, 3), "centred", G.ACT_SNAKE)
    r64, e = G.with_e_ref(c["gy"], c["x"], c["w"], c["alpha"], c["k"], c["s"], c["d"], c["pl"], c["pr"], c["act"], 0.2)
    assert len(r64) == 4 and len(e) == 4 and all(0 < v < 1e-4 for v in e)


# ------------------------------------------------------------------ C boundary, host side
def _args(N, **kw):
    a = N.ConvBackwardArgs()
    a.c_in, a.c_out, a.kernel, a.stride, a.dilation = 16, 16, 3, 1, 1
    a.pad_left, a.pad_right, a.batch, a.t_in, a.t_out = 1, 1, 1, 32, 32
    a.leaky_slope = 0.2
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_and_struct():
    from rave_amd import _native as N
    for name in ("rave_conv1d_backward_data", "rave_conv1d_backward_weight", "rave_conv1d_backward_workspace"):
        assert name in N.EXPORTS and hasattr(N.lib, name)
    assert N.ConvBackwardArgs in N.STRUCTS and C.sizeof(N.ConvBackwardArgs) == 184


def test_host_refusals():
    from rave_amd import _native as N

    def rc_text(a, fn=None):
        rc = (fn or N.lib.rave_conv1d_backward_data)(C.byref(a), None)
        return rc, N.lib.rave_last_error().decode()

    rc, text = rc_text(_args(N, transposed=1))
    assert rc == N.RAVE_ERR_ARG and "transposed" in text
    for prec in (1, 4, 5):
        rc, text = rc_text(_args(N, precision=prec))
        assert rc == N.RAVE_ERR_ARG and "precision" in text
    rc, text = rc_text(_args(N, kernel=5))
    assert rc == N.RAVE_ERR_UNSUPPORTED and "unsupported" in text
    rc, text = rc_text(_args(N, kernel=7, dilation=2, pad_left=6, pad_right=6))
    assert rc == N.RAVE_ERR_ARG and "dilation" in text
    rc, text = rc_text(_args(N, t_out=31))
    assert rc == N.RAVE_ERR_ARG and "t_out" in text
    assert N.lib.rave_conv1d_backward_workspace(C.byref(_args(N, t_out=31))) == N.RAVE_ERR_ARG
    # a missing x where the activation's derivative or gweight needs it (dummy non-null pointers: refused before any launch)
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    rc, text = rc_text(_args(N, act=1, gy=p, weight=p, gx=p))
    assert rc == N.RAVE_ERR_ARG and "needs the input x" in text
    rc, text = rc_text(_args(N, gy=p, weight=p, gweight=p), N.lib.rave_conv1d_backward_weight)
    assert rc == N.RAVE_ERR_ARG and "needs the input x" in text
    rc, text = rc_text(_args(N, act=2, gy=p, weight=p, gx=p, x=p))
    assert rc == N.RAVE_ERR_ARG and "alpha" in text
