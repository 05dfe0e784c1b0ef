"""What tests/test_gpu_conv_grad.py and tests/test_gpu_convt_grad.py share: the library
accessor, the stream, one data + weight call through the C boundary on guarded views, and
the 4 e_ref bar.  A plain module: each test file keeps its own cases and `_args`."""
import ctypes as C

import torch

from tests.conv_grad_ref import ACT_SNAKE
from tests.test_gpu_aux_kernels import DEV, maxerr, put, guarded, report, untouched


def native():
    from rave_amd import _native as N
    return N


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bwd(prefix, wshape, args, c, want=("gx", "gw", "gb", "ga"), null_x=False, check=True, **kw):
    """One data + one weight call of the `prefix`_workspace / _data / _weight entry points on
    guarded views, the struct filled by args(c, **kw) and gweight shaped `wshape`; returns
    (dict of outputs, workspace floats)."""
    N = native()
    lib = {name: getattr(N.lib, f"{prefix}_{name}") for name in ("workspace", "data", "weight")}
    B, ci, co, nw = c["B"], c["c_in"], c["c_out"], wshape[0] * wshape[1] * wshape[2]
    snake = c["act"] == ACT_SNAKE
    xb, xv, xm = put(c["x"], [(1, 1), (2, 3), (5, 7)])
    gb_, gv, gm = put(c["gy"], [(0, 1), (3, 1), (4, 9)])
    ob, ov, om = guarded((B, ci, c["t_in"]), [(1, 0), (1, 2), (8, 3)])
    w = torch.from_numpy(c["w"]).to(DEV)
    al = torch.from_numpy(c["alpha"]).to(DEV)
    gw = torch.full((nw + 16,), float("nan"), device=DEV)
    gbias = torch.full((co + 16,), float("nan"), device=DEV)
    galpha = torch.full((ci + 16,), float("nan"), device=DEV)
    a = args(c, **kw)
    if not null_x:
        a.x, a.x_sb, a.x_sc = xv.data_ptr(), xv.stride(0), xv.stride(1)
    a.gy, a.gy_sb, a.gy_sc = gv.data_ptr(), gv.stride(0), gv.stride(1)
    a.weight = w.data_ptr()
    if snake:
        a.alpha = al.data_ptr()
    if "gx" in want:
        a.gx, a.gx_sb, a.gx_sc = ov.data_ptr(), ov.stride(0), ov.stride(1)
    if "gw" in want:
        a.gweight = gw.data_ptr()
    if "gb" in want:
        a.gbias = gbias.data_ptr()
    if "ga" in want and snake:
        a.galpha = galpha.data_ptr()
    nws = lib["workspace"](C.byref(a))
    if nws < 0:
        return nws, None
    ws = torch.full((max(nws, 1) + 16,), float("nan"), device=DEV)      # never zeroed
    if nws > 0:
        a.workspace = ws.data_ptr()
    rc = lib["data"](C.byref(a), stream())
    if rc == N.RAVE_OK:
        rc = lib["weight"](C.byref(a), stream())
    if not check:
        return rc, None
    N.check(rc)
    torch.cuda.synchronize()
    assert untouched(xb, xm) and untouched(gb_, gm) and untouched(ob, om)
    assert bool(torch.isnan(gw[nw:]).all() and torch.isnan(gbias[co:]).all() and torch.isnan(galpha[ci:]).all())
    assert bool(torch.isnan(ws[max(nws, 1):]).all())
    out = {}
    if "gx" in want:
        out["gx"] = ov.clone()
    if "gw" in want:
        out["gw"] = gw[:nw].reshape(wshape).clone()
    if "gb" in want:
        out["gb"] = gbias[:co].clone()
    if "ga" in want and snake:
        out["ga"] = galpha[:ci].clone()
    return out, nws


def held(what, out, ref):
    """Print every figure, then assert 4 e_ref per output; returns the worst ratio.
    `ref` is a reference's with_e_ref(): the float64 outputs and their e_ref."""
    r64, e = ref
    worst, fails = 0.0, []
    for name, r, e_ref in zip(("gx", "gw", "gb", "ga"), r64, e):
        if r is None or name not in out:
            continue
        err = maxerr(out[name], r)
        worst = max(worst, report(f"{what} {name}", err, e_ref))
        assert bool(torch.isfinite(out[name]).all()), (what, name)
        if err > 4 * e_ref:
            fails.append((name, err, e_ref))
    assert not fails, (what, fails)
    return worst
