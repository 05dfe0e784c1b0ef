"""Plain restatements of the forward kernels of the inference path (rave_conv1d,
rave_residual_unit, rave_residual_stack; include/rave_amd.h "conv1d", "fused
residual unit", "residual stack"): each function takes the fields of its args
struct and the precision as ``dtype``, so that one function gives both the
float64 reference and the float32 CPU run whose error against it (``e_ref``,
``with_e_ref``) sets the bound of tests/test_gpu_conv_fwd.py (4 e_ref for the
exact fp32 kernels, the rule of tests/aux_ref.py).  No GPU, nothing imported
from the library; tests/test_conv_fwd_ref_host.py pins these against torch and
the oracle on the CPU.

    conv   y[b,m,n]     = bias[m] + sum_{ci,j} W[m,ci,j] a[b,ci,n s + j d - pl] (+ res[b,m,n])
    convt  y[b,m,u r+q] = bias[m] + sum_ci W[ci,m,q+P+r] a[b,ci,u-1+pl] + W[ci,m,q+P] a[b,ci,u+pl]    q <  r-P
                          bias[m] + sum_ci W[ci,m,q+P] a[b,ci,u+pl] + W[ci,m,q+P-r] a[b,ci,u+1+pl]    q >= r-P
           (P = out_shift; offline pl = 0, P = r/2, t_out = t_in r; cached pl = 1, P = 0,
           t_out = (t_in - 1) r: the view starts with one history column)
    unit   h = act(W1 *_d act(x) + b1),  y[..., n] = x[..., n + res_shift] + W2 h + b2
    stack  three units one after the other

a = act(x), zero outside [0, t_in) (the unit: outside [0, x_len)).  Every sum is
one sequential chain per output in the kernels' documented K order: chunks of
``CHUNK[taps]`` input channels (rave_conv1d_chunk), inside a chunk tap-major and
channel-minor (the packed image of rave_conv1d_pack_weight); the unit's W1 sum
runs tap-major over all C channels, its W2 sum in channel order
(rave_unit_pack_weight).  The accumulator is held in ``dtype`` after every step,
and a step is one fused multiply-add (``_fma`` of tests/filterbank_ref.py, whose
docstring records why a separate multiply and add gives a wrong e_ref: the
MFMA fp32 path is a k-ordered fmaf chain).  No np.dot and no np.sum.  The
unit's intermediate h is rounded to ``dtype``, as the kernel holds it in fp32.

``S`` is the condition sum of an output, in float64: sum |W| |a| over its taps
(plus |bias| and |residual|); for the unit, through both GEMMs:
|x| + |b2| + sum_ci |W2[m,ci]| (|b1[ci]| + sum |W1| |a|); for the stack the sum
of its units' S, each at that unit's float64 input."""
import numpy as np

from tests.conv_grad_ref import ACT_LEAKY, ACT_NONE, ACT_SNAKE, act_fwd      # noqa: F401
from tests.filterbank_ref import _fma, _window

# input channels per K-chunk by tap count (rave_conv1d_chunk; 2 taps: transposed)
CHUNK = {1: 32, 2: 32, 3: 16, 4: 16, 7: 8, 8: 8}


def _act(x, act, slope, alpha, dtype):
    return np.asarray(act_fwd(x, act, slope, alpha, dtype), dtype)


def _abs_step(S, w, a):
    return S + np.abs(w) * np.abs(a)


def _finish(acc, S, bias, res, dtype, cond):
    if bias is not None:
        b = np.asarray(bias, dtype).reshape(1, -1, 1)
        acc = acc + b
        if cond:
            S = S + np.abs(b.astype(np.float64))
    if res is not None:
        r = np.asarray(res, dtype)
        acc = acc + r
        if cond:
            S = S + np.abs(r.astype(np.float64))
    return (acc, S) if cond else acc


def conv(x, w, bias, alpha, res, k, s, d, pl, t_out, act, slope, dtype=np.float64, cond=False, chunk=None):
    """rave_conv1d, transposed = 0.  x (B, c_in, t_in), w (c_out, c_in, k) -> (B, c_out, t_out);
    with ``cond`` also S.  ``chunk``: input channels per K-chunk where the kernel's is not
    CHUNK[k] (the fused edges' convs, tests/edge_ref.py)."""
    x = np.asarray(x)
    B, c_in, _ = x.shape
    wd = np.asarray(w, dtype).astype(np.float64)
    c_out = wd.shape[0]
    a = _act(x, act, slope, alpha, dtype)
    ap = _window(a, -pl, (t_out - 1) * s + (k - 1) * d + 1, dtype).astype(np.float64)
    at = s * np.arange(t_out)
    acc = np.zeros((B, c_out, t_out), dtype)
    S = np.zeros((B, c_out, t_out), np.float64)
    chunk = chunk or CHUNK[k]
    for c0 in range(0, c_in, chunk):
        for j in range(k):
            for ci in range(c0, min(c0 + chunk, c_in)):
                wv, av = wd[None, :, ci, j, None], ap[:, ci][:, None, at + j * d]
                acc = _fma(wv, av, acc)
                if cond:
                    S = _abs_step(S, wv, av)
    return _finish(acc, S, bias, res, dtype, cond)


def convt_geometry(t_in, r, cached):
    """(pad_left, out_shift, t_out) of the two documented forms."""
    return (1, 0, (t_in - 1) * r) if cached else (0, r // 2, t_in * r)


def convt(x, w, bias, alpha, r, pl, out_shift, act, slope, dtype=np.float64, cond=False):
    """rave_conv1d, transposed = 1: nn.ConvTranspose1d(c_in, c_out, 2 r, stride = r) in
    polyphase form.  x (B, c_in, t_in), w (c_in, c_out, 2 r) -> (B, c_out, (t_in - pl) r)."""
    x = np.asarray(x)
    B, c_in, t_in = x.shape
    wd = np.asarray(w, dtype).astype(np.float64)
    c_out, P, U = wd.shape[1], out_shift, t_in - pl
    a = _act(x, act, slope, alpha, dtype)
    ap = _window(a, pl - 1, U + 2, dtype).astype(np.float64)      # ap[i] = a[pl - 1 + i]
    q = np.arange(r)
    first = q < r - P                                             # phases that read (u - 1, u)
    kidx = [np.where(first, q + P + r, q + P), np.where(first, q + P, q + P - r)]
    off = [np.where(first, -1, 0), np.where(first, 0, 1)]
    u = np.arange(U)
    acc = np.zeros((B, c_out, U, r), dtype)
    S = np.zeros((B, c_out, U, r), np.float64)
    for c0 in range(0, c_in, CHUNK[2]):
        for j in range(2):
            cols = u[:, None] + off[j][None, :] + 1
            for ci in range(c0, min(c0 + CHUNK[2], c_in)):
                wv, av = wd[ci][:, kidx[j]][None, :, None, :], ap[:, ci][:, cols][:, None]
                acc = _fma(wv, av, acc)
                if cond:
                    S = _abs_step(S, wv, av)
    return _finish(acc.reshape(B, c_out, U * r), S.reshape(B, c_out, U * r), bias, None, dtype, cond)


def unit(x, w1, w2, b1, b2, a0, a2, d, pl, t_len, act, slope, x_len=0, res_shift=0, dtype=np.float64, cond=False):
    """rave_residual_unit.  x (B, C, >= x_len), w1 (C, C, 3), w2 (C, C, 1) -> (B, C, t_len).
    pad_left anywhere in [0, 2 d]; the cached form is pl = 0, x_len = 2 d + t_len,
    res_shift = 2 d - delay.  Columns past x_len (0: t_len) are never read."""
    xl = x_len if x_len > 0 else t_len
    x = np.asarray(x)[:, :, :xl]
    B, C, _ = x.shape
    w1d = np.asarray(w1, dtype).astype(np.float64)
    w2d = np.asarray(w2, dtype).astype(np.float64).reshape(C, C)
    xd = np.asarray(x, dtype)
    ap = _window(_act(xd, act, slope, a0, dtype), -pl, t_len + 2 * d, dtype).astype(np.float64)
    acc = np.zeros((B, C, t_len), dtype)
    S1 = np.zeros((B, C, t_len), np.float64)
    for j in range(3):
        for ci in range(C):
            wv, av = w1d[None, :, ci, j, None], ap[:, ci][:, None, j * d:j * d + t_len]
            acc = _fma(wv, av, acc)
            if cond:
                S1 = _abs_step(S1, wv, av)
    if b1 is not None:
        acc = acc + np.asarray(b1, dtype).reshape(1, -1, 1)
        S1 = S1 + np.abs(np.asarray(b1, np.float64)).reshape(1, -1, 1)
    g = _act(acc, act, slope, a2, dtype).astype(np.float64)       # h, rounded to dtype
    acc = np.zeros((B, C, t_len), dtype)
    S = np.zeros((B, C, t_len), np.float64)
    for ci in range(C):
        acc = _fma(w2d[None, :, ci, None], g[:, ci][:, None, :], acc)
        if cond:
            S = _abs_step(S, w2d[None, :, ci, None], S1[:, ci][:, None, :])
    if b2 is not None:
        acc = acc + np.asarray(b2, dtype).reshape(1, -1, 1)
        S = S + np.abs(np.asarray(b2, np.float64)).reshape(1, -1, 1)
    xr = xd[:, :, res_shift:res_shift + t_len]
    y = xr + acc
    return (y, S + np.abs(xr.astype(np.float64))) if cond else y


def stack(x, units, act, slope, dtype=np.float64, cond=False):
    """rave_residual_stack: ``units`` is three (w1, w2, b1, b2, a0, a2, d, pl); one-shot form."""
    y = np.asarray(x, dtype)
    T = y.shape[-1]
    S = 0.0
    for w1, w2, b1, b2, a0, a2, d, pl in units:
        out = unit(y, w1, w2, b1, b2, a0, a2, d, pl, T, act, slope, dtype=dtype, cond=cond)
        if cond:
            y, s = out
            S = S + s
        else:
            y = out
    return (y, S) if cond else y


def with_e_ref(fn, *args, **kw):
    """(float64 result, e_ref, S): e_ref the max-abs error of fn's float32 run against its
    float64 run over the case's outputs; S the condition sum per output, in float64."""
    r64, S = fn(*args, dtype=np.float64, cond=True, **kw)
    r32 = fn(*args, dtype=np.float32, **kw)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    return r64, float(np.abs(r32.astype(np.float64) - r64).max()), S
