"""NumPy restatement of the ConvTranspose1d forward and backward (include/rave_amd.h,
"conv_transpose1d backward"): nn.ConvTranspose1d(c_in, c_out, 2 r, stride=r, padding=r // 2),
even r, with the fused input activation, bias and residual.

Direct loops over the formulas, in the dtype asked for: float64 is the
reference, the float32 run is the same chain of sums in the kernels' number
format and its error against float64 (``e_ref``, ``with_e_ref``) sets the bound
of tests/test_gpu_convt_grad.py (4 e_ref per output).  No GPU, nothing imported
from the library; tests/test_convt_grad_ref_host.py pins it to torch autograd on
the CPU and to the adjoint identity.

    a          = act(x), P = r / 2, W (c_in, c_out, 2 r), t_out = t_in r
    y[b,m,t]   = bias[m] + sum_{ci,u,j : u r + j - P = t} W[ci,m,j] a[b,ci,u] (+ res[b,m,t])
    gbias[m]   = sum_{b,t} gy[b,m,t]
    gW[ci,m,j] = sum_{b,u} a[b,ci,u] gy[b,m,u r + j - P]
    ga[b,ci,u] = sum_{m,j} W[ci,m,j] gy[b,m,u r + j - P]
    gx         = ga act'(x)
    galpha[ci] = sum_{b,u} ga[b,ci,u] d act/d alpha (x[b,ci,u])
"""
import numpy as np

from tests.conv_grad_ref import ACT_LEAKY, ACT_NONE, ACT_SNAKE, act_dalpha, act_dx, act_fwd  # noqa: F401

STRIDES = [2, 4]


def _taps(t_in, r):
    """Per tap j: (u, t) index arrays of the inputs u whose output column t = u r + j - P is inside the output."""
    u = np.arange(t_in)
    for j in range(2 * r):
        t = u * r + j - r // 2
        ok = (t >= 0) & (t < t_in * r)
        yield j, u[ok], t[ok]


def forward(x, w, bias, alpha, res, r, act, slope, dtype=np.float64):
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    B, c_in, t_in = x.shape
    assert w.shape[0] == c_in and w.shape[2] == 2 * r and r % 2 == 0
    a = act_fwd(x, act, slope, alpha, dtype)
    y = np.zeros((B, w.shape[1], t_in * r), dtype)
    for j, u, t in _taps(t_in, r):
        for ci in range(c_in):
            y[:, :, t] += w[None, ci, :, j, None] * a[:, None, ci, u]
    if bias is not None:
        y += np.asarray(bias, dtype).reshape(1, -1, 1)
    if res is not None:
        y += np.asarray(res, dtype)
    return y


def backward(gy, x, w, alpha, r, act, slope, dtype=np.float64):
    """The gradients stacked in one flat array (so ``with_e_ref`` covers them
    all); ``split`` takes them apart.  The residual's gradient is gy itself."""
    gy = np.asarray(gy, dtype)
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    B, c_in, t_in = x.shape
    c_out, t_out = gy.shape[1], gy.shape[2]
    assert t_out == t_in * r and w.shape == (c_in, c_out, 2 * r) and r % 2 == 0
    a = act_fwd(x, act, slope, alpha, dtype)
    gbias = np.zeros(c_out, dtype)
    gw = np.zeros((c_in, c_out, 2 * r), dtype)
    ga = np.zeros((B, c_in, t_in), dtype)
    for b in range(B):
        for t in range(t_out):
            gbias += gy[b, :, t]
    for j, u, t in _taps(t_in, r):
        for b in range(B):
            for uu, tt in zip(u, t):                        # K of the weight gradient, in (b, u) order
                gw[:, :, j] += a[b, :, uu, None] * gy[b, None, :, tt]
    for m in range(c_out):                                  # K of the data gradient, in (m, j) order
        for j, u, t in _taps(t_in, r):
            ga[:, :, u] += w[:, m, j][None, :, None] * gy[:, m, t][:, None, :]
    gx = (ga * act_dx(x, act, slope, alpha, dtype)).astype(dtype)
    out = [gx.ravel(), gw.ravel(), gbias]
    if act == ACT_SNAKE:
        term = ga * act_dalpha(x, alpha, dtype)
        galpha = np.zeros(c_in, dtype)
        for b in range(B):
            for u in range(t_in):
                galpha += term[b, :, u]
        out.append(galpha)
    return np.concatenate(out).astype(dtype)


def split(flat, B, c_in, c_out, t_in, r, act):
    """(gx, gweight, gbias, galpha or None) of ``backward``'s flat result."""
    sizes = [B * c_in * t_in, c_in * c_out * 2 * r, c_out] + ([c_in] if act == ACT_SNAKE else [])
    parts = np.split(np.asarray(flat), np.cumsum(sizes)[:-1])
    return (parts[0].reshape(B, c_in, t_in), parts[1].reshape(c_in, c_out, 2 * r), parts[2],
            parts[3] if act == ACT_SNAKE else None)


def with_e_ref(gy, x, w, alpha, r, act, slope):
    """((gx, gW, gbias, galpha) in float64, the same tuple of e_ref): per output,
    the max-abs error of the reference's float32 run against its float64 run."""
    B, c_in, t_in = np.asarray(x).shape
    c_out = np.asarray(gy).shape[1]
    args = (gy, x, w, alpha, r, act, slope)
    r64 = split(backward(*args, dtype=np.float64), B, c_in, c_out, t_in, r, act)
    f32 = backward(*args, dtype=np.float32)
    assert f32.dtype == np.float32
    r32 = split(f32, B, c_in, c_out, t_in, r, act)
    e = tuple(None if a64 is None else float(np.abs(a32.astype(np.float64) - a64).max())
              for a32, a64 in zip(r32, r64))
    return r64, e
