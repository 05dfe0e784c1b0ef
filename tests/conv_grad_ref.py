"""NumPy restatement of the conv1d backward (include/rave_amd.h, "conv1d backward").

Direct loops over the formulas, in the dtype asked for: float64 is the
reference, the float32 run is the same chain of sums in the kernels' number
format and its error against float64 (``e_ref``, ``with_e_ref``) sets the bound
of tests/test_gpu_conv_grad.py (4 e_ref per output).  No GPU, nothing imported
from the library; tests/test_conv_grad_ref_host.py pins it to torch autograd on
the CPU and to the adjoint identity.

    a          = act(x), zero outside [0, t_in)
    y[b,m,n]   = bias[m] + sum_{ci,j} W[m,ci,j] a[b,ci,n s + j d - pl] (+ res[b,m,n])
    gbias[m]   = sum_{b,n} gy[b,m,n]
    gW[m,ci,j] = sum_{b,n} gy[b,m,n] a[b,ci,n s + j d - pl]
    ga[b,ci,t] = sum_{m,j} W[m,ci,j] gy[b,m,(t + pl - j d)/s]
    gx         = ga act'(x)
    galpha[ci] = sum_{b,t} ga[b,ci,t] d act/d alpha (x[b,ci,t])
"""
import numpy as np

ACT_NONE, ACT_LEAKY, ACT_SNAKE = 0, 1, 2
# (kernel, stride, dilation): every layer family of the non-transposed conv
FAMILIES = [(1, 1, 1), (3, 1, 1), (3, 1, 3), (3, 1, 9), (3, 1, 16), (7, 1, 1), (4, 2, 1), (8, 4, 1)]


def t_out_of(t_in, k, s, d, pl, pr):
    return (t_in + pl + pr - ((k - 1) * d + 1)) // s + 1


def act_fwd(x, act, slope, alpha, dtype):
    """modules.LeakyReLU / modules.Snake's expression."""
    x = np.asarray(x, dtype)
    if act == ACT_LEAKY:
        return np.where(x > 0, x, x * dtype(slope))
    if act == ACT_SNAKE:
        al = np.asarray(alpha, dtype).reshape(1, -1, 1)
        return x + (dtype(1) / (al + dtype(1e-9))) * np.sin(al * x) ** 2
    return x


def act_dx(x, act, slope, alpha, dtype):
    x = np.asarray(x, dtype)
    if act == ACT_LEAKY:
        return np.where(x > 0, dtype(1), dtype(slope)).astype(dtype)
    if act == ACT_SNAKE:
        al = np.asarray(alpha, dtype).reshape(1, -1, 1)
        return dtype(1) + al * np.sin(dtype(2) * al * x) / (al + dtype(1e-9))
    return np.ones_like(x)


def act_dalpha(x, alpha, dtype):
    x = np.asarray(x, dtype)
    al = np.asarray(alpha, dtype).reshape(1, -1, 1)
    r = al + dtype(1e-9)
    return x * np.sin(dtype(2) * al * x) / r - np.sin(al * x) ** 2 / (r * r)


def _taps(t_in, t_out, k, s, d, pl):
    """Per tap j: (n, t) index arrays of the outputs n whose column t = n s + j d - pl is inside the input."""
    n = np.arange(t_out)
    for j in range(k):
        t = n * s + j * d - pl
        ok = (t >= 0) & (t < t_in)
        yield j, n[ok], t[ok]


def forward(x, w, bias, alpha, res, k, s, d, pl, pr, act, slope, dtype=np.float64):
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    B, c_in, t_in = x.shape
    t_out = t_out_of(t_in, k, s, d, pl, pr)
    a = act_fwd(x, act, slope, alpha, dtype)
    y = np.zeros((B, w.shape[0], t_out), dtype)
    for j, n, t in _taps(t_in, t_out, k, s, d, pl):
        for ci in range(c_in):
            y[:, :, n] += w[None, :, ci, j, None] * a[:, None, ci, t]
    if bias is not None:
        y += np.asarray(bias, dtype).reshape(1, -1, 1)
    if res is not None:
        y += np.asarray(res, dtype)
    return y


def backward(gy, x, w, alpha, k, s, d, pl, pr, act, slope, dtype=np.float64):
    """The five gradients stacked in one flat array (so ``with_e_ref`` covers them
    all); ``split`` takes them apart.  The residual's gradient is gy itself."""
    gy = np.asarray(gy, dtype)
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    B, c_in, t_in = x.shape
    c_out, t_out = gy.shape[1], gy.shape[2]
    assert t_out == t_out_of(t_in, k, s, d, pl, pr) and w.shape == (c_out, c_in, k)
    a = act_fwd(x, act, slope, alpha, dtype)
    gbias = np.zeros(c_out, dtype)
    gw = np.zeros((c_out, c_in, k), dtype)
    ga = np.zeros((B, c_in, t_in), dtype)
    for b in range(B):
        for n in range(t_out):                              # K of the weight gradient, in (b, n) order
            gbias += gy[b, :, n]
    for j, n, t in _taps(t_in, t_out, k, s, d, pl):
        for b in range(B):
            for nn, tt in zip(n, t):
                gw[:, :, j] += gy[b, :, nn, None] * a[b, None, :, tt]
        for m in range(c_out):                              # K of the data gradient, in (j, m) order
            ga[:, :, t] += w[m, :, j][None, :, None] * gy[:, m, n][:, None, :]
    gx = (ga * act_dx(x, act, slope, alpha, dtype)).astype(dtype)
    out = [gx.ravel(), gw.ravel(), gbias]
    if act == ACT_SNAKE:
        term = ga * act_dalpha(x, alpha, dtype)
        galpha = np.zeros(c_in, dtype)
        for b in range(B):
            for t in range(t_in):
                galpha += term[b, :, t]
        out.append(galpha)
    return np.concatenate(out).astype(dtype)


def split(flat, B, c_in, c_out, t_in, k, act):
    """(gx, gweight, gbias, galpha or None) of ``backward``'s flat result."""
    sizes = [B * c_in * t_in, c_out * c_in * k, c_out] + ([c_in] if act == ACT_SNAKE else [])
    parts = np.split(np.asarray(flat), np.cumsum(sizes)[:-1])
    return (parts[0].reshape(B, c_in, t_in), parts[1].reshape(c_out, c_in, k), parts[2],
            parts[3] if act == ACT_SNAKE else None)


def with_e_ref(gy, x, w, alpha, k, s, d, pl, pr, act, slope):
    """((gx, gW, gbias, galpha) in float64, the same tuple of e_ref): per output,
    the max-abs error of the reference's float32 run against its float64 run."""
    B, c_in, t_in = np.asarray(x).shape
    c_out = np.asarray(gy).shape[1]
    args = (gy, x, w, alpha, k, s, d, pl, pr, act, slope)
    r64 = split(backward(*args, dtype=np.float64), B, c_in, c_out, t_in, k, act)
    f32 = backward(*args, dtype=np.float32)
    assert f32.dtype == np.float32
    r32 = split(f32, B, c_in, c_out, t_in, k, act)
    e = tuple(None if a64 is None else float(np.abs(a32.astype(np.float64) - a64).max())
              for a32, a64 in zip(r32, r64))
    return r64, e
