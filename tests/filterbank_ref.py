"""Plain restatements of the filterbank kernels (rave_amd/csrc/pqmf.hip and
fir_kernel of rave_amd/csrc/speaker.hip): each function takes the fields of its
args struct in include/rave_amd.h and the precision as ``dtype``, so that one
function gives both the float64 reference and the fp32 CPU run whose error
against it (``e_ref``) sets the bound of tests/test_gpu_filterbank.py (4 e_ref,
the rule of tests/aux_ref.py).  No GPU, no import of the reference;
tests/test_filterbank_ref_host.py pins these against the oracle and the
fixtures on the CPU.

The sums are one sequential chain per output, in the order the kernels document
(k order; (tap, channel) order for the synthesis): a loop over the taps,
vectorised over the outputs, the accumulator held in ``dtype`` after every
step.  No np.dot or np.sum: their pairwise sums are more accurate than a chain
and would make e_ref smaller than any fp32 chain can meet.

A step is a fused multiply-add, because that is what the kernels document:
fir_kernel is ``acc = fmaf(h, x, acc)``, and the PQMF kernels run on
v_mfma_f32_16x16x4_f32, "a k-ordered fmaf chain, bitwise equal to f32 FMAs in
k order" (pqmf.hip).  numpy has no fma, so the fp32 step is
float32(float64(h) float64(x) + float64(acc)): the product of two fp32 values
is exact in float64, and the sum is rounded to 53 bits and then to 24, which
differs from the single rounding only when the 53-bit value falls on a 24-bit
tie.  A separate multiply and add (two roundings per step) is a different
arithmetic: with it e_ref of a one-output case (t_out = 1) is the error of a
single draw and was measured at 1.6e-9 where the kernel's correctly chained
fmaf result was 3.1e-8, half an ulp, off (ratio 19.95; 1.00 with the fma step).

    analysis   y[b, k, t]     = rh(k, t) sum_j hkf[k, j] x[b, 16 t + j - pad_left]
    synthesis  y[b, 16 t + i] = 16 sum_{k, c} hki[15 - i, c, k] in[b, c, t + k - pad_left]
    fir        y[b, t P + p]  = sum_k h[p, k] x[b, t S + k - pad_left]

rh(k, t) = -1 for odd k at even t (reverse_half), +1 otherwise; samples and
frames outside the input read as zero."""
import numpy as np

N_BAND = 16


def rh(k, t):
    """reverse_half's sign for band k at (global) frame t; broadcasts."""
    k, t = np.asarray(k), np.asarray(t)
    return np.where((k % 2 == 1) & (t % 2 == 0), -1.0, 1.0)


def _fma(a, b, acc):
    """acc + a b as one fused step in acc's dtype; a and b are float64 copies of
    values of that dtype."""
    if acc.dtype == np.float64:
        return acc + a * b
    return (a * b + acc.astype(np.float64)).astype(acc.dtype)


def _window(x, first, n, dtype):
    """x[..., first : first + n] in ``dtype`` with zeros outside [0, x.shape[-1])."""
    out = np.zeros(x.shape[:-1] + (n,), dtype)
    lo, hi = max(first, 0), min(first + n, x.shape[-1])
    if hi > lo:
        out[..., lo - first:hi - first] = x[..., lo:hi]
    return out


def analysis(x, hkf, pad_left, t_out, n_out_bands, dtype=np.float64):
    """rave_pqmf_analysis.  x (B, t_in), hkf (16, taps) -> (B, n_out_bands, t_out)."""
    x, h = np.asarray(x), np.asarray(hkf, dtype)[:n_out_bands].astype(np.float64)
    taps = h.shape[1]
    xp = _window(x, -pad_left, N_BAND * (t_out - 1) + taps, dtype).astype(np.float64)
    at = N_BAND * np.arange(t_out)
    acc = np.zeros((x.shape[0], n_out_bands, t_out), dtype)
    for j in range(taps):
        acc = _fma(h[None, :, j, None], xp[:, None, at + j], acc)
    sign = rh(np.arange(n_out_bands)[:, None], np.arange(t_out)[None, :]).astype(dtype)
    return acc * sign[None]


def staged(x, pad_left, mode, frame0, x_len, noise, t_in, dtype=np.float64, taps=33):
    """The synthesis input as the kernel stages it: in[b, c, w] for the window
    frames f = w - pad_left, w in [0, t_in + taps - 1); columns [0, x_len) of x
    are input (x_len = 0 means t_in), everything else is zero *after* the
    epilogue (the padding is the convolution's, not the activation's)."""
    x = np.asarray(x)
    n = x_len if x_len > 0 else t_in
    one = dtype(1.0)
    v = x[:, :N_BAND, :n].astype(dtype)
    if mode != 0:
        if mode == 1:
            with np.errstate(over="ignore"):
                v = v * (one / (one + np.exp(-x[:, N_BAND:2 * N_BAND, :n].astype(dtype))))
        if noise is not None:
            v = v + np.asarray(noise)[:, :, :n].astype(dtype)
        v = np.tanh(v)
    sign = rh(np.arange(N_BAND)[:, None], frame0 + np.arange(n)[None, :]).astype(dtype)
    return _window(v * sign[None], -pad_left, t_in + taps - 1, dtype)


def synthesis(x, hki, pad_left, mode, frame0, x_len, noise, t_in, dtype=np.float64):
    """rave_pqmf_synthesis.  x (B, 16 or 32, >= x_len), noise (B, 16, >= x_len)
    or None, hki (16, 16, taps) -> (B, 16 t_in)."""
    h = np.asarray(hki, dtype).astype(np.float64)
    taps = h.shape[2]
    w = staged(x, pad_left, mode, frame0, x_len, noise, t_in, dtype, taps).astype(np.float64)
    acc = np.zeros((w.shape[0], N_BAND, t_in), dtype)
    for k in range(taps):
        for c in range(N_BAND):
            acc = _fma(h[None, :, c, k, None], w[:, None, c, k:k + t_in], acc)
    acc = acc * dtype(N_BAND)
    # y[16 t + i] = acc[15 - i, t]
    return np.ascontiguousarray(acc[:, ::-1, :].transpose(0, 2, 1)).reshape(w.shape[0], N_BAND * t_in)


def fir(x, h, stride, pad_left, t_out, dtype=np.float64):
    """rave_fir.  x (B, t_in), h (phases, taps) -> (B, t_out phases)."""
    x, h = np.asarray(x), np.asarray(h, dtype).astype(np.float64)
    phases, taps = h.shape
    xp = _window(x, -pad_left, stride * (t_out - 1) + taps, dtype).astype(np.float64)
    at = stride * np.arange(t_out)
    acc = np.zeros((x.shape[0], t_out, phases), dtype)
    for k in range(taps):
        acc = _fma(h[None, None, :, k], xp[:, at + k, None], acc)
    return acc.reshape(x.shape[0], t_out * phases)


def with_e_ref(fn, *args):
    """(float64 result, e_ref): the max-abs error of fn's fp32 run against its
    float64 run over the case's outputs."""
    r64 = fn(*args, dtype=np.float64)
    r32 = fn(*args, dtype=np.float32)
    assert r32.dtype == np.float32
    return r64, float(np.abs(r32.astype(np.float64) - r64).max())


# ------------------------------------------------------------------ closed forms
def analysis_impulse(hkf, s, pad_left, t_out, n_out_bands):
    """analysis of a unit impulse at sample s: rh(k, t) hkf[k, s + pad_left - 16 t]
    (the tap j with 16 t + j - pad_left = s)."""
    h = np.asarray(hkf)
    j = s + pad_left - N_BAND * np.arange(t_out)
    ok = (j >= 0) & (j < h.shape[1])
    y = np.where(ok[None, :], h[:n_out_bands][:, np.clip(j, 0, h.shape[1] - 1)], 0)
    return (y * rh(np.arange(n_out_bands)[:, None], np.arange(t_out)[None, :])).astype(h.dtype)


def synthesis_impulse(hki, c, f, pad_left, frame0, t_in):
    """synthesis (mode 0) of a unit impulse in channel c at column f:
    y[16 t + i] = 16 rh(c, frame0 + f) hki[15 - i, c, f - t + pad_left]."""
    h = np.asarray(hki)
    k = f - np.arange(t_in) + pad_left
    ok = (k >= 0) & (k < h.shape[2])
    y = np.where(ok[None, :], h[::-1, c][:, np.clip(k, 0, h.shape[2] - 1)], 0)       # (i, t)
    return (N_BAND * float(rh(c, frame0 + f)) * y.T.reshape(-1)).astype(h.dtype)


def fir_impulse(h, s, stride, pad_left, t_out):
    """fir of a unit impulse at sample s: y[t P + p] = h[p, s - t S + pad_left]."""
    h = np.asarray(h)
    k = s - stride * np.arange(t_out) + pad_left
    ok = (k >= 0) & (k < h.shape[1])
    y = np.where(ok[None, :], h[:, np.clip(k, 0, h.shape[1] - 1)], 0)                # (p, t)
    return np.ascontiguousarray(y.T).reshape(-1).astype(h.dtype)


# ------------------------------------------------------------------ the streaming case
STREAM_FRAMES, STREAM_HIST = 300, 32
STREAM_BLOCKS = (1, 37, 128, 134)           # starts 0, 1, 38, 166; 0 - 32, 1 - 32 ... : both parities


def stream_signal(batch=2):
    """(x (B, 32, 300), noise (B, 16, 300)) fp32: the signal of the streaming
    identity, host and GPU.  |x| stays far below 2^15."""
    rng = np.random.default_rng(300)
    x = rng.standard_normal((batch, 2 * N_BAND, STREAM_FRAMES)).astype(np.float32)
    noise = (0.1 * rng.standard_normal((batch, N_BAND, STREAM_FRAMES))).astype(np.float32)
    return x, noise


def stream_blocks(x, noise):
    """[(start, T, x block (B, 32, 32 + T), noise block)]: each block behind its
    32 history columns (zeros before the signal starts; zero noise there too,
    so that the history of the first block is the convolution's zero padding)."""
    assert sum(STREAM_BLOCKS) == x.shape[-1]
    xp = np.pad(x, ((0, 0), (0, 0), (STREAM_HIST, 0)))
    npad = np.pad(noise, ((0, 0), (0, 0), (STREAM_HIST, 0)))
    out, s = [], 0
    for T in STREAM_BLOCKS:
        out.append((s, T, np.ascontiguousarray(xp[..., s:s + STREAM_HIST + T]),
                    np.ascontiguousarray(npad[..., s:s + STREAM_HIST + T])))
        s += T
    return out
