"""Plain restatements of the two fused edges (rave_encoder_head and
rave_decoder_tail, rave_amd/csrc/edge_split.hip): each function takes the fields
of rave_edge_args and the precision as ``dtype``, so that one function gives both
the float64 reference and the float32 CPU run whose error against it (``e_ref``,
``with_e_ref``) sets the bounds of tests/test_gpu_edge_sweep.py (4 e_ref for the
exact fp32 kernels, the rule of tests/aux_ref.py).  No GPU, nothing imported from
the library; tests/test_edge_ref_host.py pins these against the oracle on the CPU.

    head   bands[b,k,f] = rh(k, f) sum_j hkf[k,j] x[b, 16 f + j - pqmf_pad_left]        f in [0, F)
           y[b,m,n]     = bias[m] + sum_{k,q} W[m,k,q] bands[b,k,n + q - conv_pad_left]
    tail   c[b,m,f]     = bias[m] + sum_{ci,q} W[m,ci,q] act(x)[b,ci,f + q - conv_pad_left]  f in [0, F)
           s[b,c,f]     = rh(c, f) tanh(c[c] sigmoid(c[c + 16]) (+ noise))   (mode 1; mode 2: tanh(c[c] (+ noise)))
           y[b,16 t+i]  = 16 sum_{k,c} hki[15 - i,c,k] s[b,c,t + k - pqmf_pad_left]

The composition is of what exists: filterbank_ref.analysis / staged / synthesis,
conv_fwd_ref.conv (with the edges' K-chunk of 16 channels) and
conv_grad_ref.act_fwd.  Every sum is one sequential ``_fma`` chain in the K order
edge_split.hip documents: the head's analysis in j order, its conv one chunk of 16
channels (the <= 8 bands) tap-major; the tail's conv 4 chunks of 16 channels by 7
taps, its synthesis in (tap, channel) order.  No np.dot and no np.sum.

The intermediate (the bands; the conv's output and its epilogue) is rounded to
``dtype``, because the exact-fp32 kernels hold it in fp32, and it is *zero outside
[0, F)* before the second stage reads it: the padding is the second stage's, so a
band frame outside the clip is 0 and not the analysis of the zero-extended audio
(which is non-zero there: the 513 taps reach real samples), and a synthesis input
outside the clip is 0 and not tanh(bias).  rh's parity is the global frame's.

``S``, the condition sum per output in float64, through both GEMMs as
conv_fwd_ref.unit carries it.  A rounding error of relative size u in each operand
and each step of a chain sum_i a_i b_i moves the sum by at most about u K sum
|a_i| |b_i|; the first stage's result therefore carries an error bounded by u K
S1, S1 its own condition sum, and the second stage sees an operand that is wrong
by that much, weighted by its |W|.  So:

  head   S_band[k,f] = sum_j |hkf[k,j]| |x[16 f + j - pad]|  (0 outside [0, F)),
         S = |bias| + sum_{k,q} |W[m,k,q]| S_band[k, n + q - pad].
         (|bands| <= S_band, so this also covers the conv's own rounding.)
  tail   S1[m,f] = |bias[m]| + sum |W| |act(x)| is the conv's condition sum.  The
         epilogue e(v, a) = tanh(v sigmoid(a) + noise) is pushed through by its
         Lipschitz factors: |d tanh| <= 1, |d/dv (v sigmoid(a))| = sigmoid(a) <= 1,
         |d/da (v sigmoid(a))| = |v| sigmoid'(a) <= |v| / 4.  Hence
         L[c,f] = S1[c,f] + (|v[c,f]| / 4) S1[c + 16,f]   (mode 1),   L = S1   (mode 2),
         zero outside [0, F) as the staged value is, and
         S[16 t + i] = 16 sum_{k,c} |hki[15 - i,c,k]| (|s| + L)[c, t + k - pad]:
         |s| for the synthesis' own rounding, L for the error it inherits.
"""
import numpy as np

from tests import filterbank_ref as FB
from tests.conv_fwd_ref import conv, with_e_ref                              # noqa: F401
from tests.conv_grad_ref import ACT_LEAKY, ACT_NONE, ACT_SNAKE              # noqa: F401
from tests.filterbank_ref import N_BAND, _window, rh

K7 = 7                  # taps of both edge convs
EDGE_CHUNK = 16         # input channels per K-chunk of both edge convs
ANA_TAPS, SYN_TAPS = 513, 33


def _hkf(hkf):
    return np.asarray(hkf).reshape(N_BAND, -1)


def bands(x, hkf, n_bands, pqmf_pad_left, first, n, dtype=np.float64):
    """Bands of the frames [first, first + n) of the zero-extended audio x (B, 16 F), with
    reverse_half's sign by the global frame: (B, n_bands, n).  (filterbank_ref.analysis counts
    its frames from 0; starting it at ``first`` is a shift of its pad_left, and its sign, taken
    from the local frame, is put right where ``first`` is odd.)"""
    y = FB.analysis(x, _hkf(hkf), pqmf_pad_left - N_BAND * first, n, n_bands, dtype)
    k, t = np.arange(n_bands)[:, None], np.arange(n)[None, :]
    return y * (rh(k, t) * rh(k, first + t)).astype(dtype)[None]


def band_cond(x, hkf, n_bands, pqmf_pad_left, frames):
    """S_band (B, n_bands, frames), float64."""
    x = np.asarray(x)
    h = np.abs(_hkf(hkf)[:n_bands].astype(np.float64))
    taps = h.shape[1]
    xp = np.abs(_window(x, -pqmf_pad_left, N_BAND * (frames - 1) + taps, np.float64))
    at = N_BAND * np.arange(frames)
    S = np.zeros((x.shape[0], n_bands, frames), np.float64)
    for j in range(taps):
        S = S + h[None, :, j, None] * xp[:, None, at + j]
    return S


def head_conv(b, w, bias, conv_pad_left, frames, dtype=np.float64, cond=False):
    """The head's conv over the band frames b (B, c_in, frames'), zero outside them."""
    return conv(b, w, bias, None, None, K7, 1, 1, conv_pad_left, frames, ACT_NONE, 0.0, dtype=dtype, cond=cond,
                chunk=EDGE_CHUNK)


def head(x, hkf, w, bias, conv_pad_left, pqmf_pad_left, frames, dtype=np.float64, cond=False):
    """rave_encoder_head.  x (B, 16 frames), hkf (16, [1,] 513), w (c_out, c_in <= 8, 7), bias (c_out)
    or None -> (B, c_out, frames); with ``cond`` also S."""
    n_bands = np.asarray(w).shape[1]
    b = bands(x, hkf, n_bands, pqmf_pad_left, 0, frames, dtype)
    assert b.dtype == dtype
    y = head_conv(b, w, bias, conv_pad_left, frames, dtype)
    if not cond:
        return y
    wa = np.abs(np.asarray(w, dtype).astype(np.float64))
    ba = None if bias is None else np.abs(np.asarray(bias, dtype).astype(np.float64))
    S = head_conv(band_cond(x, hkf, n_bands, pqmf_pad_left, frames), wa, ba, conv_pad_left, frames)
    return y, S


def tail_conv(x, w, bias, alpha, act, slope, conv_pad_left, frames, dtype=np.float64, cond=False):
    """The tail's act -> conv: x (B, 64, >= frames) -> (B, c_out, frames)."""
    return conv(np.asarray(x)[:, :, :frames], w, bias, alpha, None, K7, 1, 1, conv_pad_left, frames, act, slope,
                dtype=dtype, cond=cond, chunk=EDGE_CHUNK)


def tail_cond(c, S1, hki, mode, noise, pqmf_pad_left, frames):
    """S of the tail from the conv's float64 output c and its condition sum S1."""
    h = np.abs(np.asarray(hki, np.float64))
    taps = h.shape[2]
    s = np.abs(FB.staged(c, 0, mode, 0, 0, noise, frames, np.float64, taps=1))          # |s| on [0, F)
    L = S1[:, :N_BAND]
    if mode == 1:
        L = L + np.abs(c[:, :N_BAND]) / 4.0 * S1[:, N_BAND:2 * N_BAND]
    win = _window(s + L, -pqmf_pad_left, frames + taps - 1, np.float64)
    S = np.zeros((c.shape[0], N_BAND, frames), np.float64)
    for k in range(taps):
        for ch in range(N_BAND):
            S = S + h[None, :, ch, k, None] * win[:, None, ch, k:k + frames]
    S = S * N_BAND
    return np.ascontiguousarray(S[:, ::-1, :].transpose(0, 2, 1)).reshape(c.shape[0], N_BAND * frames)


def tail(x, hki, w, bias, alpha, noise, act, slope, mode, conv_pad_left, pqmf_pad_left, frames, dtype=np.float64,
         cond=False):
    """rave_decoder_tail.  x (B, 64, frames), hki (16, 16, 33), w (32 | 16, 64, 7) for mode 1 | 2, noise
    (B, 16, frames) or None -> (B, 16 frames); with ``cond`` also S."""
    assert mode in (1, 2) and np.asarray(w).shape[0] == (2 if mode == 1 else 1) * N_BAND
    out = tail_conv(x, w, bias, alpha, act, slope, conv_pad_left, frames, dtype, cond)
    c, S1 = out if cond else (out, None)
    assert c.dtype == dtype
    y = FB.synthesis(c, hki, pqmf_pad_left, mode, 0, 0, noise, frames, dtype)
    if not cond:
        return y
    return y, tail_cond(c.astype(np.float64), S1, hki, mode, noise, pqmf_pad_left, frames)
