"""Plain restatements of the PQMF adjoint kernels (rave_amd/csrc/pqmf_grad.hip),
in the style of tests/filterbank_ref.py and on its helpers: each function takes
the fields of its args struct in include/rave_amd.h and the precision as
``dtype``, so that one function gives the float64 reference and the fp32 CPU run
whose error against it (``e_ref``, filterbank_ref.with_e_ref) sets the bound of
tests/test_gpu_pqmf_grad.py (4 e_ref).  No GPU, no import of the reference;
tests/test_pqmf_grad_ref_host.py pins these against the forward restatements
(the adjoint identity) and against torch autograd on the CPU.

One fused-multiply-add chain per output, in the order the kernels document:

    synthesis  gv[b, c, f] = 16 rh(c, frame0 + f) sum_{k, i} hki[15 - i, c, k] gy[b, 16 (f - k + pad_left) + i]
               (k, i) order; frames f - k + pad_left outside [0, t_in) read as zero
    analysis   gx[b, 16 u + i] = sum_{d, k} hkf[k, 16 d + i] rh(k, t) gy[b, k, t],  t = u + pad_left / 16 - d
               (d, k) order, d < 33, k < n_out_bands; t outside [0, t_out) and taps >= 513 read as zero

The epilogue's derivative is formed in ``dtype`` from the saved inputs the way
the kernel forms it: s = 1 / (1 + exp(-x_a)) (mode 1; s = 1 in mode 2),
u = fma(x_w, s, noise), t = tanh(u), gn = gv fma(-t, t, 1), gx_w = gn s,
gx_a = (gn x_w) (s (1 - s))."""
import numpy as np

from tests.filterbank_ref import N_BAND, _fma, _window, rh

TAPS_S = 33                     # frame taps of both adjoints (33 synthesis taps; ceil(513 / 16) analysis taps)


def synthesis_backward(gy, x, hki, pad_left, mode, frame0, x_len, noise, t_in, dtype=np.float64):
    """rave_pqmf_synthesis_backward.  gy (B, 16 t_in), x (B, 16 or 32, >= x_len) or
    None in mode 0, noise (B, 16, >= x_len) or None -> (B, rows, x_len) with the
    rows of gx (16, or 32 in mode 1) followed, when noise is given, by the 16
    rows of gnoise (``split`` takes them apart)."""
    h = np.asarray(hki, dtype).astype(np.float64)
    assert h.shape[2] == TAPS_S
    gy = np.asarray(gy)
    B = gy.shape[0]
    n = x_len if x_len > 0 else t_in
    g = np.ascontiguousarray(gy.reshape(B, t_in, N_BAND).transpose(0, 2, 1))            # g[b, i, t]
    gw = _window(g, pad_left - (TAPS_S - 1), n + TAPS_S - 1, dtype).astype(np.float64)  # column w: t = pad_left - 32 + w
    acc = np.zeros((B, N_BAND, n), dtype)
    for k in range(TAPS_S):
        for i in range(N_BAND):
            acc = _fma(h[None, N_BAND - 1 - i, :, k, None], gw[:, i, None, TAPS_S - 1 - k:TAPS_S - 1 - k + n], acc)
    sign = rh(np.arange(N_BAND)[:, None], frame0 + np.arange(n)[None, :]).astype(dtype)
    gv = acc * dtype(N_BAND) * sign[None]
    if mode == 0:
        assert noise is None
        return gv
    x = np.asarray(x)
    one = dtype(1.0)
    xw = x[:, :N_BAND, :n].astype(dtype)
    if mode == 1:
        with np.errstate(over="ignore"):
            s = one / (one + np.exp(-x[:, N_BAND:2 * N_BAND, :n].astype(dtype)))
    else:
        s = np.ones_like(xw)
    nz = np.zeros_like(xw) if noise is None else np.asarray(noise)[:, :, :n].astype(dtype)
    t = np.tanh(_fma(xw.astype(np.float64), s.astype(np.float64), nz))
    assert t.dtype == dtype
    gn = gv * _fma(-t.astype(np.float64), t.astype(np.float64), np.ones_like(t))
    out = [gn * s]
    if mode == 1:
        out.append((gn * xw) * (s * (one - s)))
    if noise is not None:
        out.append(gn)
    out = np.concatenate(out, 1)
    assert out.dtype == dtype
    return out


def split(out, mode, with_noise):
    """(gx, gnoise or None) of synthesis_backward's stacked rows."""
    rows = 2 * N_BAND if mode == 1 else N_BAND
    assert out.shape[1] == rows + (N_BAND if with_noise else 0)
    return out[:, :rows], (out[:, rows:] if with_noise else None)


def analysis_backward(gy, hkf, pad_left, t_in, n_out_bands, dtype=np.float64):
    """rave_pqmf_analysis_backward.  gy (B, n_out_bands, t_out), hkf (16, taps) -> (B, t_in)."""
    assert pad_left % N_BAND == 0
    gy = np.asarray(gy)
    B, nb, t_out = gy.shape
    assert nb == n_out_bands
    h = np.asarray(hkf, dtype)[:n_out_bands].astype(np.float64)
    taps = h.shape[1]
    nd = -(-taps // N_BAND)
    hp = np.zeros((n_out_bands, nd * N_BAND))
    hp[:, :taps] = h                                                                    # hp[k, 16 d + i]
    sg = gy.astype(dtype) * rh(np.arange(nb)[:, None], np.arange(t_out)[None, :]).astype(dtype)[None]
    cols = -(-t_in // N_BAND)
    sw = _window(sg, pad_left // N_BAND - (nd - 1), cols + nd - 1, dtype).astype(np.float64)
    acc = np.zeros((B, N_BAND, cols), dtype)
    for d in range(nd):
        for k in range(n_out_bands):
            acc = _fma(hp[None, k, N_BAND * d:N_BAND * (d + 1), None], sw[:, k, None, nd - 1 - d:nd - 1 - d + cols], acc)
    return np.ascontiguousarray(acc.transpose(0, 2, 1)).reshape(B, cols * N_BAND)[:, :t_in]


# ------------------------------------------------------------------ closed forms
def analysis_backward_impulse(hkf, k, t, pad_left, t_in):
    """analysis backward of a unit cotangent at band k, frame t:
    gx[s] = rh(k, t) hkf[k, s + pad_left - 16 t]."""
    h = np.asarray(hkf)
    j = np.arange(t_in) + pad_left - N_BAND * t
    ok = (j >= 0) & (j < h.shape[1])
    return (np.where(ok, h[k, np.clip(j, 0, h.shape[1] - 1)], 0) * float(rh(k, t))).astype(h.dtype)


def synthesis_backward_impulse(hki, s, pad_left, frame0, x_len):
    """synthesis backward (mode 0) of a unit cotangent at sample s = 16 t + i:
    gx[c, f] = 16 rh(c, frame0 + f) hki[15 - i, c, f - t + pad_left]."""
    h = np.asarray(hki)
    t, i = divmod(s, N_BAND)
    k = np.arange(x_len) - t + pad_left
    ok = (k >= 0) & (k < h.shape[2])
    g = np.where(ok[None, :], h[N_BAND - 1 - i][:, np.clip(k, 0, h.shape[2] - 1)], 0)     # (c, f)
    sign = rh(np.arange(N_BAND)[:, None], frame0 + np.arange(x_len)[None, :])
    return (N_BAND * sign * g).astype(h.dtype)
