"""The backwards of the noise filter stage and of eval-mode AdaIN
(rave_noise_synth_backward in rave_amd/csrc/noise.hip, rave_adain_backward in
adain.hip) in closed form in numpy, with the precision as a parameter: one
function gives the float64 reference and the fp32 CPU run whose error against
it (``e_ref``) sets the bound of tests/test_gpu_noise_grad.py (4 e_ref, the
rule of tests/test_gpu_aux_kernels.py).  Beside them the torch restatements of
tests/aux_ref.py's noise_synth (torch.fft, the same operation order) and AdaIN
that autograd differentiates: tests/test_noise_grad_ref_host.py checks the
closed forms against those in float64, and the GPU tests use them as the plain
torch composition.  No GPU, no import of the reference.

Notation: NB = noise_bands, FS = 2 (NB - 1), T = target, v = 2 u - 1, win the
periodic Hann window of length FS.  For every cell (b, frame f, band j)

    s_k    = sigmoid(amp[b, j NB + k, f] - 5)
    gh[n]  = sum_{i=n}^{T-1} gy[b, j, f T + i] v[b, f, j, i - n]
    gir[n] = gh[n] win[n + FS/2]                n <  FS/2
    gir[m] = gh[m + T - FS] win[m - FS/2]       FS/2 <= m < FS
    gA_k   = (c_k / FS) sum_{n<FS} gir[n] cos(2 pi k n / FS)     c_0 = c_{NB-1} = 1, else 2
    gamp[b, j NB + k, f] = gA_k 4.6 s_k^2.3 (1 - s_k)

with 1 - s_k as sigmoid(5 - amp) (by subtraction it has no digits left once
amp > ~20).  The draw u is a constant.

AdaIN: gx = gy / (std_x + 1e-5) std_y where the forward transferred (mode != 2
and both counters, AFTER the forward call, non-zero), gx = gy where it did
not; the statistics are constants in every mode."""
import numpy as np
import torch

PAIRS = [(5, 8), (5, 16), (9, 16)]          # the compiled (noise_bands, target)


# ------------------------------------------------------------------ closed forms (numpy)
def noise_synth_backward(gy, amp, u, n_band: int, noise_bands: int, target: int, dtype=np.float64):
    """gy (B, n_band, F target), amp (B, n_band noise_bands, F), u (B, F, n_band,
    target) -> gamp like amp, in ``dtype``."""
    NB, T = noise_bands, target
    FS, H = 2 * (NB - 1), NB - 1
    assert T >= FS
    one = dtype(1.0)
    a = np.asarray(amp, dtype)
    B, _, F = a.shape
    x = a.reshape(B, n_band, NB, F).transpose(0, 3, 1, 2) - dtype(5.0)          # (B, F, n_band, NB)
    with np.errstate(over="ignore"):
        s = one / (one + np.exp(-x))
        c = one / (one + np.exp(x))                                             # 1 - s
    v = np.asarray(u, dtype) * dtype(2.0) - one                                 # (B, F, n_band, T)
    g = np.asarray(gy, dtype).reshape(B, n_band, F, T).transpose(0, 2, 1, 3)    # (B, F, n_band, T)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(FS) / FS)).astype(dtype)
    gir = np.zeros((B, F, n_band, FS), dtype)
    for q in range(FS):
        n = q if q < H else q + T - FS
        gh = (g[..., n:] * v[..., :T - n]).sum(-1, dtype=dtype)
        gir[..., q] = gh * win[q + H if q < H else q - H]
    k, n = np.arange(NB)[:, None], np.arange(FS)[None, :]
    cos = np.cos(2 * np.pi * ((k * n) % FS) / FS).astype(dtype)                 # (NB, FS)
    ck = np.where((k[:, 0] == 0) | (k[:, 0] == NB - 1), 1.0, 2.0).astype(dtype) / dtype(FS)
    gA = (gir[..., None, :] * cos).sum(-1, dtype=dtype) * ck                    # (B, F, n_band, NB)
    gamp = gA * (dtype(4.6) * s ** dtype(2.3) * c)
    return np.ascontiguousarray(gamp.transpose(0, 2, 3, 1)).reshape(B, n_band * NB, F).astype(dtype)


def adain_transfers(counters_after, mode: int) -> bool:
    return mode != 2 and float(counters_after[0]) != 0 and float(counters_after[1]) != 0


def adain_backward(gy, stats_after, counters_after, mode: int, row0: int, dtype=np.float64):
    """gy (B, C, T), stats (4, max_batch, C) and counters [nx, ny] as the forward
    left them -> gx, in ``dtype``."""
    g = np.asarray(gy, dtype)
    if not adain_transfers(counters_after, mode):
        return g.copy()
    st = np.asarray(stats_after, dtype)
    rows = slice(row0, row0 + g.shape[0])
    return g / (st[1, rows, :, None] + dtype(1e-5)) * st[3, rows, :, None]


# ------------------------------------------------------------------ torch restatements (autograd)
def noise_synth_torch(amp: torch.Tensor, u: torch.Tensor, n_band: int, noise_bands: int, target: int) -> torch.Tensor:
    """tests/aux_ref.noise_synth operation by operation on torch.fft, in amp's
    dtype and on its device; differentiable in amp."""
    s = 1.0 / (1.0 + torch.exp(-(amp - 5.0)))
    a = 2.0 * s ** 2.3 + 1e-7
    B, _, F = a.shape
    a = a.transpose(1, 2).reshape(B, F, n_band, noise_bands)
    ir = torch.fft.irfft(torch.complex(a, torch.zeros_like(a)), dim=-1)
    fs = ir.shape[-1]
    assert fs == 2 * (noise_bands - 1) and target >= fs
    ir = torch.roll(ir, fs // 2, -1)
    ir = ir * torch.hann_window(fs, dtype=ir.dtype, device=ir.device)           # periodic
    ir = torch.nn.functional.pad(ir, (0, target - fs))
    ir = torch.roll(ir, -(fs // 2), -1)
    noise = u.to(amp.dtype) * 2.0 - 1.0
    sig = torch.nn.functional.pad(noise, (0, target))
    ker = torch.nn.functional.pad(ir, (target, 0))
    out = torch.fft.irfft(torch.fft.rfft(sig) * torch.fft.rfft(ker), n=2 * target)[..., target:]
    return out.permute(0, 2, 1, 3).reshape(B, n_band, F * target)


def adain_torch(x: torch.Tensor, stats: torch.Tensor, counters, mode: int, row0: int):
    """tests/aux_ref.adain with the statistics as constants: the update runs on
    x's values (aux_ref.adain itself, detached), the transfer on x.  Returns
    (y, stats after, counters after)."""
    from tests import aux_ref as R
    _, st, cnt = R.adain(x.detach(), stats.detach(), counters, mode, row0)
    if mode != 2 and cnt[0] != 0 and cnt[1] != 0:
        rows = slice(row0, row0 + x.shape[0])
        mx, sx, my, sy = (st[i, rows, :, None] for i in range(4))
        y = (x - mx) / (sx + 1e-5) * sy + my
    else:
        y = x.clone()
    return y, st, cnt
