"""CPU reference of the spectral-loss tests: a torch.stft restatement of
stft_loss.MultiResolutionSTFTLoss (rave/stft_loss.py:12-144) in the dtype of its
inputs, a differentiable AudioDistanceV1 on tests/distance_ref.py's stft_mag,
gradients by torch autograd, a direct DFT evaluation of the definition, and the
seeded inputs the tests run on.  tests/golden/make_stft_loss_check.py checks the
restatement against the reference's own functions in float64 (1e-12 relative)."""
import math

import numpy as np
import torch

from tests import distance_ref

POWER_CLAMP = 1e-7                                   # stft_loss.py:35
# (2, 4096); (3, 5000): T no multiple of any hop; (1, 2049): the smallest T that
# n_fft = 4096's reflect pad accepts, the pads spanning nearly the whole signal
MR_CASES = {"a": (2, 4096), "b": (3, 5000), "c": (1, 2049)}
ODD = ((64, 5, 37),)                                 # an odd small geometry off the fork's numbers
ODD_SHAPE = (2, 300)


def fork_resolutions(sr: int = 44100):
    """rave/model.py:191-196."""
    res = []
    for hop_ms, win_ms in ((5, 25), (10, 50), (2, 10)):
        hop, win = int(0.001 * hop_ms * sr), int(0.001 * win_ms * sr)
        res.append((int(math.pow(2, int(math.log2(win)) + 1)), hop, win))
    return tuple(res)


def synth(rows: int, t: int, seed0: int):
    """(pred, target) float32 (rows, T): distance_ref.inputs' signal -- per row a
    440 Hz sine plus 0.1 N(0,1) -- as the target, pred = target + 0.03 N(0,1)."""
    n = np.arange(t)
    tgt = []
    for r in range(rows):
        rng = np.random.Generator(np.random.PCG64(seed0 + r))
        tgt.append(0.3 * np.sin(2 * np.pi * 440 * n / 48000) + 0.1 * rng.standard_normal(t))
    target = np.stack(tgt).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(1000 + seed0))
    pred = (target + 0.03 * rng.standard_normal(target.shape)).astype(np.float32)
    return pred, target


def mr_inputs(case: str):
    rows, t = MR_CASES[case]
    return synth(rows, t, 100 + 10 * list(MR_CASES).index(case))


def odd_inputs():
    return synth(*ODD_SHAPE, 200)


def power(x: torch.Tensor, n_fft: int, hop: int, win: int) -> torch.Tensor:
    """x (B, T) -> (B, n_fft/2 + 1, frames) re^2 + im^2 of torch.stft with the
    reference's arguments (center, reflect, onesided, periodic Hann of length win)."""
    z = torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=x.dtype),
                   return_complex=True)
    return z.real ** 2 + z.imag ** 2


def mr_mag(x, n_fft, hop, win):
    return torch.sqrt(torch.clamp(power(x, n_fft, hop, win), min=POWER_CLAMP)).transpose(2, 1)


def mr_terms(pred: torch.Tensor, target: torch.Tensor, resolutions):
    """[(sc, mag)] per resolution, tensors on the autograd graph of pred."""
    out = []
    for n_fft, hop, win in resolutions:
        p, t = mr_mag(pred, n_fft, hop, win), mr_mag(target, n_fft, hop, win)
        sc = torch.norm(t - p, p="fro") / torch.norm(t, p="fro")
        mag = torch.nn.functional.l1_loss(torch.log(t), torch.log(p))
        out.append((sc, mag))
    return out


def mr_loss(pred, target, resolutions):
    terms = mr_terms(pred, target, resolutions)
    return sum(s for s, _ in terms) / len(terms), sum(m for _, m in terms) / len(terms)


def clamped_share(pred: torch.Tensor, resolutions) -> float:
    """Share of pred's bins under the power clamp."""
    under = total = 0
    for n_fft, hop, win in resolutions:
        pw = power(pred, n_fft, hop, win)
        under += int((pw < POWER_CLAMP).sum())
        total += pw.numel()
    return under / total


def v1_distance(x: torch.Tensor, y: torch.Tensor, scales=distance_ref.DEFAULT_SCALES, log_epsilon: float = 1e-7):
    """distance_ref.distance as a tensor on y's autograd graph; x (B, C, T) is the target."""
    d = 0.
    for n in scales:
        sx, sy = distance_ref.stft_mag(x, n), distance_ref.stft_mag(y, n)
        d = d + ((sx - sy) ** 2).mean() / (sx * sx).mean()
        d = d + (torch.log(sx + log_epsilon) - torch.log(sy + log_epsilon)).abs().mean()
    return d


def grad_of(fn, value: np.ndarray, dtype):
    """(loss values, gradients): fn maps the value tensor to a tuple of scalars;
    one gradient with respect to the value per scalar."""
    v = torch.from_numpy(value).to(dtype).requires_grad_(True)
    outs = fn(v)
    grads = [torch.autograd.grad(o, v, retain_graph=True)[0] for o in outs]
    return [float(o.detach()) for o in outs], grads


def dft_terms(pred: np.ndarray, target: np.ndarray, n_fft: int, hop: int, win: int):
    """(sc, mag) of one resolution from the definition, float64 numpy, no FFT:
    reflect pad of n_fft/2, 1 + T // hop frames, the periodic Hann window of
    length win at offset (n_fft - win) // 2 of the FFT buffer, bins 0..n_fft/2."""
    def mags(x):
        x = np.asarray(x, np.float64)
        t = x.shape[-1]
        xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
        w = np.zeros(n_fft)
        off = (n_fft - win) // 2
        w[off:off + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
        frames = 1 + t // hop
        k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None]
        basis = np.exp(-2j * np.pi * k / n_fft)                      # (bins, n_fft)
        fr = np.stack([xp[:, f * hop:f * hop + n_fft] * w for f in range(frames)], 1)   # (B, frames, n_fft)
        z = fr @ basis.T
        return np.sqrt(np.maximum(z.real ** 2 + z.imag ** 2, POWER_CLAMP))
    p, t = mags(pred), mags(target)
    sc = np.sqrt(((t - p) ** 2).sum()) / np.sqrt((t ** 2).sum())
    return float(sc), float(np.abs(np.log(t) - np.log(p)).mean())
