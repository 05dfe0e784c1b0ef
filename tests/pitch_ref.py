"""CPU reference of the pitch tests: a torch restatement of the YIN half of
rave/pitch_utils.py (_frame :45-49, _diff :52-72, _search :75-86, estimate
:15-42, get_pitch :90-96, one_hot :98-104, quantize_f0_norm / get_f0_norm in
'abs' mode :112-127) that runs in the dtype of its input, and the seeded inputs
the tests run on.  tests/golden/make_pitch_check.py runs the reference's own
functions on the same inputs and checks this restatement against them."""
import functools
import math

import numpy as np
import torch

# name -> (shape, sample_rate, pitch_min, pitch_max, frame stride in seconds or block size, glide range)
#   est:   27 frames, no multiple of anything; short: T < L, one zero-padded frame;
#   wave:  L = 160, one wave per frame, 75 frames (no multiple of the 4 a workgroup takes);
#   block: get_pitch's binding, 16 frames per row = T / 1024;
#   max:   the longest frame the op accepts (L = 4410, three lag passes per thread)
CASES = {
    "est": dict(shape=(3, 5000), sr=44100, pmin=70.0, pmax=400.0, stride=0.01, glide=(80.0, 380.0)),
    "short": dict(shape=(1, 1000), sr=44100, pmin=70.0, pmax=400.0, stride=0.01, glide=(80.0, 380.0)),
    "wave": dict(shape=(3, 4000), sr=16000, pmin=200.0, pmax=2000.0, stride=0.01, glide=(250.0, 1500.0)),
    "block": dict(shape=(2, 1, 16384), sr=44100, pmin=70.0, pmax=400.0, block=1024, glide=(80.0, 380.0)),
    "max": dict(shape=(1, 8000), sr=44100, pmin=20.0, pmax=20000.0, stride=0.02, glide=(80.0, 380.0)),
}
THRESHOLD = 0.1
EXCUSED_CAP = 0.02           # of a shape's frames
ONEHOT_EDGE = 1e-6           # float64 v this close to a bin edge excuses a period
ONEHOT_CAP = 0.01            # of the periods


def glides(shape, sr, f_lo, f_hi, seed, gate=True):
    """float32 `shape` (..., T): per row a harmonic glide between two pitches in
    [f_lo, f_hi] (six partials at 1/k, 20 % vibrato at 5 Hz), gated on and off in
    segments of 40 ms to leave unvoiced gaps, plus 0.02 sigma noise."""
    T = shape[-1]
    rows = int(np.prod(shape[:-1]))
    n = np.arange(T)
    seg = max(1, int(0.04 * sr))
    out = []
    for r in range(rows):
        rng = np.random.Generator(np.random.PCG64(seed + r))
        fa, fb = np.exp(rng.uniform(np.log(f_lo), np.log(f_hi), 2))
        f = fa * (fb / fa) ** (n / max(T - 1, 1))
        f = f * (1.0 + 0.2 * np.sin(2 * np.pi * 5.0 * n / sr + rng.uniform(0, 2 * np.pi)))
        ph = 2 * np.pi * np.cumsum(f) / sr
        s = sum(np.sin(k * ph) / k for k in range(1, 7))
        on = rng.uniform(size=T // seg + 1) < 0.7
        if gate:
            s = s * np.repeat(on, seg)[:T]
        out.append(0.3 * s + 0.02 * rng.standard_normal(T))
    return np.stack(out).astype(np.float32).reshape(shape)


@functools.lru_cache(maxsize=None)
def inputs(case: str) -> np.ndarray:
    c = CASES[case]
    x = glides(c["shape"], c["sr"], *c["glide"], seed=100 * list(CASES).index(case))
    x.setflags(write=False)
    return x


def frame_stride(case: str) -> float:
    """The frame stride in seconds: the case's own, or get_pitch's (pitch_utils.py:91-94)."""
    c = CASES[case]
    if "stride" in c:
        return c["stride"]
    T = c["shape"][-1]
    desired = T / c["block"]
    frame_length = 2 * int(c["sr"] / c["pmin"])
    return (T - frame_length) / (desired - 1) / c["sr"]


def geometry(case: str):
    """(tau_min, tau_max, L, stride in samples, frames per row)."""
    c = CASES[case]
    tau_min, tau_max = int(c["sr"] / c["pmax"]), int(c["sr"] / c["pmin"])
    L = 2 * tau_max
    stride = int(frame_stride(case) * c["sr"])
    T = c["shape"][-1]
    return tau_min, tau_max, L, stride, (1 if T < L else (T - L) // stride + 1)


# ------------------------------------------------------------------ YIN
def frame(signal: torch.Tensor, frame_length: int, stride: int) -> torch.Tensor:
    if signal.shape[-1] < frame_length:
        signal = torch.nn.functional.pad(signal, [0, frame_length - signal.shape[-1]])
    return signal.unfold(dimension=-1, size=frame_length, step=stride)


def diff_fft(frames: torch.Tensor, tau_max: int) -> torch.Tensor:
    """d(tau), tau < tau_max, by the reference's route: the autocorrelation as the
    inverse FFT of the power spectrum, zero-padded to twice the next power of two."""
    n = frames.shape[-1]
    size = 1 << (math.ceil(math.log(n) / math.log(2)) + 1)
    spec = torch.fft.rfft(frames, size, dim=-1)
    r = torch.fft.irfft(spec * spec.conj())[..., :tau_max]
    energy = torch.nn.functional.pad((frames * frames).cumsum(-1), [1, 0])      # energy[i] = sum_{j<i} x_j^2
    c0 = energy[..., -1:]
    ct = energy.flip(-1)[..., :tau_max] - energy[..., :tau_max]                # energy[L - tau] - energy[tau]
    return c0 + ct - 2 * r


def cmdf_of(d: torch.Tensor) -> torch.Tensor:
    lags = torch.arange(1, d.shape[-1])
    return d[..., 1:] * lags / torch.clamp(d[..., 1:].cumsum(-1), min=1e-5)


def search(cmdf: torch.Tensor, tau_max: int, threshold: float) -> torch.Tensor:
    start = (cmdf < threshold).int().argmax(-1, keepdim=True)                  # 0 when none is below
    start = torch.where(start > 0, start, tau_max)                             # index 0 or none: nothing passes
    j = torch.arange(cmdf.shape[-1])
    stops_falling = torch.nn.functional.pad(cmdf.diff() >= 0.0, [0, 1], value=1.0)   # the last index counts
    return ((j >= start) & stops_falling).int().argmax(-1)


def analyse(x: torch.Tensor, sr: int, pmin: float, pmax: float, stride_s: float, threshold: float = THRESHOLD):
    """estimate() with its intermediates: (sliced cmdf, idx, f0), in x's dtype."""
    tau_min, tau_max = int(sr / pmax), int(sr / pmin)
    frames = frame(x, 2 * tau_max, int(stride_s * sr))
    cmdf = cmdf_of(diff_fft(frames, tau_max))[..., tau_min:]
    tau = search(cmdf, tau_max, threshold)
    f0 = torch.where(tau > 0, sr / (tau + tau_min + 1).type(x.dtype), torch.tensor(0).type(x.dtype))
    return cmdf, tau, f0


def estimate(x, sr=44100, pmin=20.0, pmax=20000.0, stride_s=0.01, threshold=THRESHOLD):
    return analyse(torch.as_tensor(x), sr, pmin, pmax, stride_s, threshold)[2]


def get_pitch(x, block_size, fs=44100, pmin=70.0, pmax=400.0):
    desired = x.shape[-1] / block_size
    frame_length = 2 * int(fs / pmin)
    stride_s = (x.shape[-1] - frame_length) / (desired - 1) / fs
    return estimate(x, fs, pmin, pmax, stride_s)


@functools.lru_cache(maxsize=None)
def reference(case: str, dtype: str = "float64"):
    """(cmdf, idx, f0) of the restatement on the case's input, computed once."""
    c = CASES[case]
    x = torch.tensor(inputs(case), dtype=getattr(torch, dtype))
    return analyse(x, c["sr"], c["pmin"], c["pmax"], frame_stride(case))


def margins(cmdf: np.ndarray, threshold: float = THRESHOLD):
    """Per frame of a float64 sliced cmdf (frames, M): the outcome of a plain
    loop over _search's rule and the smallest margin among the comparisons that
    fix it -- cmdf[j] against the threshold up to the first crossing, then
    cmdf[j+1] - cmdf[j] against 0 from there to the chosen index."""
    idx = np.zeros(len(cmdf), np.int64)
    margin = np.full(len(cmdf), np.inf)
    for n, c in enumerate(cmdf):
        M = len(c)
        first = next((j for j in range(M) if c[j] < threshold), None)
        upto = M - 1 if first is None else first
        m = np.abs(c[:upto + 1] - threshold).min()
        if first is not None and first > 0:
            j = first
            while j < M - 1 and not c[j + 1] - c[j] >= 0.0:
                j += 1
            idx[n] = j
            if j > first or j < M - 1:
                m = min(m, np.abs(np.diff(c[first:min(j + 2, M)])).min())
        margin[n] = m
    return idx, margin


# ------------------------------------------------------------------ one-hot
def f0_norm(f0: torch.Tensor) -> torch.Tensor:
    """quantize_f0_norm 'abs' + get_f0_norm's 0.5, with the reference's
    arithmetic as written (log(400 - log 40)); f0 = 0 becomes NaN."""
    f0 = torch.where(f0 == 0, torch.full_like(f0, float("nan")), f0)
    lo, hi = torch.tensor([40]).to(f0), torch.tensor([400]).to(f0)
    return (torch.log(f0) - torch.log(lo)) / torch.log(hi - torch.log(lo)) + 0.5


def f0_classes(f0: torch.Tensor, num_bins: int = 256) -> torch.Tensor:
    """The class index in [0, num_bins] (the -1 of bucketize wraps to the last)."""
    bins = torch.linspace(0, 1, num_bins + 1).to(f0)
    idx = torch.bucketize(f0_norm(f0), bins, right=True) - 1
    return torch.where(idx < 0, idx + num_bins + 1, idx)


def one_hot(a: torch.Tensor, num_classes: int) -> torch.Tensor:
    return torch.eye(num_classes, dtype=torch.float32)[a.reshape(-1)].reshape(a.shape[0], a.shape[1], num_classes)


def f0_one_hot(f0: torch.Tensor, num_bins: int = 256) -> torch.Tensor:
    """get_f0_norm's one-hot (B, frames, num_bins + 1) of an f0 contour (B, frames)."""
    bins = torch.linspace(0, 1, num_bins + 1).to(f0)
    return one_hot(torch.bucketize(f0_norm(f0), bins, right=True) - 1, num_bins + 1)


def table_f0(sr: int = 44100, tau_min: int = 110, tau_max: int = 630) -> np.ndarray:
    """float32 f0 of every integer period in [tau_min + 1, tau_max], then 0, a
    value that drives v < 0 (below 40 exp(-0.5 log(400 - log 40)) = 2.0 Hz) and
    one that drives v >= 1 (above 40 exp(+0.5 ...) = 796 Hz)."""
    periods = np.arange(tau_min + 1, tau_max + 1, dtype=np.float32)
    return np.concatenate([np.float32(sr) / periods, np.float32([0.0, 1.5, 900.0])]).astype(np.float32)
