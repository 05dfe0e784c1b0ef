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


def glides(shape, sr, f_lo, f_hi, seed, gate=True, vibrato=0.2):
    """float32 `shape` (..., T): per row a harmonic glide between two pitches in
    [f_lo, f_hi] (six partials at 1/k, `vibrato` (20 %) at 5 Hz), gated on and off in
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
        f = f * (1.0 + vibrato * np.sin(2 * np.pi * 5.0 * n / sr + rng.uniform(0, 2 * np.pi)))
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
    # the reference's own floor division: at n = 512 it gives 2048 where ceil(log n / log 2) gives 1024
    size = int(2 ** (-int(-math.log(n) // math.log(2)) + 1))
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


# ------------------------------------------------------------------ exact sums
def _exact(frames: np.ndarray, tau_max: int):
    """(d, cond) of float64 frames (N, L): d(tau) = sum_{j < L - tau} (x_j - x_{j+tau})^2,
    YIN's definition, and cond(tau) = c0 + sq[L - tau] + sq[tau] + 2 sum_j |x_j x_{j+tau}|,
    the magnitudes the three-sum formula adds up (sq[i] = sum_{j < i} x_j^2, c0 = sq[L])."""
    f = np.asarray(frames, np.float64)
    N, L = f.shape
    sq = np.concatenate([np.zeros((N, 1)), np.cumsum(f * f, -1)], -1)
    d, cond = np.empty((N, tau_max)), np.empty((N, tau_max))
    with np.errstate(all="ignore"):
        for tau in range(tau_max):
            a, b = f[:, :L - tau], f[:, tau:]
            d[:, tau] = ((a - b) ** 2).sum(-1)
            cond[:, tau] = sq[:, L] + sq[:, L - tau] + sq[:, tau] + 2 * np.abs(a * b).sum(-1)
    return d, cond


def d_truth(frames, tau_max: int) -> np.ndarray:
    """d(tau), tau < tau_max, of float64 frames (N, L) by YIN's definition.  The
    FFT formula equals it algebraically; a difference of two fp32 values is exact
    in double and every term is non-negative, so this form cancels nothing."""
    return _exact(frames, tau_max)[0]


def cmdf_truth(frames, tau_max: int) -> np.ndarray:
    """The unsliced cmdf (N, tau_max - 1) of d_truth, by cmdf_of."""
    return cmdf_of(torch.from_numpy(d_truth(frames, tau_max))).numpy()


def cmdf_bound(frames, tau_max: int) -> np.ndarray:
    """Worst-case forward error (N, tau_max - 1) of any double evaluation, in any
    summation order, of cmdf = d tau / max(S, 1e-5) with d = c0 + (sq[L - tau] -
    sq[tau]) - 2 r(tau) and S the running sum of d.  Products of fp32 values are
    exact in double, each sum has at most L terms and four more roundings join
    them, so with gamma = (L + 4) 2^-53
        dd(tau)   = gamma (c0 + sq[L - tau] + sq[tau] + 2 sum_j |x_j x_{j+tau}|)
        dcmdf(tau) = (tau dd(tau) + |cmdf(tau)| sum_{k <= tau} dd(k)) / max(S, 1e-5),
    the second term only where the clamp is idle (a clamped denominator is the
    constant 1e-5).  A silent frame has bound 0.  Derived, not measured."""
    d, cond = _exact(frames, tau_max)
    L = np.asarray(frames).shape[-1]
    dd = (L + 4) * 2.0 ** -53 * cond[:, 1:]
    lags = np.arange(1, tau_max)
    with np.errstate(all="ignore"):
        S = np.cumsum(d[:, 1:], -1)
        den = np.maximum(S, 1e-5)
        cm = d[:, 1:] * lags / den
        return (lags * dd + np.where(S >= 1e-5, np.abs(cm) * np.cumsum(dd, -1), 0.0)) / den


# ------------------------------------------------------------------ the edge sweep
# Seeded cases for tests/test_pitch_host.py and tests/test_gpu_pitch_edges.py, at
# sr 16000 with pmin = sr / (tau_max + 0.5), pmax = sr / (tau_min + 0.5).
#   sweep:  tau_max on both sides of the launch forms' border (256), every
#           tau_max % 4, L % 4 == 2, frames too small to give every thread a
#           lag, the longest frame; per case 2-3 glide rows and the SPECIAL
#           rows, 5 frames a row (50 or 55 frames, never whole workgroups of 4)
#   frame:  t_len around L and L + stride, stride 1 .. beyond L, 1-7 frames
#   thr:    thresholds at and beyond the cmdf's range, one geometry per form
SWEEP_SR = 16000
SWEEP_TAU_MAX = (3, 4, 5, 63, 64, 65, 66, 254, 255, 256, 257, 258, 259, 260, 513, 1023, 2205)
SPECIAL = ("silence", "dc", "impulse", "sine_min", "sine_last", "falling", "nan", "inf")
FRAME_TAU_MAX = (5, 64, 257)
THRESHOLDS = (0.0, -1.0, 2.0, float("inf"), THRESHOLD)


def _case(kind, tau_min, tau_max, stride, T, rows, seed, threshold=THRESHOLD):
    sr = SWEEP_SR
    pmin, pmax = sr / (tau_max + 0.5), sr / (tau_min + 0.5)
    stride_s = (stride + 0.5) / sr
    assert int(sr / pmin) == tau_max and int(sr / pmax) == tau_min and int(stride_s * sr) == stride
    L = 2 * tau_max
    return dict(kind=kind, sr=sr, pmin=pmin, pmax=pmax, tau_min=tau_min, tau_max=tau_max, L=L, m=tau_max - 1 - tau_min,
                stride=stride, stride_s=stride_s, T=T, rows=tuple(rows), seed=seed, threshold=threshold,
                frames=1 if T < L else (T - L) // stride + 1)


def _build_cases():
    out = {}
    for n, tau_max in enumerate(SWEEP_TAU_MAX):
        L = 2 * tau_max
        stride = max(1, L // 3)
        tau_mins = sorted({t for t in (0, 1, tau_max // 5, tau_max - 2) if t < tau_max - 1})
        for k, tau_min in enumerate(tau_mins):
            if tau_max == 2205:                   # the longest frame: two frames of one glide
                rows, T = ("glide",), L + stride
            else:
                rows, T = ("glide",) * (2 + (n + k) % 2) + SPECIAL, L + 4 * stride + 1
            out[f"sweep-{tau_max}-{tau_min}"] = _case("sweep", tau_min, tau_max, stride, T, rows, 1000 + 10 * n + k)
    for n, tau_max in enumerate(FRAME_TAU_MAX):
        L, k = 2 * tau_max, 0
        for stride in (1, 3, L, L + 5):
            lens = [(T, 1 + (k + i) % 3) for i, T in enumerate((1, L - 1, L, L + 1, L + stride - 1, L + stride))]
            if stride <= 3:
                lens += [(L + 4 * stride, 1), (L + 6 * stride, 1)]       # 5 and 7 frames of one row
            for T, rows in lens:
                k += 1
                out[f"frame-{tau_max}-{stride}-{T}"] = _case("frame", tau_max // 5, tau_max, stride, T,
                                                             ("glide",) * rows, 2000 + 100 * n + k)
    for n, (tau_min, tau_max) in enumerate(((0, 64), (51, 257))):
        L = 2 * tau_max
        for k, thr in enumerate(THRESHOLDS):
            out[f"thr-{tau_max}-{thr}"] = _case("thr", tau_min, tau_max, L // 3, L + 4 * (L // 3) + 1,
                                                ("glide",) * 3, 3000 + n, thr)
    return out


SWEEP = _build_cases()


def _periodic(T, period, phase=0.3):
    """0.5 cos of an integer period, one period tabulated and repeated, so that
    x[n + period] == x[n] bit for bit and d(period) is exactly 0."""
    table = 0.5 * np.cos(2 * np.pi * np.arange(period) / period + phase)
    return table[np.arange(T) % period]


@functools.lru_cache(maxsize=None)
def sweep_input(name: str) -> np.ndarray:
    """float32 (rows, T).  Glide rows span the searched pitches; the special rows:
    silence; the first glide + 10.0; one impulse; a cosine of period tau_min + 1
    (cmdf[0] is 0: every frame unvoiced); one of period tau_max - 1 (the last
    searched index); a sine whose period lies 3 % of tau_max (at least 2 lags)
    beyond the last searched lag, so the cmdf is below the threshold and still
    falling at the end; the second glide with one NaN, and with one inf, at T // 2."""
    c = SWEEP[name]
    T, tau_min, tau_max, sr = c["T"], c["tau_min"], c["tau_max"], c["sr"]
    n_glide = c["rows"].count("glide")
    f_lo = 2.0 * c["pmin"]                            # four periods and more to a frame
    g = glides((n_glide, T), sr, f_lo, max(min(0.8 * c["pmax"], 6.0 * c["pmin"], 0.45 * sr), 1.25 * f_lo), c["seed"],
               gate=T >= 2 * int(0.04 * sr) and tau_max <= 513,      # not a short row as a whole, nor inside long frames
               vibrato=0.2 if tau_max <= 260 else 0.01)
    rows = []
    for kind in c["rows"][n_glide:]:
        r = np.zeros(T)
        if kind == "dc":
            r = g[0].astype(np.float64) + 10.0
        elif kind == "impulse":
            r[T // 2] = 0.7
        elif kind == "sine_min":
            r = _periodic(T, tau_min + 1)
        elif kind == "sine_last":
            r = _periodic(T, tau_max - 1)
        elif kind == "falling":
            r = 0.5 * np.sin(2 * np.pi * np.arange(T) / (tau_max - 1 + max(2.0, 0.03 * tau_max)))
        elif kind in ("nan", "inf"):
            r = g[1].astype(np.float64)
            r[T // 2] = float(kind)
        rows.append(r)
    x = np.concatenate([g, np.stack(rows).astype(np.float32)]) if rows else g
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sweep_truth(name: str) -> dict:
    """Everything the tests judge a case by, computed once, per (row, frame):
    cmdf / bound (sliced, float64), idx / margin (margins() of the truth), limit
    (the frame's largest bound: the margin below which a frame is excused),
    poisoned (the frame holds a NaN or inf: f0 = 0, cmdf all NaN, nothing else
    judged), fft64 / fft32 (the restatement's sliced cmdf in both dtypes) and
    idx_fft64 / idx_fft32."""
    c = SWEEP[name]
    x = sweep_input(name)
    R, F, m, tau_min, tau_max = len(x), c["frames"], c["m"], c["tau_min"], c["tau_max"]
    fr = frame(torch.tensor(x, dtype=torch.float64), c["L"], c["stride"]).numpy()
    assert fr.shape == (R, F, c["L"])
    fr = fr.reshape(R * F, c["L"])
    poisoned = ~np.isfinite(fr).all(-1)
    cm = cmdf_truth(fr, tau_max)[:, tau_min:]
    bound = cmdf_bound(fr, tau_max)[:, tau_min:]
    idx, margin = margins(np.where(poisoned[:, None], 1.0, cm), c["threshold"])
    idx[poisoned] = 0
    margin[poisoned] = np.inf
    limit = np.where(poisoned, 0.0, np.where(poisoned[:, None], 0.0, bound).max(-1))
    out = dict(cmdf=cm, bound=bound, idx=idx, margin=margin, limit=limit, poisoned=poisoned)
    for dt in ("float64", "float32"):
        with np.errstate(all="ignore"):
            cf, i, _ = analyse(torch.tensor(x, dtype=getattr(torch, dt)), c["sr"], c["pmin"], c["pmax"],
                               c["stride_s"], c["threshold"])
        out["fft" + dt[5:]] = cf.double().numpy().reshape(R * F, m)
        out["idx_fft" + dt[5:]] = i.numpy().reshape(R * F)
    return {k: v.reshape((R, F) + v.shape[1:]) for k, v in out.items()}


def intended(name: str) -> dict:
    """What each special row of a sweep case was built to produce, as row name ->
    ("unvoiced" | "last" | "first0"): "first0" is unvoiced because cmdf[0] is
    below the threshold, "last" has every frame choose index m - 1.  The tiny
    frames (tau_max <= 5) still pin "last" with the period tau_max - 1 wherever two
    lags or more are searched, but have no room for a cmdf that is below the
    threshold and still falling; tau_min = tau_max - 2 (one searched lag) has room
    for neither.  There the rows are judged against the truth alone."""
    c = SWEEP[name]
    if "silence" not in c["rows"]:
        return {}
    want = dict(silence="first0", impulse="unvoiced", sine_min="first0")
    if c["tau_max"] >= 63 and c["tau_min"] <= c["tau_max"] // 5:
        want.update(sine_last="last", falling="last")
    elif c["tau_max"] <= 5 and c["m"] > 1:
        want.update(sine_last="last")
    return want


# ------------------------------------------------------------------ one-hot
F0_LO, F0_HI = 40.0, 400.0
LOG_LO, LOG_SPAN = math.log(F0_LO), math.log(F0_HI - math.log(F0_LO))      # f0_norm's constants, as the kernel gets them
ONEHOT_SPECIAL = (0.0, -0.0, -1.0, float("inf"), float("nan"), 1e-40, 1.5, 900.0)
ONEHOT_FAR = 128             # fp32 ulps from an edge at which float64 is clear of ONEHOT_EDGE


def onehot_edges(bins: int, seed: int = 7):
    """(f0, k, off): float32 values around the class edges exp(LOG_LO + (k / bins -
    0.5) LOG_SPAN), k in [0, bins] (a seeded 512 of them for bins = 4096), built
    in float64: the rounded edge and its fp32 neighbours at off = +-1, +-2 and
    +-ONEHOT_FAR ulp."""
    k = np.arange(bins + 1)
    if bins == 4096:
        k = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(bins + 1, 512, replace=False))
    edge = np.exp(LOG_LO + (k / bins - 0.5) * LOG_SPAN).astype(np.float32)
    offs = np.array([0, 1, -1, 2, -2, ONEHOT_FAR, -ONEHOT_FAR])
    f0 = (edge.view(np.int32)[:, None] + offs[None, :]).astype(np.int32).view(np.float32)
    return f0.reshape(-1), np.repeat(k, len(offs)), np.tile(offs, len(k))


def onehot_sample(n: int, seed: int = 11) -> np.ndarray:
    """float32: n log-uniform f0 in [1.5, 900] Hz (both ends outside the classes)."""
    u = np.random.Generator(np.random.PCG64(seed)).uniform(math.log(1.5), math.log(900.0), n)
    return np.exp(u).astype(np.float32)


def f0_norm(f0: torch.Tensor) -> torch.Tensor:
    """quantize_f0_norm 'abs' + get_f0_norm's 0.5, with the reference's
    arithmetic as written (log(400 - log 40)); f0 = 0 becomes NaN."""
    f0 = torch.where(f0 == 0, torch.full_like(f0, float("nan")), f0)
    lo, hi = torch.tensor([F0_LO]).to(f0), torch.tensor([F0_HI]).to(f0)
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
