"""Plain restatements of the small kernels (rave_amd/csrc/misc.hip, noise.hip,
adain.hip, speaker.hip): the counter-based uniform draw in numpy uint64, and
the RVQ, AdaIN, noise-filter and pooling-head arithmetic with the precision as
a parameter, so that one function gives both the float64 reference and the
fp32 CPU run whose error against it (``e_ref``) sets the bound of
tests/test_gpu_aux_kernels.py (4 e_ref, the rule of the pitch and spectrogram
tests).  No GPU, no import of the reference; tests/test_aux_ref_host.py checks
these against the oracle and torch on the CPU.

The uniform draw (rave_fill_uniform).  With mix() the splitmix64 finaliser and
G = 0x9E3779B97F4A7C15 (2^64 / golden ratio):

    key   = mix(seed + G)                      on the host, once per call
    z_i   = mix(key + G (i + 1))               element i, on the device
    u_i   = (z_i >> 40) 2^-24                  24 bits -> [0, 1), exact in fp32
    y_i   = lo + (hi - lo) u_i                 fp32

``key`` is the first output of splitmix64 seeded with ``seed``; within a call
the elements are the outputs of splitmix64 seeded with ``key``.  Hashing the
seed first is what makes the streams of related seeds unrelated: without it
(key = seed) the engine's per-call seeds base + G c put element i of call c at
state base + G (c + i + 1), and call c + 1 is call c moved by one element."""
import numpy as np
import torch

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
ENGINE_BASES = (0x243F6A8885A308D3, 0x13198A2E03707344)     # Model::noise_ptr, stream_dec (engine.cpp)


# ------------------------------------------------------------------ uniform draw
def mix_int(z: int) -> int:
    """splitmix64's finaliser on a Python int (the independent statement the
    numpy one is pinned against)."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def stream_key(seed: int) -> int:
    return mix_int(seed + G)


def uniform_state(seed: int, n: int, hashed_seed: bool = True) -> np.ndarray:
    """The 64-bit state behind each of the first n elements.  hashed_seed=False
    is the draw before the seed was hashed (key = seed), kept to show what the
    engine's schedule did with it."""
    key = np.uint64(stream_key(seed) if hashed_seed else seed & M64)
    with np.errstate(over="ignore"):
        return mix(key + np.uint64(G) * np.arange(1, n + 1, dtype=np.uint64))


def uniform(seed: int, n: int, lo: float = 0.0, hi: float = 1.0, hashed_seed: bool = True) -> np.ndarray:
    u = (uniform_state(seed, n, hashed_seed) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    lo, scale = np.float32(lo), np.float32(hi) - np.float32(lo)
    return (lo + scale * u).astype(np.float32)


def engine_seed(base: int, call: int) -> int:
    """The seed of the engine's call number ``call`` (1-based: ++noise_calls)."""
    return (base + G * call) & M64


def xcorr(a, b, max_lag: int) -> np.ndarray:
    """Normalised cross-correlation of two equally long rows at lags
    -max_lag..max_lag: sum_t a'[t] b'[t + lag] / (|a'| |b'|), a' = a - mean."""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    n = len(a)
    out = []
    for lag in range(-max_lag, max_lag + 1):
        out.append((a[:n - lag] * b[lag:]).sum() if lag >= 0 else (a[-lag:] * b[:n + lag]).sum())
    return np.array(out) / den


def repeat_cap(n: int, bits: int = 24, miss: float = 1e-9) -> int:
    """Largest multiplicity n draws from 2^bits equally likely values may show:
    the expected number of values drawn at least k times is at most
    C(n, k) / 2^(bits (k - 1)) <= n (n / 2^bits)^(k - 1) / k!  (the birthday
    bound for k-fold coincidences); the cap is the smallest k at which the
    bound for k + 1 falls below ``miss``."""
    lam, k, bound = n / 2.0 ** bits, 1, float(n)
    while True:
        bound = bound * lam / (k + 1)          # bound for multiplicity k + 1
        if bound < miss:
            return k
        k += 1


# ------------------------------------------------------------------ RVQ
def rvq_encode(z: np.ndarray, cbs: np.ndarray):
    """float64 ResidualVectorQuantization.encode (rave/quantization.py:131-140,
    302-318): per layer the first index of the smallest |e|^2 - 2 r.e, and that
    layer's top-2 gap.  z (B, D, T), cbs (n_q, K, D) -> idx, gap (B, n_q, T)."""
    B, D, T = z.shape
    r = z.transpose(0, 2, 1).reshape(-1, D).astype(np.float64)
    idx, gaps = [], []
    for E in cbs.astype(np.float64):
        d = (E * E).sum(1)[None] - 2.0 * r @ E.T
        i = d.argmin(1)                                   # first index on ties
        if d.shape[1] > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            gaps.append(two[:, 1] - two[:, 0])
        else:
            gaps.append(np.full(len(d), np.inf))
        idx.append(i)
        r = r - E[i]
    shape = lambda a: np.stack(a, 0).reshape(len(cbs), B, T).transpose(1, 0, 2)
    return shape(idx), shape(gaps)


def rvq_pair_margin(z: np.ndarray, cbs: np.ndarray, pair_of: np.ndarray):
    """For codebooks with duplicated rows: pair_of[q][k] is the smallest index
    holding row k's values.  Returns (the canonical winner per frame and layer,
    the float64 gap between the winner and every code outside its pair)."""
    B, D, T = z.shape
    r = z.transpose(0, 2, 1).reshape(-1, D).astype(np.float64)
    win, margin = [], []
    for q, E in enumerate(cbs.astype(np.float64)):
        d = (E * E).sum(1)[None] - 2.0 * r @ E.T
        i = pair_of[q][d.argmin(1)]
        others = np.where(pair_of[q][None, :] == i[:, None], np.inf, d)
        margin.append(others.min(1) - d[np.arange(len(d)), i])
        win.append(i)
        r = r - E[i]
    shape = lambda a: np.stack(a, 0).reshape(len(cbs), B, T).transpose(1, 0, 2)
    return shape(win), shape(margin)


def rvq_decode(idx: np.ndarray, cbs: np.ndarray) -> np.ndarray:
    """fp32 sum of the clamped indices' codewords in layer order, starting at
    0.0 (ResidualVectorQuantization.decode; the clamp is DiscreteScriptedRAVE's).
    idx (B, n_q, T), cbs (n_q, K, D) fp32 -> (B, D, T) fp32."""
    K = cbs.shape[1]
    k = np.clip(idx, 0, K - 1)
    acc = np.zeros((idx.shape[0], idx.shape[2], cbs.shape[2]), np.float32)
    for q in range(cbs.shape[0]):
        acc = acc + cbs[q][k[:, q, :]]
    return np.ascontiguousarray(acc.transpose(0, 2, 1))


def dup_codebooks(rng, n_q: int, K: int, D: int, pairs):
    """Gaussian codebooks in which row b is a bitwise copy of row a for every
    (a, b) in pairs; also pair_of (n_q, K)."""
    cbs = rng.standard_normal((n_q, K, D)).astype(np.float32)
    pair_of = np.tile(np.arange(K), (n_q, 1))
    for a, b in pairs:
        assert a < b < K
        cbs[:, b] = cbs[:, a]
        pair_of[:, b] = a
    return cbs, pair_of


# Duplicated rows of the tie cases (K = 200: splits of 64 codes, the last one
# ragged with 8).  Within a split, code m sits in wave m / 32, lane half
# (m / 4) % 2, accumulator row by m % 4 and m / 8:
#   (8, 9)     differ by 1: same wave, same lane half, other accumulator row
#   (16, 20)   differ by 4: the other lane half
#   (3, 35)    differ by 32: the other wave
#   (21, 85)   differ by 64: the next split
#   (50, 180)  differ by 130: two splits on
#   (100, 195) ends in the ragged last split; (193, 198) lies inside it
TIE_PAIRS = [(8, 9), (16, 20), (3, 35), (21, 85), (50, 180), (100, 195), (193, 198)]
TIE_K, TIE_NQ, TIE_B, TIE_T = 200, 2, 2, 45
GAP_RULE = 1e-3            # _rvq_encode_np's excuse: float64 top-2 gap below this
EXCUSED_CAP = 0.01


def rvq_tie_case(D: int):
    """(z (B, D, T), cbs, pair_of, wanted idx): every frame is the exact fp32 sum
    of one duplicated row per layer, so each layer's winner is a bitwise tie."""
    rng = np.random.default_rng(100 + D)
    cbs, pair_of = dup_codebooks(rng, TIE_NQ, TIE_K, D, TIE_PAIRS)
    rows = np.array([k for p in TIE_PAIRS for k in p])
    f = np.arange(TIE_B * TIE_T)
    k0, k1 = rows[f % len(rows)], rows[(5 * f + 3) % len(rows)]
    z = (cbs[0][k0] + cbs[1][k1]).reshape(TIE_B, TIE_T, D).transpose(0, 2, 1)
    want = np.stack([pair_of[0][k0], pair_of[1][k1]], 0).reshape(TIE_NQ, TIE_B, TIE_T).transpose(1, 0, 2)
    return np.ascontiguousarray(z), cbs, pair_of, want


# name -> (D, K, n_q): Gaussian codebooks, z = 2 N(0, 1), B = 2, T = 45
RVQ_CASES = {"k40": (64, 40, 3), "k65": (128, 65, 3), "strided": (128, 200, 2)}


def rvq_case(name: str):
    D, K, nq = RVQ_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    cbs = rng.standard_normal((nq, K, D)).astype(np.float32)
    z = (2.0 * rng.standard_normal((TIE_B, D, TIE_T))).astype(np.float32)
    return z, cbs


# ------------------------------------------------------------------ AdaIN
def _mean_std(x):
    """x.mean(-1) and the unbiased x.std(-1) written out as the two passes they
    are (mean, then centred squares), so that the fp32 run accumulates in fp32:
    torch's own fp32 std accumulates in double on the CPU and would set an
    e_ref no fp32 kernel can meet."""
    T = x.shape[-1]
    mean = x.sum(-1) / T
    d = x - mean[..., None]
    return mean, ((d * d).sum(-1) / (T - 1)).sqrt()


def adain(x, stats, counters, mode: int, row0: int):
    """AdaptiveInstanceNormalization.forward in eval mode (rave/blocks.py:856-919)
    in x's dtype.  x (B, C, T); stats (4, max_batch, C) = mean_x, std_x, mean_y,
    std_y; counters [num_update_x, num_update_y].  Returns (y, stats, counters)
    without touching the arguments."""
    stats = stats.clone()
    nx, ny = float(counters[0]), float(counters[1])
    B = x.shape[0]
    rows = slice(row0, row0 + B)
    if mode in (1, 2):
        mean, std = _mean_std(x)
        o, n = (0, nx) if mode == 1 else (2, ny)
        stats[o, rows] = stats[o, rows] + (mean - stats[o, rows]) / (n + 1)
        stats[o + 1, rows] = stats[o + 1, rows] + (std - stats[o + 1, rows]) / (n + 1)
        if mode == 1:
            nx += 1
        else:
            ny += 1
    if mode != 2 and nx != 0 and ny != 0:
        mx, sx, my, sy = (stats[i, rows, :, None] for i in range(4))
        y = (x - mx) / (sx + 1e-5) * sy + my
    else:
        y = x.clone()
    return y, stats, [nx, ny]


# ------------------------------------------------------------------ noise filter stage
def noise_synth(amp: np.ndarray, u: np.ndarray, n_band: int, noise_bands: int, target: int, dtype=np.float64):
    """NoiseGeneratorV2's filter stage after its convs (rave/blocks.py:281-291):
    mod_sigmoid(amp - 5) -> amp_to_impulse_response (irfft, roll, Hann, pad,
    roll; rave/core.py:95-116) -> fft_convolve with 2 u - 1 (the kept half of the
    zero-padded circular product; rave/core.py:119-129), in ``dtype`` (numpy's
    FFT keeps float32).  amp (B, n_band noise_bands, frames), u (B, frames,
    n_band, target) -> (B, n_band, frames target)."""
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    a = np.asarray(amp, dtype)
    one = dtype(1.0)
    s = one / (one + np.exp(-(a - dtype(5.0))))
    a = dtype(2.0) * s ** dtype(2.3) + dtype(1e-7)
    B, _, F = a.shape
    a = a.transpose(0, 2, 1).reshape(B, F, n_band, noise_bands)
    ir = np.fft.irfft(a.astype(ctype), axis=-1).astype(dtype)
    fs = ir.shape[-1]
    assert fs == 2 * (noise_bands - 1) and target >= fs
    ir = np.roll(ir, fs // 2, -1)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(fs) / fs)).astype(dtype)      # periodic Hann
    ir = ir * win
    ir = np.pad(ir, [(0, 0)] * 3 + [(0, target - fs)])
    ir = np.roll(ir, -(fs // 2), -1)
    noise = np.asarray(u, dtype) * dtype(2.0) - one
    sig = np.pad(noise, [(0, 0)] * 3 + [(0, target)])
    ker = np.pad(ir, [(0, 0)] * 3 + [(target, 0)])
    out = np.fft.irfft(np.fft.rfft(sig) * np.fft.rfft(ker), n=2 * target).astype(dtype)
    out = out[..., target:]
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, n_band, F * target)


# ------------------------------------------------------------------ speaker pooling head
def _act(x, act: str, slope: float):
    return torch.where(x < 0, x * slope, x) if act == "leaky" else x


def row_stats(x, act: str, slope: float, var_min: float, var_max: float):
    """mean and sqrt(clamp(unbiased var)) over time (rave/CombinedRave.py:316-318);
    x (B, Ch, T) -> (B, 2 Ch) in x's dtype."""
    a = _act(x, act, slope)
    mean, std = _mean_std(a)
    return torch.cat([mean, (std * std).clamp(var_min, var_max).sqrt()], 1)


def attn_pool(x, logits, act: str, slope: float, var_min: float, var_max: float):
    """Attentive statistics pooling as the reference writes it, one pass
    (rave/CombinedRave.py:320-323): w = softmax_t(logits), mu = sum a w,
    sg = sqrt(clamp(sum a^2 w - mu^2))."""
    a = _act(x, act, slope)
    w = torch.softmax(logits, -1)
    mu = (a * w).sum(-1)
    sg = ((a * a * w).sum(-1) - mu * mu).clamp(var_min, var_max).sqrt()
    return torch.cat([mu, sg], 1)


def linear(x, w, bias=None):
    y = x @ w.T
    return y if bias is None else y + bias


def maxpool(x: np.ndarray, kernel: int) -> np.ndarray:
    """nn.MaxPool1d(kernel): stride = kernel, no padding, the tail dropped."""
    t_out = x.shape[-1] // kernel
    return x[..., :t_out * kernel].reshape(*x.shape[:-1], t_out, kernel).max(-1)


def shift_history(a: np.ndarray, hist: int, t_new: int) -> np.ndarray:
    """cached_conv's cache update: the newest ``hist`` columns move to the front."""
    out = a.copy()
    out[..., :hist] = a[..., t_new:t_new + hist]
    return out


def e_ref_of(fn, *args32):
    """(float64 result, e_ref): fn on the float64 copies of the fp32 torch
    arguments, and the max-abs error of its fp32 run against that."""
    up = [a.double() if isinstance(a, torch.Tensor) else a for a in args32]
    r64 = fn(*up)
    r32 = fn(*args32)
    return r64, float((r32.double() - r64).abs().max())
