"""The cached (streaming) mode of the model from its definition -- TEST
INFRASTRUCTURE ONLY, plain numpy, float64 or float32.

``cc.use_cached_conv(True)`` turns every operator of the reference's graph into
a stateful one (cached-conv>=2.5.0, restated in rave_amd/cc.py and SURVEY.md
section 8a rows 6-8).  ``StreamRef`` states that mode on the offline oracle
(oracle/rave_oracle.py: its conv primitives, weights, activations, AdaIN,
noise filter stage and RVQ), one cache per module, any block length on any
call:

* CachedPadding1d(n)          -- prepend the last n columns of [cache | x] of
  the call before (zeros at first); ``crop`` drops as many at the end, which
  makes it a delay line.  It works for a block shorter than n.
* CachedConv1d, padding (l, r) -- a ``stride_delay`` crop-pad (s - r % s) % s,
  then an l + r input cache, then the conv with no padding.  It lags the
  offline conv by (r + stride_delay) / s output columns.
* CachedConvTranspose1d(2r, r, r//2) -- the full (uncropped) transposed conv
  of the block, the first r columns summed with the r columns the call before
  left over, the last r kept for the next: the offline output delayed by r//2.
* Residual = AlignBranches(unit, Identity, delays=[d, 0]) -- the identity
  branch delayed by the unit's delay d (its k-3 conv's r).
* CachedPQMF -- forward: 512 audio samples of history, the stride-16 conv,
  reverse_half on the call's frames; inverse: 32 frames of history of the
  generator's pre-epilogue output and of the noise, the epilogue (amplitude
  modulation, noise, tanh) and reverse_half over [history | block], the k-33
  conv, the band flip and the interleave.  A zero history is a zero epilogue
  output (tanh(0 sigmoid(0) + 0) = 0), so this is CachedConv1d's cache of the
  epilogue's output, as the reference holds it.
* NoiseGeneratorV2 -- its strided convs (padding (r, 0)) cache r columns; the
  filter stage is per noise frame and has no state.  Its output is summed with
  the waveform conv's unaligned, as the reference does.
* AdaIN -- per call, on the call's columns (``Oracle._adain``).
* RVQ -- stateless (``Oracle.rvq_encode`` / ``rvq_decode``).

With ``dtype=np.float32`` every tensor, weight and sum is float32 (the noise
filter stage and AdaIN compute in float64 from float32 inputs and are rounded
back): the yardstick for what a float32 implementation can reach.  Nothing
here imports rave_amd.cc (which loads the GPU ops).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from oracle.rave_oracle import F64, Oracle, conv1d, conv_transpose1d, get_padding, reverse_half


def conv_valid(x, w, b, stride, dilation, dtype):
    """The unpadded conv in ``dtype``: the oracle's in float64, the same
    im2col + matmul with float32 operands and sums in float32."""
    if dtype == F64:
        return conv1d(x, w, b, stride, dilation)
    x = np.ascontiguousarray(x, dtype)
    B, C, T = x.shape
    Co, Ci, K = w.shape
    assert Ci == C, (w.shape, x.shape)
    To = (T - ((K - 1) * dilation + 1)) // stride + 1
    sb, sc, st = x.strides
    cols = np.lib.stride_tricks.as_strided(x, shape=(B, C, K, To), strides=(sb, sc, st * dilation, st * stride))
    y = np.einsum("ock,bckt->bot", np.asarray(w, dtype), cols, optimize=True)
    if b is not None:
        y += np.asarray(b, dtype)[None, :, None]
    assert y.dtype == dtype
    return y


def conv_transpose_full(x, w, stride, dtype):
    """ConvTranspose1d with padding 0 (every output column), in ``dtype``."""
    if dtype == F64:
        return conv_transpose1d(x, w, stride, 0)
    x = np.asarray(x, dtype)
    B, _, T = x.shape
    _, Co, K = w.shape
    full = np.zeros((B, Co, (T - 1) * stride + K), dtype)
    for k in range(K):
        full[:, :, k:k + (T - 1) * stride + 1:stride] += np.einsum("io,bit->bot", np.asarray(w[:, :, k], dtype), x,
                                                                   optimize=True)
    return full


class StreamRef(Oracle):
    """The model of ``Oracle`` in cached mode: ``encode`` / ``decode`` /
    ``encode_codes`` / ``decode_codes`` take one block and keep the caches;
    ``reset()`` zeroes them (AdaIN statistics are the model's, not the
    stream's, and stay)."""

    def __init__(self, cfg, params, speaker, hk=None, adain_stats=None, dtype=np.float64):
        super().__init__(cfg, params, speaker, hk=hk, adain_stats=adain_stats)
        self.dtype = np.dtype(dtype).type
        assert self.dtype in (np.float64, np.float32)
        self.state: Dict[str, np.ndarray] = {}
        self._weights: Dict[str, np.ndarray] = {}

    def reset(self) -> None:
        self.state.clear()

    # -------------------------------------------------------------- state
    def _cached_pad(self, key: str, x: np.ndarray, n: int, crop: bool = False) -> np.ndarray:
        """CachedPadding1d(n, crop)."""
        if n == 0:
            return x
        st = self.state.get(key)
        if st is None:
            st = np.zeros(x.shape[:2] + (n,), self.dtype)
        assert st.shape[:2] == x.shape[:2], (key, st.shape, x.shape)
        full = np.concatenate([st, x], -1)
        self.state[key] = full[..., full.shape[-1] - n:].copy()
        return full[..., :x.shape[-1]] if crop else full

    def _weight(self, name: str, wn: bool) -> np.ndarray:
        if name not in self._weights:
            self._weights[name] = np.ascontiguousarray(self._w(name, wn), self.dtype)   # folded in float64, then rounded
        return self._weights[name]

    # -------------------------------------------------------------- operators
    def _act(self, x, module):
        if self.dtype == F64:
            return super()._act(x, module)
        x = np.asarray(x, self.dtype)
        if self.cfg.activation == "snake":
            a = np.asarray(self.p[module + ".alpha"], self.dtype).reshape(1, -1, 1)
            y = x + (self.dtype(1) / (a + self.dtype(1e-9))) * np.sin(a * x) ** 2
        else:
            y = np.where(x > 0, x, x * self.dtype(self.cfg.leaky_slope))
        assert y.dtype == self.dtype
        return y

    def _conv(self, x, name, k, stride=1, dilation=1, wn=True, pad=None):
        """CachedConv1d (built with cumulative_delay 0, as the module tree builds every conv)."""
        if pad is None:
            pad = get_padding(k, stride, dilation, self.cfg.causal)
        l, r = pad
        stride_delay = (stride - r % stride) % stride
        x = np.asarray(x, self.dtype)
        x = self._cached_pad(name + ".downsampling_delay", x, stride_delay, crop=True)
        x = self._cached_pad(name + ".cache", x, l + r)
        y = conv_valid(x, self._weight(name, wn), self._b(name), stride, dilation, self.dtype)
        if self.record:
            self.trace[name] = y
        return y

    def _conv_transpose(self, x, name, r):
        """CachedConvTranspose1d(2r, stride r, padding r//2)."""
        x = np.asarray(x, self.dtype)
        full = conv_transpose_full(x, self._weight(name, True), r, self.dtype)     # (T + 1) r columns
        key = name + ".cache"
        st = self.state.get(key)
        if st is not None:
            full[..., :r] += st
        self.state[key] = full[..., full.shape[-1] - r:].copy()
        y = full[..., :x.shape[-1] * r]
        b = self._b(name)
        if b is not None:
            y = y + np.asarray(b, self.dtype)[None, :, None]
        return y

    def _adain(self, x, name):
        return np.asarray(super()._adain(np.asarray(x, self.dtype), name), self.dtype)

    def unit_delay(self, dilation: int) -> int:
        return get_padding(self.cfg.kernel_size, 1, dilation, self.cfg.causal)[1]

    def _dilated_residual(self, x, res, d):
        """Residual(DilatedUnit): the identity branch waits for the unit."""
        unit = f"{res}.aligned.branches.0.net"
        x = np.asarray(x, self.dtype)
        h = self._act(x, f"{unit}.0")
        h = self._conv(h, f"{unit}.1", self.cfg.kernel_size, dilation=d)
        h = self._act(h, f"{unit}.2")
        h = self._conv(h, f"{unit}.3", 1)
        return self._cached_pad(f"{res}.aligned.paddings.1", x, self.unit_delay(d), crop=True) + h

    # -------------------------------------------------------------- pqmf
    def pqmf_analysis(self, x):
        x = np.asarray(x, self.dtype)
        k = self.hkf.shape[-1]
        xc = self._cached_pad("pqmf.forward_conv.cache", x, k - 1)
        y = conv_valid(xc, np.asarray(self.hkf, self.dtype), None, self.hk.shape[0], 1, self.dtype)
        assert y.shape[-1] == x.shape[-1] // self.hk.shape[0]
        return reverse_half(y)

    def _synthesis(self, wave, noise):
        """CachedPQMF.inverse of the generator's epilogue."""
        m = self.hk.shape[0]
        h = self.hki.shape[-1] - 1
        F = wave.shape[-1]
        y = self._cached_pad("pqmf.inverse_conv.cache.wave", np.asarray(wave, self.dtype), h)
        if self.cfg.amplitude_modulation:
            a, amp = np.split(y, 2, axis=1)
            y = a * (self.dtype(1) / (self.dtype(1) + np.exp(-amp)))
        if noise is not None:
            y = y + self._cached_pad("pqmf.inverse_conv.cache.noise", np.asarray(noise, self.dtype), h)
        y = np.tanh(y)
        assert y.dtype == self.dtype and h % 2 == 0
        y = reverse_half(y)                            # h is even: the block's own parity
        y = conv_valid(y, np.asarray(self.hki, self.dtype), None, 1, 1, self.dtype) * self.dtype(m)
        assert y.shape[-1] == F
        y = y[:, ::-1, :]
        return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(y.shape[0], 1, F * m)

    # -------------------------------------------------------------- model
    def decoder_features(self, z):
        cfg = self.cfg
        pre = "decoder.net"
        i = 0
        x = self._conv(z, f"{pre}.{i}", cfg.kernel_size)
        i += 1
        for r, dils in zip(cfg.ratios[::-1], cfg.dilations[::-1]):
            x = self._act(x, f"{pre}.{i}")
            i += 1
            x = self._conv_transpose(x, f"{pre}.{i}", r)
            i += 1
            for d in dils:
                if cfg.adain:
                    x = self._adain(x, f"{pre}.{i}")
                    i += 1
                x = self._dilated_residual(x, f"{pre}.{i}", d)
                i += 1
        x = self._act(x, f"{pre}.{i}")
        i += 1
        return x, i

    def encode(self, x):
        """One block of audio (B, 1, k hop) -> latents (B, latent [+ speaker], k)."""
        return np.asarray(super().encode(np.asarray(x, self.dtype)), self.dtype)

    def decode(self, z, noise_u: Optional[np.ndarray] = None):
        """One block of latents (B, dec_in, k) -> audio (B, 1, k hop)."""
        cfg = self.cfg
        x, i = self.decoder_features(np.asarray(z, self.dtype))
        noise = None
        wave = "decoder.waveform_module" if cfg.noise is not None else f"decoder.net.{i}"
        if cfg.noise is not None:
            if noise_u is None:
                raise ValueError("noise synthesizer needs the uniform noise tensor")
            noise = np.asarray(self.noise_generator(x, np.asarray(noise_u, self.dtype)), self.dtype)
        return self._synthesis(self._conv(x, wave, 2 * cfg.kernel_size + 1), noise)

    def decoder(self, z, noise_u=None):
        raise NotImplementedError("the cached generator's epilogue lives in the PQMF inverse: use decode()")

    def encode_codes(self, x, return_gaps: bool = False):
        """One block of audio -> RVQ indices (B, n_q, k) (and the top-2 gaps (n_q, B k))."""
        return self.rvq_encode(self.encode(x), return_gaps)

    def decode_codes(self, idx, noise_u=None):
        return self.decode(self.cat_speaker(self.rvq_decode(np.asarray(idx))), noise_u)

    # -------------------------------------------------------------- delay
    def decode_delay(self) -> int:
        """Samples by which streamed decoding lags ``Oracle.decode``, from the
        operators' own lags: a cached conv r (stride 1), a Residual its unit's
        delay, a cached ConvTranspose1d its input's lag times r plus r//2, the
        PQMF inverse conv its r, all times n_band."""
        cfg = self.cfg
        d = get_padding(cfg.kernel_size, causal=cfg.causal)[1]
        for r, dils in zip(cfg.ratios[::-1], cfg.dilations[::-1]):
            d = d * r + r // 2
            d += sum(self.unit_delay(x) for x in dils)
        d += get_padding(2 * cfg.kernel_size + 1, causal=cfg.causal)[1]
        d += get_padding(self.hki.shape[-1], causal=cfg.causal)[1]
        return d * cfg.n_band


def stream(fn, x, sizes, axis=-1, extra=None):
    """Feed ``x`` to ``fn`` in consecutive pieces of ``sizes`` columns (``extra``:
    a function of (start, stop) giving further arguments) and concatenate."""
    out, pos = [], 0
    for n in sizes:
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(pos, pos + n)
        args = extra(pos, pos + n) if extra else ()
        out.append(fn(x[tuple(sl)], *args))
        pos += n
    return np.concatenate(out, -1)


# ---------------------------------------------------------------------- the block-length sweep's cases
def sweep_configs():
    """name -> (config, latent frames of its signal): the small models of the
    block-length sweep (tests/test_stream_ref_host.py, tests/test_gpu_stream_blocks.py).
    Capacity 8 throughout.  The hop-1024 ones keep dilations up to 9, so the
    deep layers' history (18) exceeds their block; in the short-hop pair one
    latent frame is 4 (hop 64) or 16 (hop 256) band frames, shorter than the
    PQMF histories, and t_in % 4 and the 16-byte history offsets change from
    layer to layer."""
    from rave_amd import config as rcfg
    return {
        "causal": (rcfg.causal(capacity=8), 24),
        "v2": (rcfg.v2(capacity=8), 24),
        "v3_noise_causal": (rcfg.v3_noise(causal=True, capacity=8), 24),
        "v3_noise": (rcfg.v3_noise(capacity=8), 24),
        "discrete": (rcfg.discrete(capacity=8), 24),
        "causal_hop64": (rcfg.causal(capacity=8, ratios=(2, 2), dilations=((1, 3), (1,))), 40),
        "v3_noise_causal_hop256": (rcfg.v3_noise(capacity=8, ratios=(2, 2, 2, 2), dilations=((1,),) * 4,
                                                 causal=True), 40),
    }


def sweep_signals(cfg, frames: int, batch: int = 2, seed: int = 0):
    """One signal per config, float32, every batch row different: audio (a sine
    plus 0.1 Gaussian noise), decoder input (Gaussian latents over the speaker
    channels) and, for a noise config, the uniform draws of the whole signal
    ((B, noise frames, n_band, target): a block's share is a slice of axis 1)."""
    from rave_amd.weights import init_speaker
    rng = np.random.default_rng(1000 + seed)
    n = np.arange(frames * cfg.hop)
    freqs = 220.0 * (1.0 + np.arange(batch))[:, None]
    x = 0.3 * np.sin(2 * np.pi * freqs * n[None] / 48000.0) + 0.1 * rng.standard_normal((batch, n.size))
    lat = rng.standard_normal((batch, cfg.latent_size, frames))
    spk = np.broadcast_to(init_speaker(cfg, seed).reshape(1, -1, 1), (batch, cfg.speaker_size, frames))
    out = {"x": x[:, None].astype(np.float32), "z": np.concatenate([lat, spk], 1).astype(np.float32), "u": None}
    if cfg.noise is not None:
        target = int(np.prod(cfg.noise.ratios))
        out["u"] = rng.uniform(0, 1, (batch, frames * cfg.hop // cfg.n_band // target, cfg.n_band,
                                      target)).astype(np.float32)
    return out


def noise_frames_per_latent(cfg) -> int:
    return cfg.hop // cfg.n_band // int(np.prod(cfg.noise.ratios))


def run_stream(ref: StreamRef, sig, sizes, what: str):
    """Stream ``sig`` through ``ref`` in blocks of ``sizes`` latent frames:
    what = "encode" (audio -> z), "decode" (z -> audio, with the blocks' noise
    draws), "encode_codes" (audio -> (indices, gaps (n_q, B, frames)))."""
    cfg = ref.cfg
    if what == "encode":
        return stream(ref.encode, sig["x"], [k * cfg.hop for k in sizes])
    if what == "encode_codes":
        idx, gaps, pos = [], [], 0
        for k in sizes:
            i, g = ref.encode_codes(sig["x"][..., pos * cfg.hop:(pos + k) * cfg.hop], return_gaps=True)
            idx.append(i)
            gaps.append(g.reshape(g.shape[0], i.shape[0], k))
            pos += k
        return np.concatenate(idx, -1), np.concatenate(gaps, -1)
    assert what == "decode"
    extra = None
    if cfg.noise is not None:
        per = noise_frames_per_latent(cfg)
        extra = lambda a, b: (sig["u"][:, a * per:b * per],)      # noqa: E731
    return stream(ref.decode, sig["z"], list(sizes), extra=extra)
