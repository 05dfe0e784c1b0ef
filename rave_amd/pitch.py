"""YIN pitch tracking and the f0 one-hot conditioning on the native kernels.

Mirrors the YIN half of ``rave/pitch_utils.py``: ``estimate`` and its helpers
(:15-86), ``get_pitch`` (:90-96), and ``one_hot`` / ``get_f0_norm`` in the
default ``'abs'`` mode (:98-127) -- the 257 channels ``ScriptedRAVE.myforward``
concatenates after the latent and the speaker embedding (scripts/export.py:
358-397).  The neural FCPE estimator and the ``'rel'`` norm mode are not
implemented.

``Yin`` is one launch per call (rave_yin), ``F0OneHot`` one launch that can write
straight into the tail channels of a decoder-input tensor (rave_f0_onehot), and
``PitchConditioner`` goes from audio to those channels in one launch
(rave_pitch_onehot, rave_amd/csrc/pitch.hip).  No call allocates inside the
native library or synchronises the host.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _native as N

F0_LO, F0_HI = 40.0, 400.0                        # pitch_utils.py:115


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _audio(x: torch.Tensor) -> Tuple[int, int, int]:
    """(rows, T, row stride) of x (..., T).  A layout whose rows do not lie at
    one stride is reported as stride 0, which the native check refuses."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32:
        raise ValueError("x must be a float32 CUDA tensor")
    if x.dim() < 1 or x.dim() > 3 or x.numel() == 0:
        raise ValueError(f"x must be (T), (rows, T) or (B, C, T), got {tuple(x.shape)}")
    T = x.shape[-1]
    rows = x.numel() // T
    if T > 1 and x.stride(-1) != 1:
        return rows, T, 0
    sr = T
    dims = [(n, s) for n, s in zip(x.shape[:-1], x.stride()[:-1]) if n > 1]
    if dims:
        sr = dims[-1][1]
        if len(dims) == 2 and dims[0][1] != dims[1][0] * dims[1][1]:
            sr = 0
    return rows, T, sr


class Yin:
    """``pitch_utils.estimate`` bound as ``get_pitch`` binds it (70-400 Hz,
    threshold 0.1): x (..., T) -> f0 (..., frames) float32 in Hz, 0 where the
    frame is not periodic."""

    def __init__(self, sample_rate: int = 44100, pitch_min: float = 70.0, pitch_max: float = 400.0,
                 threshold: float = 0.1):
        self.sample_rate = int(sample_rate)
        self.pitch_min, self.pitch_max = float(pitch_min), float(pitch_max)
        self.threshold = float(threshold)

    def args(self, rows: int, T: int, frame_stride: float, x_sr: Optional[int] = None) -> N.YinArgs:
        return N.YinArgs(rows=rows, t_len=T, sample_rate=self.sample_rate, pitch_min=self.pitch_min,
                         pitch_max=self.pitch_max, frame_stride=float(frame_stride), threshold=self.threshold,
                         x_sr=T if x_sr is None else x_sr)

    def shape(self, T: int, frame_stride: float) -> dict:
        """tau_min, tau_max, frame_length, stride (samples) and frames for a
        signal of T samples, by the library's own host arithmetic."""
        out = (N.i32 * 5)()
        N.check(N.lib.rave_yin_shape(C.byref(self.args(1, T, frame_stride)), out), "yin_shape")
        return dict(zip(("tau_min", "tau_max", "frame_length", "stride", "frames"), (int(v) for v in out)))

    def estimate(self, x: torch.Tensor, frame_stride: float = 0.01, return_cmdf: bool = False):
        """``frame_stride`` in seconds, as the reference takes it.  With
        ``return_cmdf`` also the sliced cmdf (..., frames, tau_max - 1 - tau_min)."""
        rows, T, x_sr = _audio(x)
        a = self.args(rows, T, frame_stride, x_sr)
        g = self.shape(T, frame_stride)
        f0 = torch.empty(x.shape[:-1] + (g["frames"],), device=x.device)
        a.x, a.f0 = x.data_ptr(), f0.data_ptr()
        cmdf = None
        if return_cmdf:
            cmdf = torch.empty(x.shape[:-1] + (g["frames"], g["tau_max"] - 1 - g["tau_min"]), device=x.device)
            a.cmdf = cmdf.data_ptr()
        with torch.cuda.device(x.device):
            N.check(N.lib.rave_yin(C.byref(a), _stream(x.device)), "yin")
        return (f0, cmdf) if return_cmdf else f0

    def block_stride(self, T: int, block_size: int) -> float:
        """``get_pitch``'s frame stride in seconds: T / block_size frames spread
        over the signal (pitch_utils.py:91-94)."""
        desired = T / block_size
        if desired == 1:
            raise ValueError("get_pitch: a single block leaves the stride undefined")
        frame_length = 2 * int(self.sample_rate / self.pitch_min)
        return (T - frame_length) / (desired - 1) / self.sample_rate

    def get_pitch(self, x: torch.Tensor, block_size: int) -> torch.Tensor:
        return self.estimate(x, self.block_stride(x.shape[-1], block_size))


class F0OneHot:
    """``get_f0_norm`` in ``'abs'`` mode followed by ``one_hot``: f0 (B, frames)
    -> (B, num_bins + 1, frames), channels first as the decoder reads them.
    Class ``num_bins`` collects f0 = 0 and everything outside the range."""

    def __init__(self, num_bins: int = 256):
        self.num_bins = int(num_bins)
        # the reference's arithmetic as written: log(400 - log 40)
        self.log_lo = math.log(F0_LO)
        self.log_span = math.log(F0_HI - math.log(F0_LO))

    @property
    def channels(self) -> int:
        return self.num_bins + 1

    def args(self, batch: int, frames: int, out: torch.Tensor, channel_offset: int) -> N.F0OneHotArgs:
        if out.device.type != "cuda" or out.dtype != torch.float32 or out.dim() != 3:
            raise ValueError("out must be a float32 CUDA tensor (B, C, frames)")
        if out.shape[0] != batch or out.shape[2] != frames or out.stride(2) != 1 and frames > 1:
            raise ValueError(f"out {tuple(out.shape)} does not take a ({batch}, {frames}) contour at time stride 1")
        if channel_offset < 0 or channel_offset + self.channels > out.shape[1]:
            raise ValueError(f"channels [{channel_offset}, {channel_offset + self.channels}) do not fit "
                             f"out's {out.shape[1]}")
        return N.F0OneHotArgs(batch=batch, frames=frames, bins=self.num_bins, log_lo=self.log_lo,
                              log_span=self.log_span, y_sb=out.stride(0), y_sc=out.stride(1),
                              y=out.data_ptr() + 4 * channel_offset * out.stride(1))

    def forward(self, f0: torch.Tensor, out: Optional[torch.Tensor] = None, channel_offset: int = 0) -> torch.Tensor:
        if not isinstance(f0, torch.Tensor) or f0.device.type != "cuda" or f0.dtype != torch.float32 or f0.dim() != 2:
            raise ValueError("f0 must be a float32 CUDA tensor (B, frames)")
        f0 = f0.contiguous()
        if out is None:
            out = torch.empty(f0.shape[0], self.channels, f0.shape[1], device=f0.device)
        a = self.args(f0.shape[0], f0.shape[1], out, channel_offset)
        a.f0 = f0.data_ptr()
        with torch.cuda.device(f0.device):
            N.check(N.lib.rave_f0_onehot(C.byref(a), _stream(f0.device)), "f0_onehot")
        return out

    __call__ = forward


class PitchConditioner:
    """Latent ``z`` (B, C, Fz) and the audio ``x`` (B, 1, T) it was encoded from
    -> (B, C + 257, Fz): ``z`` copied once, the f0 one-hot of ``get_pitch(x,
    cfg.hop)`` written behind it by the fused op."""

    def __init__(self, cfg, sample_rate: int = 44100, num_bins: int = 256):
        self.block_size = int(cfg.hop)
        self.yin = Yin(sample_rate)
        self.onehot = F0OneHot(num_bins)

    def pitch_onehot(self, x: torch.Tensor, out: torch.Tensor, channel_offset: int = 0,
                     f0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fused launch: the one-hot of x's contour into ``out``'s channels
        from ``channel_offset``; ``f0`` (B, frames), if given, receives the contour."""
        rows, T, x_sr = _audio(x)
        stride = self.yin.block_stride(T, self.block_size)
        a = self.yin.args(rows, T, stride, x_sr)
        frames = self.yin.shape(T, stride)["frames"]
        h = self.onehot.args(rows, frames, out, channel_offset)
        a.x = x.data_ptr()
        if f0 is not None:
            if f0.device != x.device or f0.dtype != torch.float32 or tuple(f0.shape) != (rows, frames) \
                    or not f0.is_contiguous():
                raise ValueError(f"f0 must be a contiguous float32 ({rows}, {frames}) tensor on x's device")
            a.f0 = f0.data_ptr()
        with torch.cuda.device(x.device):
            N.check(N.lib.rave_pitch_onehot(C.byref(a), C.byref(h), _stream(x.device)), "pitch_onehot")
        return out

    def forward(self, z: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        if z.dim() != 3 or z.device.type != "cuda" or z.dtype != torch.float32:
            raise ValueError("z must be a float32 CUDA tensor (B, C, Fz)")
        if x.dim() != 3 or x.shape[0] != z.shape[0] or x.shape[1] != 1:
            raise ValueError(f"x must be (B, 1, T) with z's batch, got {tuple(x.shape)} for z {tuple(z.shape)}")
        B, Cz, Fz = z.shape
        out = torch.empty(B, Cz + self.onehot.channels, Fz, device=z.device)
        out[:, :Cz].copy_(z)
        return self.pitch_onehot(x, out, Cz)

    __call__ = forward
