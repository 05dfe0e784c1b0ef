"""Multi-scale STFT and the spectral audio distance on the native kernels.

Mirrors ``core.MultiScaleSTFT`` and ``core.AudioDistanceV1`` (rave/core.py:
278-353) as the reference binds them (rave/configs/v1.gin:21-28: scales 2048 /
1024 / 512 / 256 / 128, magnitude output; ``log_epsilon`` 1e-7, 1 for
discrete.gin:22) -- the metric ``RAVE.validation_step`` reports
(rave/model.py:636-686).

``AudioDistance`` is two launches that read only the audio (rave_audio_distance,
rave_amd/csrc/stft.hip): the spectrograms never reach memory.  ``MultiScaleSTFT``
writes them out, one launch per scale (rave_stft_mag).  The window / twiddle
tables and the workspace are built once and kept on the object; no call
allocates inside the native library or synchronises the host.  There is no CPU
path.

Both losses are differentiable with respect to the value signal
(rave_amd/csrc/stft_loss.hip): ``AudioDistance`` when ``y`` requires grad, and
``MultiResolutionSTFTLoss`` (rave/stft_loss.py:108-144, the criterion of
``RAVE.training_step``, rave/model.py:191-198), whose resolutions are general
(n_fft, hop, win) triples.  The backward is one native call that reads the
upstream gradients from device memory; the target is a constant.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple

import torch

from . import _native as N

DEFAULT_SCALES = (2048, 1024, 512, 256, 128)     # v1.gin:24


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _rows(x: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 CUDA tensor")
    if x.dim() != 3:
        raise ValueError(f"{name} must be (B, C, T), got {tuple(x.shape)}")
    return x.contiguous()


class _Tables:
    """Per-device cache of the packed window / twiddle tables."""

    def __init__(self, scales: Sequence[int]):
        self.host = {int(n): N.pack_stft_table(int(n)) for n in scales}
        self.dev: Dict[Tuple[torch.device, int], torch.Tensor] = {}

    def get(self, dev: torch.device, n: int) -> torch.Tensor:
        key = (dev, int(n))
        if key not in self.dev:
            self.dev[key] = torch.from_numpy(self.host[int(n)]).to(dev)
        return self.dev[key]


class MultiScaleSTFT:
    """``core.MultiScaleSTFT.forward``: x (B, C, T) -> one magnitude spectrogram
    per scale, each ((B C), n/2 + 1, 1 + T // (n/4)) float32 (torchaudio's
    Spectrogram: periodic Hann, hop n/4, centred with reflect padding)."""

    def __init__(self, scales: Sequence[int] = DEFAULT_SCALES, sample_rate: int = 0, magnitude: bool = True,
                 normalized: bool = False, num_mels=None):
        if not magnitude:
            raise NotImplementedError("MultiScaleSTFT: complex output (magnitude=False) is not implemented")
        if num_mels is not None:
            raise NotImplementedError("MultiScaleSTFT: mel scales are not implemented")
        if normalized:
            raise NotImplementedError("MultiScaleSTFT: normalized=True is not implemented")
        self.scales = tuple(int(n) for n in scales)
        self._tables = _Tables(self.scales)

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        x = _rows(x, "x")
        rows, T = x.shape[0] * x.shape[1], x.shape[2]
        out = []
        with torch.cuda.device(x.device):
            for n in self.scales:
                y = torch.empty(rows, n // 2 + 1, 1 + T // (n // 4), device=x.device)
                a = N.StftArgs(rows=rows, t_len=T, n=n, x=x.data_ptr(),
                               table=self._tables.get(x.device, n).data_ptr(), y=y.data_ptr())
                N.check(N.lib.rave_stft_mag(C.byref(a), _stream(x.device)), "stft_mag")
                out.append(y)
        return out

    __call__ = forward


class AudioDistance:
    """``core.AudioDistanceV1``: per scale ``mean((|X|-|Y|)^2) / mean(|X|^2) +
    mean|log(|X|+eps) - log(|Y|+eps)|``, summed over the scales.  ``x`` is the
    target: the relative term divides by its power, so the distance is not
    symmetric.  Results are bit-reproducible run to run (no atomics)."""

    def __init__(self, scales: Sequence[int] = DEFAULT_SCALES, log_epsilon: float = 1e-7):
        self.scales = tuple(int(n) for n in scales)
        self.log_epsilon = float(log_epsilon)
        if len(self.scales) > N.STFT_MAX_SCALES:
            raise NotImplementedError(f"at most {N.STFT_MAX_SCALES} scales per AudioDistance")
        self._tables = _Tables(self.scales)
        self._work: Dict[tuple, torch.Tensor] = {}       # (device, rows, T) -> workspace
        self._loss = None                                # the differentiable kernels, built on first use

    @classmethod
    def for_config(cls, cfg, scales: Sequence[int] = DEFAULT_SCALES) -> "AudioDistance":
        """The reference's binding for a config: ``log_epsilon`` 1 for the
        discrete config (discrete.gin:22), 1e-7 otherwise (v2.gin)."""
        return cls(scales, 1.0 if cfg.rvq is not None else 1e-7)

    def _args(self, x: torch.Tensor, y: torch.Tensor) -> N.DistanceArgs:
        rows, T = x.shape[0] * x.shape[1], x.shape[2]
        a = N.DistanceArgs(rows=rows, t_len=T, n_scales=len(self.scales), log_epsilon=self.log_epsilon)
        for i, n in enumerate(self.scales):
            a.scales[i] = n
            a.tables[i] = self._tables.get(x.device, n).data_ptr()
        key = (x.device, rows, T)
        if key not in self._work:
            size = int(N.lib.rave_audio_distance_workspace(C.byref(a)))
            if size < 0:
                raise ValueError("audio_distance: " + N.lib.rave_last_error().decode(errors="replace"))
            self._work[key] = torch.empty(size // 4, device=x.device)
        a.x, a.y = x.data_ptr(), y.data_ptr()
        a.workspace = self._work[key].data_ptr()
        return a

    def _run(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        x, y = _rows(x, "x"), _rows(y, "y")
        if x.shape != y.shape or x.device != y.device:
            raise ValueError(f"x and y must have one shape and device, got {tuple(x.shape)} and {tuple(y.shape)}")
        out = torch.empty(1 + 2 * len(self.scales), device=x.device)
        with torch.cuda.device(x.device):
            a = self._args(x, y)
            a.out = out.data_ptr()
            N.check(N.lib.rave_audio_distance(C.byref(a), _stream(x.device)), "audio_distance")
        return out

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``y`` may require grad: the distance then comes from the differentiable
        kernels (rave_stft_loss_forward / _backward) and carries a ``grad_fn``.
        Otherwise the path is rave_audio_distance, as before.  ``x`` is the target
        and a constant."""
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise ValueError("AudioDistance: the target is constant (x must not require grad)")
        if isinstance(y, torch.Tensor) and y.requires_grad and torch.is_grad_enabled():
            x, y = _rows(x, "x"), _rows(y, "y")
            if x.shape != y.shape or x.device != y.device:
                raise ValueError(f"x and y must have one shape and device, got {tuple(x.shape)} and {tuple(y.shape)}")
            if self._loss is None:
                self._loss = _LossKernels(N.STFT_LOSS_V1, [(n, n // 4, n) for n in self.scales], self.log_epsilon)
            out = _StftLossFn.apply(y.reshape(-1, y.shape[-1]), x.reshape(-1, x.shape[-1]), self._loss)
            return {"spectral_distance": out[0]}
        return {"spectral_distance": self._run(x, y)[0]}

    __call__ = forward

    def terms(self, x: torch.Tensor, y: torch.Tensor) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """Per scale the (relative L2, log L1) pair, 0-dim device tensors."""
        out = self._run(x, y)
        return [(out[1 + 2 * i], out[2 + 2 * i]) for i in range(len(self.scales))]


class _LossKernels:
    """Tables, workspace and argument block of rave_stft_loss_forward /
    rave_stft_loss_backward for one loss kind and list of (n_fft, hop, win)."""

    def __init__(self, kind: int, resolutions: Sequence[Tuple[int, int, int]], log_epsilon: float = 0.0):
        self.kind = int(kind)
        self.resolutions = tuple((int(n), int(h), int(w)) for n, h, w in resolutions)
        self.log_epsilon = float(log_epsilon)
        if not 1 <= len(self.resolutions) <= N.STFT_MAX_SCALES:
            raise ValueError(f"1 to {N.STFT_MAX_SCALES} resolutions per loss, got {len(self.resolutions)}")
        self._host = {(n, w): N.pack_stft_loss_table(n, w) for n, _, w in self.resolutions}
        self._tables: Dict[tuple, torch.Tensor] = {}     # (device, n_fft, win) -> table
        self._work: Dict[tuple, torch.Tensor] = {}       # (device, rows, T) -> workspace

    def args(self, value: torch.Tensor, target: torch.Tensor) -> N.StftLossArgs:
        rows, T = value.shape
        dev = value.device
        a = N.StftLossArgs(rows=rows, t_len=T, n_res=len(self.resolutions), kind=self.kind,
                           log_epsilon=self.log_epsilon)
        for i, (n, h, w) in enumerate(self.resolutions):
            a.n_fft[i], a.hop[i], a.win[i] = n, h, w
            if (dev, n, w) not in self._tables:
                self._tables[(dev, n, w)] = torch.from_numpy(self._host[(n, w)]).to(dev)
            a.tables[i] = self._tables[(dev, n, w)].data_ptr()
        key = (dev, rows, T)
        if key not in self._work:
            size = int(N.lib.rave_stft_loss_workspace(C.byref(a)))
            if size < 0:
                raise ValueError("stft_loss: " + N.lib.rave_last_error().decode(errors="replace"))
            self._work[key] = torch.empty(size // 4, device=dev)
        a.value, a.target = value.data_ptr(), target.data_ptr()
        a.workspace = self._work[key].data_ptr()
        return a


class _StftLossFn(torch.autograd.Function):
    """value, target (rows, T) -> the native ``out`` vector (2 + 2 n_res floats).
    Only out[0] (and out[1] for the multi-resolution loss) are differentiable
    outputs of the library; the wrappers hand out nothing else with a grad_fn."""

    @staticmethod
    def forward(ctx, value: torch.Tensor, target: torch.Tensor, kern: _LossKernels):
        n_res = len(kern.resolutions)
        out = torch.empty(2 + 2 * n_res, device=value.device)
        saved = torch.empty(4 * n_res, device=value.device)
        with torch.cuda.device(value.device):
            a = kern.args(value, target)
            a.out, a.saved = out.data_ptr(), saved.data_ptr()
            N.check(N.lib.rave_stft_loss_forward(C.byref(a), _stream(value.device)), "stft_loss_forward")
        ctx.kern = kern
        ctx.save_for_backward(value, target, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad: torch.Tensor):
        value, target, saved = ctx.saved_tensors
        kern = ctx.kern
        grad = grad.to(torch.float32).contiguous()       # [0] (V1) or [0:2] (multi-resolution) reach the kernel
        out = torch.empty_like(value)
        with torch.cuda.device(value.device):
            a = kern.args(value, target)
            a.saved, a.grad_out, a.grad_value = saved.data_ptr(), grad.data_ptr(), out.data_ptr()
            N.check(N.lib.rave_stft_loss_backward(C.byref(a), _stream(value.device)), "stft_loss_backward")
        return out, None, None


class MultiResolutionSTFTLoss:
    """``stft_loss.MultiResolutionSTFTLoss`` (rave/stft_loss.py:108-144):
    ``(pred, target) -> (sc_loss, mag_loss)``, spectral convergence and the
    log-magnitude L1, each the mean over the (n_fft, hop, win) resolutions.
    ``pred`` and ``target`` are (B, T) float32 CUDA tensors; when ``pred``
    requires grad both results carry a ``grad_fn`` whose backward is one native
    call.  The target is a constant.  Bit-reproducible, forward and backward."""

    def __init__(self, resolutions: Sequence[Tuple[int, int, int]]):
        self._kern = _LossKernels(N.STFT_LOSS_MULTIRES, resolutions)
        self.resolutions = self._kern.resolutions

    @classmethod
    def for_sample_rate(cls, sr: int = 44100) -> "MultiResolutionSTFTLoss":
        """The three resolutions RAVE.__init__ builds (rave/model.py:191-196):
        hops of 5 / 10 / 2 ms, windows of 25 / 50 / 10 ms, n_fft the next power
        of two above the window."""
        import math
        res = []
        for hop_ms, win_ms in ((5, 25), (10, 50), (2, 10)):
            hop = int(0.001 * hop_ms * sr)
            win = int(0.001 * win_ms * sr)
            res.append((int(math.pow(2, int(math.log2(win)) + 1)), hop, win))
        return cls(res)

    def _run(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if isinstance(target, torch.Tensor) and target.requires_grad and torch.is_grad_enabled():
            raise ValueError("MultiResolutionSTFTLoss: the target is constant (it must not require grad)")
        for name, v in (("pred", pred), ("target", target)):
            if not isinstance(v, torch.Tensor) or v.device.type != "cuda" or v.dtype != torch.float32:
                raise ValueError(f"{name} must be a float32 CUDA tensor")
            if v.dim() != 2:
                raise ValueError(f"{name} must be (B, T), got {tuple(v.shape)}")
        if pred.shape != target.shape or pred.device != target.device:
            raise ValueError(f"pred and target must have one shape and device, got {tuple(pred.shape)} and "
                             f"{tuple(target.shape)}")
        return _StftLossFn.apply(pred.contiguous(), target.contiguous(), self._kern)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        out = self._run(pred, target)
        return out[0], out[1]

    __call__ = forward

    def terms(self, pred: torch.Tensor, target: torch.Tensor) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """Per resolution the (spectral convergence, log-magnitude) pair, 0-dim
        device tensors without a grad_fn."""
        out = self._run(pred, target).detach()
        return [(out[2 + 2 * i], out[3 + 2 * i]) for i in range(len(self.resolutions))]
