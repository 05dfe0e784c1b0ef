#!/usr/bin/env python3
"""Time the differentiable spectral losses against the composition a user writes
without them: torch.stft on the device per resolution and input, the elementwise
ops of stft_loss.MultiResolutionSTFTLoss (rave/stft_loss.py:12-144) or
core.AudioDistanceV1 (rave/core.py:339-353), and torch autograd for the
gradient.

Two losses -- the fork's three resolutions at 44.1 kHz and AudioDistanceV1's
default scales -- each forward only and forward + backward, on the same seeded
broadband inputs (rows x T, default 16 x 65536).  The method is
tools/distance_bench.py's: fused and composition alternate in one process, each
timed window is a run of back-to-back calls between two HIP events (no host
synchronisation inside), and the figure is the median over the windows.  Values
and gradients of the two are compared before anything is timed.  Prints one
JSON line and saves it (default profiles/stft_loss/bench.json).  Needs the GPU;
there is no fallback.

Usage:  python tools/stft_loss_bench.py [--rows 16] [--t 65536] [--iters 50] [--windows 7]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

SCALES = (2048, 1024, 512, 256, 128)


def mr_composition(pred, target, resolutions, windows):
    sc = mag = 0.
    for n_fft, hop, win in resolutions:
        def m(x):
            z = torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=win, window=windows[win], return_complex=True)
            return torch.sqrt(torch.clamp(z.real ** 2 + z.imag ** 2, min=1e-7))
        p, t = m(pred), m(target)
        sc = sc + torch.norm(t - p, p="fro") / torch.norm(t, p="fro")
        mag = mag + torch.nn.functional.l1_loss(torch.log(t), torch.log(p))
    return sc / len(resolutions), mag / len(resolutions)


def v1_composition(x, y, windows, eps):
    d = 0.
    for n in SCALES:
        kw = dict(hop_length=n // 4, win_length=n, window=windows[n], center=True, pad_mode="reflect",
                  return_complex=True)
        sx, sy = torch.stft(x, n, **kw).abs(), torch.stft(y, n, **kw).abs()
        diff = sx - sy
        d = d + (diff * diff).mean() / (sx * sx).mean() + (torch.log(sx + eps) - torch.log(sy + eps)).abs().mean()
    return d


def window_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(name, fused, comp, a):
    """Warm up, check fused against the composition, then alternate timed windows."""
    for _ in range(a.warmup):
        rf, rc = fused(), comp()
    torch.cuda.synchronize()
    diff = float((rf.double() - rc.double()).norm() / rc.double().norm())
    t_f, t_c = [], []
    for _ in range(a.windows):
        t_f.append(window_ms(fused, a.iters))
        t_c.append(window_ms(comp, a.iters))
    mf, mc = statistics.median(t_f), statistics.median(t_c)
    return {f"{name}_fused_ms": mf, f"{name}_fused_ms_min": min(t_f), f"{name}_fused_ms_max": max(t_f),
            f"{name}_composition_ms": mc, f"{name}_composition_ms_min": min(t_c), f"{name}_composition_ms_max": max(t_c),
            f"{name}_ratio": mc / mf, f"{name}_rel_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--t", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log-epsilon", type=float, default=1e-7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stft_loss", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stft_loss_bench needs the GPU")
    from rave_amd.distance import AudioDistance, MultiResolutionSTFTLoss
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    t = torch.arange(a.t, dtype=torch.float64)
    target = (0.3 * torch.sin(2 * torch.pi * 440 * t / 48000)[None]
              + 0.1 * torch.randn(a.rows, a.t, generator=g, dtype=torch.float64))
    pred = target + 0.03 * torch.randn(a.rows, a.t, generator=g, dtype=torch.float64)
    target, pred = target.float().to(dev), pred.float().to(dev)
    pred_g = pred.clone().requires_grad_(True)

    loss = MultiResolutionSTFTLoss.for_sample_rate(44100)
    res = loss.resolutions
    hann = {w: torch.hann_window(w, device=dev) for _, _, w in res}
    hann.update({n: torch.hann_window(n, device=dev) for n in SCALES})
    dist = AudioDistance(SCALES, a.log_epsilon)
    x3, y3, y3g = target[:, None], pred[:, None], pred_g[:, None]

    def both(pair):
        return torch.stack(list(pair))
    out = {}
    out.update(compare("multires_forward", lambda: both(loss(pred, target)),
                       lambda: both(mr_composition(pred, target, res, hann)), a))
    out.update(compare("multires_forward_backward",
                       lambda: torch.autograd.grad(sum(loss(pred_g, target)), pred_g)[0],
                       lambda: torch.autograd.grad(sum(mr_composition(pred_g, target, res, hann)), pred_g)[0], a))
    out.update(compare("v1_forward", lambda: dist(x3, y3)["spectral_distance"],
                       lambda: v1_composition(target, pred, hann, a.log_epsilon), a))
    out.update(compare("v1_forward_backward",
                       lambda: torch.autograd.grad(dist(x3, y3g)["spectral_distance"], pred_g)[0],
                       lambda: torch.autograd.grad(v1_composition(target, pred_g, hann, a.log_epsilon), pred_g)[0], a))
    out.update({
        "tool": "tools/stft_loss_bench.py", "device": torch.cuda.get_device_name(0),
        "rows": a.rows, "t": a.t, "resolutions": [list(r) for r in res], "v1_scales": list(SCALES),
        "log_epsilon": a.log_epsilon, "iters": a.iters, "windows": a.windows,
        "timing": "HIP events around back-to-back calls, fused and composition alternating, median of windows",
        "rel_diff": "relative L2 difference of the fused result (values or gradient) from the composition's",
        "multires_workspace_bytes": sum(w.numel() * 4 for w in loss._kern._work.values()),
        "v1_workspace_bytes": sum(w.numel() * 4 for w in dist._loss._work.values()),
        "audio_bytes": 4 * a.rows * a.t,
    })
    line = json.dumps(out, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
