#!/usr/bin/env python3
"""Time the fused audio -> f0 one-hot call against the composition a user would
write without it: rave/pitch_utils.py's get_pitch and get_f0_norm ('abs') as
fp32 torch ops on the device -- unfold, rfft / irfft at 4096, two cumsums, the
search, bucketize and the eye gather.

Both run on the same seeded harmonic glides (tests/pitch_ref.py; rows x T,
default 16 x 65536, one f0 per 1024-sample latent frame, 70-400 Hz at 44.1 kHz), alternating in one
process; each timed window is a run of back-to-back calls between two HIP events
(no host synchronisation inside), and the figure is the median over the
windows.  The two results are compared before anything is timed.  Prints one
JSON line and saves it (default profiles/pitch/bench.json).  Needs the GPU;
there is no fallback.

Usage:  python tools/pitch_bench.py [--rows 16] [--t 65536] [--iters 200] [--windows 7]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

SR, PMIN, PMAX, THRESHOLD, BINS = 44100, 70.0, 400.0, 0.1, 256


def composition(x, block, eye, edges):
    """get_pitch + get_f0_norm as the reference writes them, on x's device."""
    T = x.shape[-1]
    tau_min, tau_max = int(SR / PMAX), int(SR / PMIN)
    L = 2 * tau_max
    stride = int((T - L) / (T / block - 1) / SR * SR)
    frames = x.unfold(-1, L, stride)
    size = 1 << (math.ceil(math.log(L) / math.log(2)) + 1)
    spec = torch.fft.rfft(frames, size, dim=-1)
    r = torch.fft.irfft(spec * spec.conj())[..., :tau_max]
    energy = torch.nn.functional.pad((frames * frames).cumsum(-1), [1, 0])
    d = energy[..., -1:] + (energy.flip(-1)[..., :tau_max] - energy[..., :tau_max]) - 2 * r
    cmdf = (d[..., 1:] * torch.arange(1, tau_max, device=x.device)
            / torch.clamp(d[..., 1:].cumsum(-1), min=1e-5))[..., tau_min:]
    start = (cmdf < THRESHOLD).int().argmax(-1, keepdim=True)
    start = torch.where(start > 0, start, tau_max)
    j = torch.arange(cmdf.shape[-1], device=x.device)
    stops_falling = torch.nn.functional.pad(cmdf.diff() >= 0.0, [0, 1], value=1.0)
    tau = ((j >= start) & stops_falling).int().argmax(-1)
    f0 = torch.where(tau > 0, SR / (tau + tau_min + 1).float(), torch.zeros((), device=x.device))
    f0 = torch.where(f0 == 0, torch.full_like(f0, float("nan")), f0)
    v = (torch.log(f0) - math.log(40.0)) / math.log(400.0 - math.log(40.0)) + 0.5
    idx = torch.bucketize(v, edges, right=True) - 1
    return eye[idx.reshape(-1)].reshape(idx.shape[0], idx.shape[1], BINS + 1).permute(0, 2, 1)


def window_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--t", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pitch", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench needs the GPU")
    from rave_amd import config as rcfg
    from rave_amd.pitch import PitchConditioner
    from tests.pitch_ref import glides
    dev = torch.device("cuda:0")
    x = torch.from_numpy(glides((a.rows, 1, a.t), SR, 80.0, 380.0, seed=0)).to(dev)
    cond = PitchConditioner(rcfg.v2(), SR, BINS)
    a.block = cond.block_size                                   # one f0 per latent frame (1024 samples)
    frames = cond.yin.shape(a.t, cond.yin.block_stride(a.t, a.block))["frames"]
    out = torch.empty(a.rows, BINS + 1, frames, device=dev)
    eye = torch.eye(BINS + 1, device=dev)
    edges = torch.linspace(0, 1, BINS + 1, device=dev)
    rows2 = x.reshape(a.rows, a.t)
    fused = lambda: cond.pitch_onehot(x, out)                    # noqa: E731
    comp = lambda: composition(rows2, a.block, eye, edges)      # noqa: E731
    for _ in range(a.warmup):
        hf, hc = fused(), comp()
    torch.cuda.synchronize()
    differ = int((hf.argmax(1) != hc.argmax(1)).sum())
    voiced = int((hf.argmax(1) != BINS).sum())
    t_f, t_c = [], []
    for _ in range(a.windows):                                  # alternate the two
        t_f.append(window_ms(fused, a.iters))
        t_c.append(window_ms(comp, a.iters))
    res = {
        "tool": "tools/pitch_bench.py", "device": torch.cuda.get_device_name(0),
        "rows": a.rows, "t": a.t, "block": a.block, "frames_per_row": frames, "bins": BINS,
        "iters": a.iters, "windows": a.windows, "timing": "HIP events around back-to-back calls, median of windows",
        "fused_ms": statistics.median(t_f), "fused_ms_min": min(t_f), "fused_ms_max": max(t_f),
        "composition_ms": statistics.median(t_c), "composition_ms_min": min(t_c), "composition_ms_max": max(t_c),
        "speedup": statistics.median(t_c) / statistics.median(t_f),
        "fused_launches": 1, "frames": a.rows * frames, "frames_voiced": voiced,
        "frames_where_fp32_composition_differs": differ,
        "fused_multiply_adds": a.rows * frames * sum(1260 - tau for tau in range(630)),
    }
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
