#!/usr/bin/env python3
"""Cost of per-row target speakers at the headline shape (v2, 16 x 65536,
f32_bf3 with the pinned launch choices of profiles/tuning/).

Three ways to run one step, alternating in one process:

* ``shared``   forward of the batch, one speaker for every row (what the model
               did before the speaker table existed);
* ``per_row``  the same forward with 16 different table rows -- the same plan,
               its speaker fill reading ``values[(row0 + b) * 256 + c]``;
* ``calls``    what a user had to do for 16 targets without the table: 16
               forwards at B = 1, each after ``set_speaker`` (device source).

Each timed window is a run of back-to-back steps between two HIP events (no
host synchronisation inside); the figure is the median over the windows.  One
round is an untimed settling window, then shared, per_row, per_row, shared,
calls (the window right after the B = 1 calls measures 8 % slow whichever
mode it runs).
Before anything is timed, rows of ``per_row`` are checked bitwise against
shared-mode forwards of the batch with that row's speaker (the same plan; the
B = 1 plans of ``calls`` pick other kernels, so they are not compared).  The
B = 1 plan is autotuned at build unless its choices are pinned.  Prints one
JSON line and saves it (default profiles/speakers/bench.json).  Needs the GPU;
there is no fallback.

Usage:  python tools/speakers_bench.py [--batch 16] [--t 65536] [--iters 20] [--windows 7]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--t", type=int, default=65536)
    ap.add_argument("--precision", default="f32_bf3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "speakers", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speakers_bench needs the GPU")
    from rave_amd import config as rcfg
    from rave_amd.model import RAVE
    from rave_amd.weights import init_params, init_speaker
    dev = torch.device("cuda:0")
    cfg = rcfg.v2()
    B, T = a.batch, a.t
    pinned = os.path.join(REPO, "profiles", "tuning", f"v2_{B}x{T}_{a.precision}.json")
    tuning = None
    if os.path.exists(pinned):
        with open(pinned) as fh:
            tuning = json.load(fh)
    m = RAVE(cfg, init_params(cfg, seed=0), init_speaker(cfg, seed=0), device=dev, precision=a.precision,
             tuning=tuning)
    x = (0.3 * torch.randn(B, 1, T, generator=torch.Generator().manual_seed(0))).to(dev)
    E = torch.from_numpy(np.stack([np.random.default_rng(100 + r).standard_normal(cfg.speaker_size)
                                   for r in range(B)]).astype(np.float32)).to(dev)
    x1 = [x[b:b + 1].contiguous() for b in range(B)]

    def shared():
        return m.forward(x)

    def per_row():
        return m.forward(x)

    def calls():
        out = None
        for b in range(B):
            m.set_speaker(E[b])
            out = m.forward(x1[b])
        return out

    # the per-row result against shared-mode runs of the same plan, before any timing
    m.set_speaker(E)
    y = per_row().clone()
    same = True
    for b in (0, B - 1):
        m.set_speaker(E[b])
        same = same and bool(torch.equal(shared()[b], y[b]))
    for _ in range(a.warmup):
        m.set_speaker(E[0]); shared()
        m.set_speaker(E); per_row()
        calls()
    torch.cuda.synchronize()
    t_s, t_p, t_c = [], [], []
    for _ in range(a.windows):
        # alternate the three; shared and per-row in ABBA order, so that whatever the
        # window before leaves behind (clocks, caches after the B = 1 calls) weighs on both
        window_ms(per_row, a.iters)           # untimed: the first window after the B = 1 calls runs 8 % slow
        for mode in ("s", "p", "p", "s"):
            m.set_speaker(E[0] if mode == "s" else E)
            (t_s if mode == "s" else t_p).append(window_ms(shared if mode == "s" else per_row, a.iters))
        t_c.append(window_ms(calls, max(1, a.iters // 4)))
    med = statistics.median
    res = {
        "tool": "tools/speakers_bench.py", "device": torch.cuda.get_device_name(0),
        "config": "v2", "precision": a.precision, "batch": B, "t": T,
        "tuning": os.path.relpath(pinned, REPO) if tuning else "autotuned at plan build",
        "iters": a.iters, "windows": a.windows, "timing": "HIP events around back-to-back steps, median of windows",
        "shared_ms": med(t_s), "shared_ms_min": min(t_s), "shared_ms_max": max(t_s),
        "per_row_ms": med(t_p), "per_row_ms_min": min(t_p), "per_row_ms_max": max(t_p),
        "calls_ms": med(t_c), "calls_ms_min": min(t_c), "calls_ms_max": max(t_c),
        "shared_windows_ms": [round(t, 4) for t in t_s], "per_row_windows_ms": [round(t, 4) for t in t_p],
        "per_row_over_shared": med(t_p) / med(t_s),
        "calls_over_per_row": med(t_c) / med(t_p),
        "per_row_rows_equal_shared_runs_bitwise": same,
    }
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
