#!/usr/bin/env python3
"""Time forward + backward of one cc.Conv1d per layer family against the
composition a user writes without it: the activation in elementwise torch ops,
F.pad, F.conv1d and torch autograd, on the same GPU and the same tensors.

One conv per family (kernel, stride, dilation) at 16 x C x T shapes of the v2
decoder / encoder widths, LeakyReLU(0.2) in front; the gradients of x, weight
and bias are asked of both.  The method is tools/stft_loss_bench.py's: the two
alternate in one process, each timed window is a run of back-to-back calls
between two HIP events, the figure is the median over the windows, and the x
gradients are compared before anything is timed.  Prints one JSON line and
saves it (default profiles/conv_grad/bench.json).  Needs the GPU.

Usage:  python tools/conv_grad_bench.py [--rows 16] [--iters 30] [--windows 7]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tools.stft_loss_bench import compare  # noqa: E402

# (kernel, stride, dilation, c_in, c_out, T)
SHAPES = [(1, 1, 1, 128, 128, 2048), (3, 1, 1, 128, 128, 2048), (3, 1, 3, 128, 128, 2048), (3, 1, 9, 128, 128, 2048),
          (3, 1, 16, 256, 256, 1024), (7, 1, 1, 64, 16, 4096), (4, 2, 1, 128, 256, 2048), (8, 4, 1, 64, 128, 4096)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_grad", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_grad_bench needs the GPU")
    from rave_amd import cc
    dev = torch.device("cuda:0")
    out = {}
    for k, s, d, c_in, c_out, T in SHAPES:
        torch.manual_seed(k * 100 + d)
        pad = cc.get_padding(k, s, d) if s == 1 else ((k - s) // 2, (k - s) - (k - s) // 2)
        conv = cc.Conv1d(c_in, c_out, k, stride=s, padding=pad, dilation=d, activation=cc.ACT_LEAKY).to(dev)
        x = torch.randn(a.rows, c_in, T, device=dev, requires_grad=True)
        params = [x, conv.weight, conv.bias]
        gy = torch.randn_like(conv(x).detach())

        def fused():
            return torch.autograd.grad(conv(x), params, gy)[0]

        def composition():
            y = F.conv1d(F.pad(F.leaky_relu(x, 0.2), pad), conv.weight, conv.bias, stride=s, dilation=d)
            return torch.autograd.grad(y, params, gy)[0]

        out.update(compare(f"k{k}_s{s}_d{d}_{c_in}to{c_out}_T{T}", fused, composition, a))
    out.update({
        "tool": "tools/conv_grad_bench.py", "device": torch.cuda.get_device_name(0), "rows": a.rows,
        "shapes": [list(sh) for sh in SHAPES], "activation": "leaky 0.2", "iters": a.iters, "windows": a.windows,
        "timing": "HIP events around back-to-back calls, fused and composition alternating, median of windows",
        "rel_diff": "relative L2 difference of the fused x gradient from the composition's",
        "fused_launches": "forward 1 (+ split-K reduce), data gradient 1, weight gradient 1 + slab reduce",
    })
    line = json.dumps(out, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
