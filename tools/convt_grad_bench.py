#!/usr/bin/env python3
"""Time forward + backward of one differentiable cc.ConvTranspose1d per v2 decoder
upsampler against the composition a user writes without it: F.leaky_relu,
F.conv_transpose1d and torch autograd, on the same GPU and the same tensors.

The four upsamplers of the v2 decoder (1024 -> 512 r2, 512 -> 256 r2, 256 -> 128 r4,
128 -> 64 r4) at 16 rows and their own input lengths, LeakyReLU(0.2) in front;
the gradients of x, weight and bias are asked of both.  The method is
tools/stft_loss_bench.py's: the two alternate in one process, each timed window
is a run of back-to-back calls between two HIP events, the figure is the median
over the windows, and the x gradients are compared before anything is timed.
Prints one JSON line and saves it (default profiles/convt_grad/bench.json).
Needs the GPU.

Usage:  python tools/convt_grad_bench.py [--rows 16] [--iters 30] [--windows 7]
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

# (c_in, c_out, r, t_in)
SHAPES = [(1024, 512, 2, 64), (512, 256, 2, 128), (256, 128, 4, 256), (128, 64, 4, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "convt_grad", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convt_grad_bench needs the GPU")
    from rave_amd import cc
    dev = torch.device("cuda:0")
    out = {}
    for c_in, c_out, r, T in SHAPES:
        torch.manual_seed(c_in + r)
        cc.use_transposed_grad(True)
        try:
            up = cc.ConvTranspose1d(c_in, c_out, 2 * r, stride=r, padding=r // 2, bias=True, activation=cc.ACT_LEAKY).to(dev)
        finally:
            cc.use_transposed_grad(False)
        x = torch.randn(a.rows, c_in, T, device=dev, requires_grad=True)
        params = [x, up.weight, up.bias]
        gy = torch.randn_like(up(x).detach())

        def fused():
            return torch.autograd.grad(up(x), params, gy)[0]

        def composition():
            y = F.conv_transpose1d(F.leaky_relu(x, 0.2), up.weight, up.bias, stride=r, padding=r // 2)
            return torch.autograd.grad(y, params, gy)[0]

        out.update(compare(f"r{r}_{c_in}to{c_out}_T{T}", fused, composition, a))
    out.update({
        "tool": "tools/convt_grad_bench.py", "device": torch.cuda.get_device_name(0), "rows": a.rows,
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
