#!/usr/bin/env python3
"""Time the differentiable PQMF synthesis against the composition a user writes
without it: the head in elementwise torch ops (x_w sigmoid(x_a) + noise -> tanh),
reverse_half, F.conv1d with the 33-tap synthesis filter, the band flip and
interleave (rave/pqmf.py:275-284), torch.stft for the loss, and torch autograd
for the gradient.

Two measurements on the same seeded multiband tensor (rows x 32 x T / 16,
default 16 rows of 65536 samples): (a) CachedPQMF.inverse (mode 1, noise)
forward + backward from a fixed cotangent; (b) inverse +
MultiResolutionSTFTLoss.for_sample_rate(44100) forward + backward down to the
multiband gradient.  The method is tools/stft_loss_bench.py's: fused and
composition alternate in one process, each timed window is a run of
back-to-back calls between two HIP events (no host synchronisation inside),
and the figure is the median over the windows.  The gradients of the two are
compared before anything is timed.  Prints one JSON line and saves it (default
profiles/pqmf_grad/bench.json).  Needs the GPU; there is no fallback.

Usage:  python tools/pqmf_grad_bench.py [--rows 16] [--t 65536] [--iters 50] [--windows 7]
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

from tools.stft_loss_bench import compare, mr_composition  # noqa: E402


def inverse_composition(x, noise, hki, mask, pad):
    """(B, 32, F), (B, 16, F) -> (B, 16 F): the head and CachedPQMF.inverse in torch ops."""
    v = torch.tanh(x[:, :16] * torch.sigmoid(x[:, 16:]) + noise) * mask
    y = F.conv1d(F.pad(v, pad), hki) * 16
    return y.flip(1).permute(0, 2, 1).reshape(x.shape[0], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--t", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pqmf_grad", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pqmf_grad_bench needs the GPU")
    from rave_amd import cc
    from rave_amd.distance import MultiResolutionSTFTLoss
    dev = torch.device("cuda:0")
    frames = a.t // 16
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(a.rows, 32, frames, generator=g)
    x[:, :16] *= 0.5
    noise = 0.01 * torch.randn(a.rows, 16, frames, generator=g)
    t = torch.arange(a.t, dtype=torch.float64)
    target = (0.3 * torch.sin(2 * torch.pi * 440 * t / 48000)[None]
              + 0.1 * torch.randn(a.rows, a.t, generator=g, dtype=torch.float64)).float().to(dev)
    gy = torch.randn(a.rows, a.t, generator=g).to(dev)
    x, noise = x.to(dev).requires_grad_(True), noise.to(dev)

    pq = cc.CachedPQMF().to(dev)
    hki = pq.hki.clone()
    mask = torch.ones(16, frames, device=dev)
    mask[1::2, ::2] = -1                                   # reverse_half
    pad = (pq.pad_s, hki.shape[-1] - 1 - pq.pad_s)
    loss = MultiResolutionSTFTLoss.for_sample_rate(44100)
    res = loss.resolutions
    hann = {w: torch.hann_window(w, device=dev) for _, _, w in res}

    out = {}
    out.update(compare("inverse_forward_backward",
                       lambda: torch.autograd.grad(pq.inverse(x, 1, noise)[:, 0], x, gy)[0],
                       lambda: torch.autograd.grad(inverse_composition(x, noise, hki, mask, pad), x, gy)[0], a))
    out.update(compare("inverse_loss_forward_backward",
                       lambda: torch.autograd.grad(sum(loss(pq.inverse(x, 1, noise)[:, 0], target)), x)[0],
                       lambda: torch.autograd.grad(sum(mr_composition(inverse_composition(x, noise, hki, mask, pad),
                                                                      target, res, hann)), x)[0], a))
    out.update({
        "tool": "tools/pqmf_grad_bench.py", "device": torch.cuda.get_device_name(0),
        "rows": a.rows, "t": a.t, "frames": frames, "mode": 1, "noise": True,
        "resolutions": [list(r) for r in res], "iters": a.iters, "windows": a.windows,
        "timing": "HIP events around back-to-back calls, fused and composition alternating, median of windows",
        "rel_diff": "relative L2 difference of the fused multiband gradient from the composition's",
        "fused_launches": {"inverse_forward_backward": 2,
                           "note": "one synthesis and one adjoint kernel; the loss adds its own (DESIGN.md 17)"},
    })
    line = json.dumps(out, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
