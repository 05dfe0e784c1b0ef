#!/usr/bin/env python3
"""Time the differentiable noise filter stage and a training step of a v3_noise decoder.

(a) noise_synth forward + backward at the v3_noise workload's shape -- amp (16, 80, 512), u
    (16, 512, 16, 8): torch.ops.rave_amd.noise_synth under autograd (two launches) against the
    torch composition with autograd on the same GPU, the torch.fft restatement of
    tests/noise_grad_ref.noise_synth_torch.  Windows of the two variants alternate inside one
    run, each window a separate measurement; the figure that decides is the fused pair's
    slowest window against the composition's fastest.
(b) one forward + backward + SGD.step() of modules.GeneratorV2 at the v2 decoder's widths with
    Snake, AdaIN and the noise module (the v3_noise decoder) in train() mode on a (16, 320, 64)
    latent with a fixed draw, beside tools/train_step_bench.py's tree without them (LeakyReLU,
    no AdaIN, no noise), re-measured in the same run, windows alternating.  For scale only.

The method is tools/train_step_bench.py's: a warm-up, then windows of back-to-back calls
between two HIP events, median / min / max over the windows.

Prints one JSON line; --out saves it.  Needs the GPU.

Usage:  python tools/noise_grad_bench.py [--out profiles/noise_grad/bench.json]
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

from tools.train_step_bench import decoder as v2_decoder, window_ms  # noqa: E402


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows_ms": ms}


def interleaved(fns, warmup, windows, iters):
    """Windows of the variants in turn (a, b, a, b, ...): {name: [ms per call, one per window]}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, iters))
    return out


def time_noise(a, dev):
    from rave_amd import cc  # noqa: F401  (loads the op library)
    from tests.noise_grad_ref import noise_synth_torch
    B, n_band, nb, F, T = 16, 16, 5, 512, 8
    g = torch.Generator(device="cpu").manual_seed(0)
    amp = (torch.randn(B, n_band * nb, F, generator=g) * 3 + 4).to(dev).requires_grad_(True)
    u = torch.rand(B, F, n_band, T, generator=g).to(dev)
    gy = torch.randn(B, n_band, F * T, generator=g).to(dev)

    def fused():
        amp.grad = None
        torch.ops.rave_amd.noise_synth(amp, u, n_band, nb).backward(gy)

    def composed():
        amp.grad = None
        noise_synth_torch(amp, u, n_band, nb, T).backward(gy)

    fused()
    g_fused = amp.grad.clone()
    composed()
    top = float(amp.grad.abs().max())
    diff = float((g_fused - amp.grad).abs().max())
    assert diff <= 1e-4 * top, (diff, top)                 # the same gradient (each against fp32 torch.fft)
    ms = interleaved({"fused": fused, "torch": composed}, a.warmup, a.windows, a.noise_iters)
    return {"shape": {"amp": [B, n_band * nb, F], "u": [B, F, n_band, T]}, "iters": a.noise_iters,
            "fused": stats(ms["fused"]), "torch": stats(ms["torch"]),
            "grad_max": top, "grad_max_abs_diff": diff,
            "torch_fastest_over_fused_slowest": min(ms["torch"]) / max(ms["fused"]),
            "torch_median_over_fused_median": statistics.median(ms["torch"]) / statistics.median(ms["fused"]),
            "fused_slowest_below_torch_fastest": max(ms["fused"]) < min(ms["torch"])}


def v3_noise_decoder(dev):
    from rave_amd import cc, config as rcfg, modules as M
    cfg = rcfg.v3_noise()
    torch.manual_seed(0)
    cc.use_transposed_grad(True)
    try:
        gen = M.GeneratorV2(cfg.n_band, cfg.capacity, cfg.ratios, cfg.dec_in, cfg.kernel_size,
                            [list(d) for d in cfg.dilations], cfg.amplitude_modulation, cfg.activation, cfg.adain,
                            cfg.noise).to(dev)
    finally:
        cc.use_transposed_grad(False)
    return gen.train(), cfg


def time_steps(a, dev):
    gen3, cfg = v3_noise_decoder(dev)
    gen2, _, _ = v2_decoder(dev, False)
    z = torch.randn(a.rows, cfg.dec_in, a.t, device=dev)
    target = 1
    for r in cfg.noise.ratios:
        target *= r
    hop = 1
    for r in cfg.ratios:
        hop *= r
    u = torch.rand(a.rows, a.t * hop // target, cfg.n_band, target, device=dev)
    opt3 = torch.optim.SGD(gen3.parameters(), lr=1e-4)
    opt2 = torch.optim.SGD(gen2.parameters(), lr=1e-4)
    last = {}

    def step3():
        opt3.zero_grad(set_to_none=True)
        loss = gen3(z, u).square().mean()
        loss.backward()
        opt3.step()
        last["v3_noise"] = loss.detach()

    def step2():
        opt2.zero_grad(set_to_none=True)
        loss = gen2(z).square().mean()
        loss.backward()
        opt2.step()
        last["v2"] = loss.detach()

    ms = interleaved({"v3_noise": step3, "v2": step2}, a.warmup, a.windows, a.iters)
    for name, gen in (("v3_noise", gen3), ("v2", gen2)):
        missing = [n for n, p in gen.named_parameters() if p.grad is None]
        assert not missing and float(last[name]) == float(last[name]), (name, missing)
    return {"rows": a.rows, "t": a.t, "iters": a.iters,
            "v3_noise": dict(stats(ms["v3_noise"]), parameters=sum(p.numel() for p in gen3.parameters())),
            "v2": dict(stats(ms["v2"]), parameters=sum(p.numel() for p in gen2.parameters())),
            "step": "forward, mean-square loss, backward, SGD.step() over every parameter; train() mode"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--t", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise-iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_grad_bench needs the GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "tools/noise_grad_bench.py", "device": torch.cuda.get_device_name(0), "windows": a.windows,
           "timing": "HIP events around back-to-back calls, the variants' windows alternating in one run",
           "noise_synth_fwd_bwd": time_noise(a, dev), "train_step": time_steps(a, dev)}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
