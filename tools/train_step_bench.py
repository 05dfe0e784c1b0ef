#!/usr/bin/env python3
"""Time one training step of the v2 decoder's module tree: forward, loss.backward() and
torch.optim.SGD.step() over every parameter, with the weights changing every step (the
section 19-21 timings all held them fixed).

The model is modules.GeneratorV2 at the v2 decoder's widths (latent 320 -> 1024 channels,
ratios (4, 4, 2, 2), LeakyReLU) without AdaIN and noise, built under
cc.use_transposed_grad(True), at --rows latent rows of --t frames; the loss is the mean square
of the output.  Two configurations: plain weights, and every conv under
torch.nn.utils.weight_norm (whose weight is a new tensor every forward).  The method is
tools/stft_loss_bench.py's: a warm-up, then windows of back-to-back steps between two HIP
events (the events sit on the GPU's timeline, so time the GPU spends waiting for the host
counts), the figure the median over the windows.  The step part uses only interfaces that
predate the device packer, so the same script times an older checkout from inside it:
compare runs of separate processes, alternating, on one GPU.

--pack adds, per distinct layer shape of the v2 encoder and decoder, the device packer's time
(rave_amd::pack_conv1d_device_) beside a device-to-device copy_ of the image's bytes (the same
bytes one way as the pack writes; the pack also reads the weight).

Prints one JSON line; --out saves it.  Needs the GPU.

Usage:  python tools/train_step_bench.py [--rows 16] [--t 64] [--iters 10] [--windows 7] [--out FILE]
        python tools/train_step_bench.py --pack [--out profiles/pack_device/pack.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def window_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def decoder(dev, weight_norm):
    from rave_amd import cc, config as rcfg, modules as M
    cfg = rcfg.v2()
    torch.manual_seed(0)
    cc.use_transposed_grad(True)
    try:
        gen = M.GeneratorV2(cfg.n_band, cfg.capacity, cfg.ratios, cfg.dec_in, cfg.kernel_size,
                            [list(d) for d in cfg.dilations], cfg.amplitude_modulation, "leaky", False, None).to(dev)
    finally:
        cc.use_transposed_grad(False)
    convs = [m for m in gen.modules() if isinstance(m, cc._PackedConv)]
    if weight_norm:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for m in convs:
                torch.nn.utils.weight_norm(m)
    return gen, cfg, len(convs)


def time_steps(a, dev, weight_norm):
    gen, cfg, n_convs = decoder(dev, weight_norm)
    z = torch.randn(a.rows, cfg.dec_in, a.t, device=dev)
    opt = torch.optim.SGD(gen.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = gen(z).square().mean()
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        first = step()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        ms.append(window_ms(step, a.iters))
        wall.append((time.perf_counter() - t0) * 1e3 / a.iters)
    last = float(step())
    missing = [n for n, p in gen.named_parameters() if p.grad is None]
    assert not missing and last == last, (missing, last)
    return {"step_ms": statistics.median(ms), "step_ms_min": min(ms), "step_ms_max": max(ms),
            "wall_ms": statistics.median(wall), "convs": n_convs,
            "parameters": sum(p.numel() for p in gen.parameters()), "loss_first": float(first), "loss_last": last}


def layer_shapes():
    """Distinct (c_in, c_out, kernel, stride, transposed, out_shift) of the v2 encoder's and
    decoder's convs, in module order (dilation does not change the image)."""
    from rave_amd import cc, config as rcfg, modules as M
    cfg = rcfg.v2()
    tree = M.RAVEModules(cfg)
    seen = []
    for m in tree.modules():
        if isinstance(m, cc._PackedConv):
            key = (m.c_in, m.c_out, m.kernel, m.stride, int(m.transposed), m.out_shift)
            if key not in seen:
                seen.append(key)
    return seen


def time_packs(a, dev):
    from rave_amd import cc  # noqa: F401
    rows = []
    for c_in, c_out, k, s, tr, shift in layer_shapes():
        n = int(torch.ops.rave_amd.conv1d_packed_size(c_in, c_out, k, s, 1, bool(tr)))
        w = torch.randn((c_in, c_out, k) if tr else (c_out, c_in, k), device=dev)
        dst, src = torch.empty(n, device=dev), torch.randn(n, device=dev)

        def pack():
            torch.ops.rave_amd.pack_conv1d_device_(w, dst, c_in, c_out, k, s, 1, bool(tr), shift)

        def copy():
            dst.copy_(src)

        for _ in range(a.warmup):
            pack(), copy()
        torch.cuda.synchronize()
        tp, tc = [], []
        for _ in range(a.windows):
            tp.append(window_ms(pack, a.pack_iters))
            tc.append(window_ms(copy, a.pack_iters))
        p, c = statistics.median(tp) * 1e3, statistics.median(tc) * 1e3
        rows.append({"c_in": c_in, "c_out": c_out, "kernel": k, "stride": s, "transposed": tr, "out_shift": shift,
                     "weight_floats": w.numel(), "image_floats": n, "pack_us": round(p, 3), "copy_us": round(c, 3),
                     "pack_over_copy": round(p / c, 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--t", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pack", action="store_true", help="time the device packer per layer shape instead")
    ap.add_argument("--pack-iters", type=int, default=200)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench needs the GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "tools/train_step_bench.py", "device": torch.cuda.get_device_name(0), "label": a.label,
           "windows": a.windows}
    from rave_amd import cc  # noqa: F401  (loads the op library)
    out["device_packer"] = hasattr(torch.ops.rave_amd, "pack_conv1d_device_")
    if a.pack:
        out.update({"layers": time_packs(a, dev), "iters": a.pack_iters,
                    "timing": "HIP events around back-to-back calls, pack and copy_ alternating, median of windows",
                    "copy": "Tensor.copy_ of the image's floats, device to device"})
    else:
        out.update({"plain": time_steps(a, dev, False), "weight_norm": time_steps(a, dev, True), "rows": a.rows,
                    "t": a.t, "iters": a.iters,
                    "step": "forward, mean-square loss, backward, SGD.step() over every parameter",
                    "timing": "HIP events around back-to-back steps, median of windows"})
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
