#!/usr/bin/env python3
"""Pin the conv and transposed-conv gradient kernels (csrc/conv_grad.hip) bit for bit, and time
them, through the C boundary alone (ctypes, as the tests' harness calls it), so that
RAVE_AMD_LIB_VARIANT selects the library under test: a refactor of those kernels runs this once
on the parent's library and once on its own and compares the two files.

Default mode: over a fixed list of small cases (built by the two GPU test files' seeded `_case`)
one JSON of the sha256 of the raw bytes of gx, gweight, gbias and galpha and the workspace's
float counts.  The list: every family (k1, the k3 dilations, k7, k4 s2, k8 s4, transposed r2 and
r4) x every activation x the paddings that apply x t in {1, 33, 65, 257} x four channel pairs on
and off the 16 / 32 / 64 tiles x B in {1, 3}; the test files' split-K cases; each output absent
in turn and bias only with a NULL x; one zero cotangent per family.  The saved file stays small:
per group of cases (a family at one padding, or one kind of extra case) one digest per output
over the group's cases in list order, each case's bytes behind its name, and the list of
workspace counts.  Two libraries agree on every case if and only if they agree on every line;
--per-case adds every case's own digests to the saved file, to find the case behind a line that
differs (such a file is for reading, not for committing).

--time: per shape of tools/conv_grad_bench.py and tools/convt_grad_bench.py (at --rows), the
median over windows of the HIP-event time around back-to-back data + weight calls
(tools/stft_loss_bench.py's method).  The output file is written anew unless --append is given,
with which alternating processes of two libraries fill one file.  Needs the GPU.

Usage:  [RAVE_AMD_LIB_VARIANT=name] python tools/conv_grad_bits.py [--per-case] [--out FILE]
        [RAVE_AMD_LIB_VARIANT=name] python tools/conv_grad_bits.py --time [--append] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import conv_grad_harness as H, conv_grad_ref as G  # noqa: E402
from tests import test_gpu_conv_grad as TC, test_gpu_convt_grad as TT  # noqa: E402
from tools.conv_grad_bench import SHAPES as CONV_SHAPES  # noqa: E402
from tools.convt_grad_bench import SHAPES as CONVT_SHAPES  # noqa: E402
from tools.stft_loss_bench import window_ms  # noqa: E402

OUT_DIR = os.path.join(REPO, "profiles", "conv_grad_refactor")
LIBRARY = os.environ.get("RAVE_AMD_LIB_VARIANT") or "head"
ACTS = [G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE]
TS = [1, 33, 65, 257]
PAIRS = [(16, 16), (40, 16), (136, 16), (16, 136)]
BS = [1, 3]
STRIDES = TT.G.STRIDES
ALL = ("gx", "gw", "gb", "ga")


def cases():
    """(group, name, which test file's _bwd, case, keyword arguments of _bwd)"""
    def fam_name(fam):
        return "k%ds%dd%d" % fam
    for fam in G.FAMILIES:
        pads = ["centred", "causal", "none"] + (["tail"] if fam[1] > 1 else [])
        for pad, act, t, (ci, co), B in itertools.product(pads, ACTS, TS, PAIRS, BS):
            c = TC._case(fam, pad, act, B, ci, co, t, seed=t)
            yield f"conv {fam_name(fam)} {pad}", f"act{act} B{B} {ci}to{co} t{t}", TC, c, {}
    for r in STRIDES:
        for act, t, (ci, co), B in itertools.product(ACTS, TS, PAIRS, BS):
            yield f"convt r{r}", f"act{act} B{B} {ci}to{co} t{t}", TT, TT._case(r, act, B, ci, co, t, seed=t), {}
    for fam in [(1, 1, 1), (3, 1, 1), (7, 1, 1), (4, 2, 1), (8, 4, 1)]:                  # one per weight-kernel instance
        yield "conv split-K", fam_name(fam), TC, TC._case(fam, "centred", G.ACT_LEAKY, 3, 16, 16, 700, seed=11), {}
    for r in STRIDES:
        yield "convt split-K", f"r{r}", TT, TT._case(r, G.ACT_LEAKY, 3, 16, 16, 700, seed=11), {}
    dropped = [(f"conv {fam_name(fam)}", TC, TC._case(fam, "causal", G.ACT_SNAKE, 3, 40, 64, 257, seed=31))
               for fam in [(3, 1, 9), (4, 2, 1)]]
    dropped += [(f"convt r{r}", TT, TT._case(r, G.ACT_SNAKE, 3, 40, 64, 257, seed=31)) for r in STRIDES]
    for name, mod, c in dropped:
        for drop in ALL:
            yield f"{name} outputs dropped", f"without {drop}", mod, c, dict(want=tuple(k for k in ALL if k != drop))
        yield f"{name} outputs dropped", "bias only, NULL x", mod, c, dict(want=("gb",), null_x=True)
    for fam in G.FAMILIES:
        c = TC._case(fam, "centred", G.ACT_SNAKE, 3, 40, 16, 65, seed=41)
        yield "conv zero cotangent", fam_name(fam), TC, dict(c, gy=np.zeros_like(c["gy"])), {}
    for r in STRIDES:
        c = TT._case(r, G.ACT_SNAKE, 3, 40, 16, 65, seed=41)
        yield "convt zero cotangent", f"r{r}", TT, dict(c, gy=np.zeros_like(c["gy"])), {}


def bits(per_case):
    groups, cases_, n = {}, {}, 0
    for group, name, mod, c, kw in cases():
        out, nws = mod._bwd(c, **kw)
        g = groups.setdefault(group, {"hash": {k: hashlib.sha256() for k in ALL}, "workspace_floats": []})
        raw = {k: v.contiguous().cpu().numpy().tobytes() for k, v in out.items()}
        for k in ALL:                                           # an absent output leaves its name alone
            g["hash"][k].update(name.encode() + raw.get(k, b""))
        g["workspace_floats"].append(nws)
        if per_case:
            cases_[f"{group} {name}"] = {k: hashlib.sha256(v).hexdigest() for k, v in raw.items()}
        n += 1
    for g in groups.values():
        g.update({k: h.hexdigest() for k, h in g.pop("hash").items()})
    return {"tool": "tools/conv_grad_bits.py", "library": LIBRARY, "library_file": os.path.basename(H.native().LIB_PATH),
            "device": torch.cuda.get_device_name(0), "cases": n, "groups": groups, **({"per_case": cases_} if per_case else {}),
            "digest": "per group and output, sha256 over the cases in list order of (case name, raw bytes of the output)"}


def timed_calls(prefix, a, wshape):
    """Contiguous device tensors behind the struct `a`; returns the data + weight call and what it keeps alive."""
    N = H.native()
    dev = H.DEV
    x = torch.randn(a.batch, a.c_in, a.t_in, device=dev)
    gy = torch.randn(a.batch, a.c_out, a.t_out, device=dev)
    w = torch.randn(wshape, device=dev) / (a.c_in * a.kernel) ** 0.5
    gx, gw, gb = torch.empty_like(x), torch.empty_like(w), torch.empty(a.c_out, device=dev)
    a.x, a.x_sb, a.x_sc = x.data_ptr(), x.stride(0), x.stride(1)
    a.gy, a.gy_sb, a.gy_sc = gy.data_ptr(), gy.stride(0), gy.stride(1)
    a.gx, a.gx_sb, a.gx_sc = gx.data_ptr(), gx.stride(0), gx.stride(1)
    a.weight, a.gweight, a.gbias = w.data_ptr(), gw.data_ptr(), gb.data_ptr()
    data, weight = getattr(N.lib, prefix + "_data"), getattr(N.lib, prefix + "_weight")
    nws = getattr(N.lib, prefix + "_workspace")(C.byref(a))
    N.check(min(nws, 0))
    ws = torch.empty(max(nws, 1), device=dev)
    a.workspace = ws.data_ptr()
    st = H.stream()

    def call():
        N.check(data(C.byref(a), st))
        N.check(weight(C.byref(a), st))
    return call, (x, gy, w, gx, gw, gb, ws)


def time_shapes(a):
    torch.manual_seed(0)
    todo = []
    for k, s, d, c_in, c_out, T in CONV_SHAPES:
        span = (k - 1) * d + 1
        pl, pr = ((span - 1) // 2, span // 2) if s == 1 else ((k - s) // 2, (k - s) - (k - s) // 2)
        c = dict(c_in=c_in, c_out=c_out, k=k, s=s, d=d, pl=pl, pr=pr, act=G.ACT_LEAKY, slope=0.2, B=a.rows, t_in=T,
                 t_out=(T + pl + pr - span) // s + 1)
        todo.append((f"k{k}_s{s}_d{d}_{c_in}to{c_out}_T{T}", "rave_conv1d_backward", TC._args(c), (c_out, c_in, k)))
    for c_in, c_out, r, T in CONVT_SHAPES:
        c = dict(c_in=c_in, c_out=c_out, r=r, act=G.ACT_LEAKY, slope=0.2, B=a.rows, t_in=T, t_out=T * r)
        todo.append((f"r{r}_{c_in}to{c_out}_T{T}", "rave_conv_transpose1d_backward", TT._args(c), (c_in, c_out, 2 * r)))
    shapes = {}
    for name, prefix, args, wshape in todo:
        call, keep = timed_calls(prefix, args, wshape)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = [window_ms(call, a.iters) for _ in range(a.windows)]
        shapes[name] = {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    return {"library": LIBRARY, "library_file": os.path.basename(H.native().LIB_PATH), "shapes": shapes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--append", action="store_true", help="--time: add this run to the runs the output file holds")
    ap.add_argument("--per-case", action="store_true", help="also save every case's own digests")
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_grad_bits needs the GPU")
    out_path = a.out or os.path.join(OUT_DIR, "time.json" if a.time else f"bits_{LIBRARY}.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if a.time:
        out = {"tool": "tools/conv_grad_bits.py --time", "device": torch.cuda.get_device_name(0), "rows": a.rows,
               "iters": a.iters, "windows": a.windows, "activation": "leaky 0.2",
               "timing": "HIP events around back-to-back data + weight calls, median of windows; one process per run",
               "runs": []}
        if a.append and os.path.exists(out_path):
            with open(out_path) as fh:
                out = json.load(fh)
        run = time_shapes(a)
        out["runs"].append(run)
        print(json.dumps(run, sort_keys=True))
    else:
        out = bits(a.per_case)
        print(json.dumps({"library": LIBRARY, "cases": out["cases"], "groups": len(out["groups"]),
                          "all": hashlib.sha256(json.dumps(out["groups"], sort_keys=True).encode()).hexdigest()}))
    with open(out_path, "w") as fh:                             # one line per group or run
        rows = out.pop("runs" if a.time else "groups")
        head = json.dumps(out, sort_keys=True)[:-1]
        if a.time:
            fh.write(head + ', "runs": [\n' + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]}\n")
        else:
            body = ",\n".join(f"{json.dumps(k)}: {json.dumps(rows[k], sort_keys=True)}" for k in rows)
            fh.write(head + ', "groups": {\n' + body + "\n}}\n")


if __name__ == "__main__":
    main()
