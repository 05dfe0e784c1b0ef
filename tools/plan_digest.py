#!/usr/bin/env python3
"""What the model engine builds, as data: per model case the op lists of its one-shot plans, the
tuner's choices, its stream plans' launch counts and delay, and digests of what those plans
compute.  A change to the engine's host side that must not alter a plan (csrc/engine.cpp's op
builders) runs this once on the parent's library and once on its own
(RAVE_AMD_LIB_VARIANT selects the library, as in tools/conv_grad_bits.py) and compares the two
files with --compare.

Cases: (a) the small v2 config in exact fp32, (b) the same in split-f16 alone, (c) the small
v3_noise / AdaIN config, (d) the small causal config (cached transposed convs, res_delay),
(e) the small discrete config (the RVQ plans), all at batch 2, one-shot length 4 hops, streams of
1 and of 4 hops: each has one arithmetic and no autotune, so no choice depends on a timing.
(f) bench config 3 (causal v2, batch 1, 2048-sample blocks) in f32_bf3 on its committed pins,
profiles/tuning/c3_f32_bf3.json, at the shape those pins were recorded at.  Two more reach the
fused path edges, which (a) to (f) barely do: (g) full-width v2 in split-f16 at batch 2 (head and
tail both fused; built without fused units, whose cooperative forms are chosen by timing even in a
single arithmetic) and (h) the bench's headline forward, 16 x 65536 in f32_bf3 on
profiles/tuning/v2_16x65536_f32_bf3.json.

--shape writes the part of cases (a), (b), (d) and (g) that tests/test_gpu_plan_shape.py asserts
(op kinds, precisions, labels, launches of a 1-hop stream) to tests/golden/plan_shape.json.

Usage:  [RAVE_AMD_LIB_VARIANT=name] python tools/plan_digest.py [--out FILE] [--cases a,b,...]
        python tools/plan_digest.py --shape
        python tools/plan_digest.py --compare FILE FILE
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

OUT_DIR = os.path.join(REPO, "profiles", "engine_fold")
SHAPE_FILE = os.path.join(REPO, "tests", "golden", "plan_shape.json")
LIBRARY = os.environ.get("RAVE_AMD_LIB_VARIANT") or "head"
TUNING = os.path.join("profiles", "tuning")


def cases():
    """name -> (config, precision, pinned tuning file or None, batch, one-shot hops or None, stream hops,
    fuse_units)"""
    from rave_amd import config as rcfg
    return {
        "a_v2_small_f32": (rcfg.v2(capacity=8), "f32", None, 2, 4, (1, 4), True),
        "b_v2_small_split16": (rcfg.v2(capacity=8), "split16", None, 2, 4, (1, 4), True),
        "c_v3_noise_small_f32": (rcfg.v3_noise(capacity=8), "f32", None, 2, 4, (1, 4), True),
        "d_causal_small_f32": (rcfg.causal(capacity=8), "f32", None, 2, 4, (1, 4), True),
        "e_discrete_small_f32": (rcfg.discrete(capacity=8), "f32", None, 2, 4, (1, 4), True),
        "f_c3_f32_bf3_pinned": (rcfg.causal(), "f32_bf3", os.path.join(TUNING, "c3_f32_bf3.json"), 1, None, (2,),
                                True),
        "g_v2_split16": (rcfg.v2(), "split16", None, 2, 4, (1,), False),
        "h_v2_16x65536_f32_bf3_pinned": (rcfg.v2(), "f32_bf3", os.path.join(TUNING, "v2_16x65536_f32_bf3.json"),
                                         16, 64, (), True),
    }


SHAPE_CASES = ("a_v2_small_f32", "b_v2_small_split16", "d_causal_small_f32", "g_v2_split16")


def build(name):
    import torch
    from rave_amd.model import RAVE
    from rave_amd.weights import init_params, init_speaker
    cfg, precision, pin, B, hops, stream_hops, fuse = cases()[name]
    tuning = None
    if pin:
        with open(os.path.join(REPO, pin)) as fh:
            tuning = json.load(fh)
    m = RAVE(cfg, init_params(cfg, 0), init_speaker(cfg, 0), device=torch.device("cuda:0"), precision=precision,
             tuning=tuning, fuse_units=fuse)
    return m, tuning


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def plan_ops(m, B, hops):
    """which -> op list; encode plans take samples, decode plans latent frames"""
    kinds = (0, 1) + ((2, 3) if m.cfg.rvq is not None else ())
    return {str(w): m.ops(w, B, hops * m.cfg.hop if w in (0, 2) else hops) for w in kinds}


def stream_of(m, B, hops, blocks=0, seed=0):
    """Launch counts and delay of one stream (captured graphs); with `blocks`, a digest of that many
    consecutive blocks of seeded input through encode and decode"""
    import torch
    from rave_amd.streaming import StreamingRAVE
    cfg = m.cfg
    s = StreamingRAVE(m, batch=B, block=hops * cfg.hop)
    out = {"launches": {"encode": s.launches("encode"), "decode": s.launches("decode")}, "delay": s.decode_delay}
    if blocks:
        gen = torch.Generator().manual_seed(seed)
        got = []
        for _ in range(blocks):
            x = (0.2 * torch.randn(B, 1, hops * cfg.hop, generator=gen)).to(m.device)
            if cfg.rvq is not None:
                idx = s.encode_codes(x)
                got += [idx, s.decode_codes(idx)]
                continue
            z = torch.randn(B, cfg.dec_in, hops, generator=gen).to(m.device)
            u = torch.rand(m.noise_shape(B, hops), generator=gen).to(m.device) if cfg.noise is not None else None
            got += [s.encode(x), s.decode(z, u)]
        torch.cuda.synchronize()
        out["sha256"] = sha(*got)
    return out


def digest(name):
    import torch
    cfg, precision, pin, B, hops, stream_hops, fuse = cases()[name]
    m, tuning = build(name)
    out = {"precision": precision, "batch": B, "pinned": pin}
    if hops:
        out["plans"] = plan_ops(m, B, hops)
        gen = torch.Generator().manual_seed(1)
        x = (0.2 * torch.randn(B, 1, hops * cfg.hop, generator=gen)).to(m.device)
        if cfg.rvq is not None:
            idx = m.encode_codes(x)
            y = [idx, m.decode_codes(idx)]
        else:
            u = torch.rand(m.noise_shape(B, hops), generator=gen).to(m.device) if cfg.noise is not None else None
            y = [m.forward(x, u)]
        torch.cuda.synchronize()
        out["forward_sha256"] = sha(*y)
    out["streams"] = {str(h): stream_of(m, B, h, blocks=3) for h in stream_hops}
    m.check()
    have = m.tuning()
    out["tuning"] = have
    if tuning is not None:         # a key the plans wanted and did not find pinned was timed and appended
        out["timed_not_pinned"] = sorted({k for k, _, _ in have} - {k for k, _, _ in tuning})
    return out


def shape(name):
    """What tests/test_gpu_plan_shape.py asserts of one case"""
    cfg, precision, pin, B, hops, stream_hops, fuse = cases()[name]
    m, _ = build(name)
    ops = {w: [[o["kind"], o["precision"], o["label"]] for o in lst] for w, lst in plan_ops(m, B, hops).items()}
    return {"encode": ops["0"], "decode": ops["1"], "stream_1hop": stream_of(m, B, 1)}


def compare(path_a, path_b):
    """Equal in every field, but for the millisecond column of the tuning text where nothing pins it"""
    with open(path_a) as fh:
        a = json.load(fh)["cases"]
    with open(path_b) as fh:
        b = json.load(fh)["cases"]
    bad = []
    if sorted(a) != sorted(b):
        bad.append(f"cases differ: {sorted(a)} / {sorted(b)}")
    for name in sorted(set(a) & set(b)):
        ca, cb = dict(a[name]), dict(b[name])
        ta, tb = ca.pop("tuning"), cb.pop("tuning")
        if not ca["pinned"] or ca.get("timed_not_pinned"):
            ta, tb = [t[:2] for t in ta], [t[:2] for t in tb]
        if ta != tb:
            bad.append(f"{name}: tuning differs")
        bad += [f"{name}: {k} differs" for k in sorted(set(ca) | set(cb)) if ca.get(k) != cb.get(k)]
    print("\n".join(bad) if bad else f"equal: {len(a)} cases")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--cases", help="comma-separated case names or their first letters (default: all)")
    ap.add_argument("--shape", action="store_true", help=f"write {os.path.relpath(SHAPE_FILE, REPO)}")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("plan_digest needs the GPU")
    want = a.cases.split(",") if a.cases else None
    names = [n for n in (SHAPE_CASES if a.shape else cases()) if want is None or n in want or n[0] in want]
    if a.shape:
        out, path = {name: shape(name) for name in names}, a.out or SHAPE_FILE
    else:
        from rave_amd import _native
        out = {"tool": "tools/plan_digest.py", "library": LIBRARY, "library_file": os.path.basename(_native.LIB_PATH),
               "device": torch.cuda.get_device_name(0), "cases": {}}
        for name in names:
            out["cases"][name] = digest(name)
            print(name, hashlib.sha256(json.dumps(out["cases"][name], sort_keys=True).encode()).hexdigest()[:16],
                  flush=True)
        path = a.out or os.path.join(OUT_DIR, f"plan_{LIBRARY}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
