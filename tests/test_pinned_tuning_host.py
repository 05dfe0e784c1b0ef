"""Drift guard for the committed launch pins (profiles/tuning/*.json), on the
host: every key of every file must be one that the workload it pins can ask
for, so a stale pin is caught before a GPU run (there a key the plan wanted and
did not find is re-timed, which tests/test_gpu_configs_pinned.py and
tests/test_gpu_headline.py catch by counting).

Only the Python graph builder and the JSON files are used.  Key formats and
values restate rave_amd/csrc/engine.cpp:

* ``conv|<node>|<stream form>|B|t_in[|noring]`` -> precision * 65536 + config
  (Model::conv_launch; config 0 = heuristic, else a rave_conv1d_args.config
  word <= 1024).  A stream plan's conv reads ``need - sd + T`` columns
  (conv_stream: need = l + r + sd history columns, 1 for the cached
  ConvTranspose, whose key alone has stream form 1); ``noring`` marks a choice
  made without the 16-byte-row kernels;
* ``unit|<k3 node>|B|T`` -> precision | coop << 8 (Model::unit_pick; coop 0..2);
* ``fuse|<k3 node>|B|T``, ``stack|<k3 node>|B|T`` -> 0 / 1;
* ``pqa|B|T|t_in``, ``pqs|B|F|x_len|pad`` -> precision (Model::pqmf_prec);
* ``head|<precision>|B|T``, ``tail|<precision>|B|F`` -> 0 / 1.

The arithmetics a mode may choose are the ``precs`` of rave_model_create:
auto {f32, split16}; f32_tuned {f32, f32_ring}; f32_bf3 {f32, f32_ring, bf16x3}."""
import glob
import json
import os

import pytest

from rave_amd import config as rcfg
from rave_amd.graph import build_graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING = os.path.join(REPO, "profiles", "tuning")

F32, SPLIT16, F32_RING, BF16X3 = 0, 1, 4, 5          # include/rave_amd.h RAVE_PREC_*
MODES = {"auto": {F32, SPLIT16}, "f32_tuned": {F32, F32_RING}, "f32_bf3": {F32, F32_RING, BF16X3}}

# what bench.py runs on each pinned file: the config, the batch, and either the
# stream block (C3) or the one-shot length in samples; ``parts``: the graph
# sections whose plans are built (C5 decodes only)
WORKLOADS = {
    "c3": dict(cfg=rcfg.causal, B=1, block=2048, parts=("encoder", "decoder", "noise")),
    "c4": dict(cfg=rcfg.discrete, B=8, T=65536, parts=("encoder", "decoder", "noise")),
    "c5": dict(cfg=rcfg.v3_noise, B=16, T=64 * rcfg.v3_noise().hop, parts=("decoder", "noise")),
    "v2_16x65536": dict(cfg=rcfg.v2, B=16, T=65536, parts=("encoder", "decoder", "noise")),
}
FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(TUNING, "*.json")))


def _split_name(fname):
    stem = fname[:-len(".json")]
    for mode in sorted(MODES, key=len, reverse=True):
        if stem.endswith("_" + mode):
            return stem[:-len(mode) - 1], mode
    raise AssertionError(f"{fname}: no precision mode in the file name")


def _nodes(w):
    """{node name: (node, T of its input, is a fused unit's k3, is a unit member)}
    from the graph's strides, for the graph sections the workload builds."""
    cfg = w["cfg"]()
    g = build_graph(cfg)
    T = w.get("block", w.get("T"))
    t = {"enc_in": T // cfg.n_band, "dec_in": T // cfg.hop}
    out = {}
    for part in ("encoder", "decoder", "noise"):
        nodes = getattr(g, part)
        for i, n in enumerate(nodes):
            ts = t[n.src]
            t[n.dst] = ts * n.stride if n.transposed else ts // n.stride
            k3 = (n.kernel == 3 and n.stride == 1 and not n.transposed and i + 1 < len(nodes)
                  and nodes[i + 1].kernel == 1 and nodes[i + 1].residual == n.src)
            k1 = n.kernel == 1 and n.residual is not None
            if part in w["parts"]:
                out[n.name] = (n, ts, k3, k3 or k1)
    return cfg, out


def _conv_t_in(w, n, ts, member):
    """(stream form, t_in, noring allowed) combinations a conv key may carry."""
    if "block" not in w:
        return {(0, ts, False)}
    if n.transposed:
        return {(1, 1 + ts, False), (1, 1 + ts, True)}
    sd = (n.stride - n.pad[1] % n.stride) % n.stride
    need = n.pad[0] + n.pad[1] + sd
    ok = {(0, need - sd + ts, False), (0, need - sd + ts, True)}
    if member:                       # fused or not is decided on the one-shot convs at the block's length
        ok.add((0, ts, False))
    return ok


def test_all_nine_files_are_known():
    assert len(FILES) == 9, FILES
    for f in FILES:
        name, mode = _split_name(f)
        assert name in WORKLOADS, f


@pytest.mark.parametrize("fname", FILES)
def test_pinned_file_matches_its_workload(fname):
    name, mode = _split_name(fname)
    w = WORKLOADS[name]
    allowed = MODES[mode]
    cfg, nodes = _nodes(w)
    B = w["B"]
    T = w.get("block", w.get("T"))
    F = T // cfg.n_band
    with open(os.path.join(TUNING, fname)) as fh:
        entries = json.load(fh)
    assert entries, fname
    keys = [e[0] for e in entries]
    dup = sorted({k for k in keys if keys.count(k) > 1})
    assert not dup, f"{fname}: keys pinned twice: {dup}"
    for e in entries:
        assert len(e) == 3 and isinstance(e[0], str) and isinstance(e[1], int) and e[1] >= 0, (fname, e)
        key, val = e[0], e[1]
        p = key.split("|")
        kind = p[0]
        if kind in ("conv", "unit", "fuse", "stack"):
            assert p[1] in nodes, f"{fname}: {key}: no such node in the {name} plans"
            n, ts, k3, member = nodes[p[1]]
        if kind == "conv":
            assert len(p) in (5, 6) and (len(p) == 5 or p[5] == "noring"), (fname, key)
            sf, kb, kt = int(p[2]), int(p[3]), int(p[4])
            assert kb == B, f"{fname}: {key}: batch {kb}, the workload's is {B}"
            want = _conv_t_in(w, n, ts, member)
            assert (sf, kt, len(p) == 6) in want, f"{fname}: {key}: the plan asks for one of {sorted(want)}"
            prec, config = val // 65536, val % 65536
            assert prec in allowed, f"{fname}: {key}: precision {prec} is not one {mode} may choose"
            assert 0 <= config <= 1024, (fname, key, config)
            assert len(p) == 5 or prec not in (F32_RING, BF16X3), f"{fname}: {key}: a 16-byte-row kernel on a noring key"
        elif kind in ("unit", "fuse", "stack"):
            assert len(p) == 4 and k3, (fname, key)
            assert (int(p[2]), int(p[3])) == (B, ts), f"{fname}: {key}: the plan asks for B {B}, T {ts}"
            if kind == "unit":
                assert val & 255 in allowed and val >> 8 in (0, 1, 2), (fname, key, val)
            else:
                assert val in (0, 1), (fname, key, val)
        elif kind == "pqa":
            assert len(p) == 4 and (int(p[1]), int(p[2])) == (B, T) and int(p[3]) >= T, (fname, key)
            assert ("block" in w) == (int(p[3]) > T), (fname, key)      # a stream reads its history too
            assert val in allowed, (fname, key, val)
        elif kind == "pqs":
            assert len(p) == 5 and (int(p[1]), int(p[2])) == (B, F), (fname, key)
            assert ("block" in w) == (int(p[3]) > F), (fname, key)
            assert val in allowed, (fname, key, val)
        elif kind in ("head", "tail"):
            assert len(p) == 4 and int(p[1]) in allowed - {F32}, (fname, key)
            assert (int(p[2]), int(p[3])) == (B, T if kind == "head" else F), (fname, key)
            assert kind == "tail" or "encoder" in w["parts"], (fname, key)
            assert val in (0, 1), (fname, key, val)
        else:
            raise AssertionError(f"{fname}: unknown key kind in {key!r}")


def test_drift_guard_catches_a_stale_key():
    """The guard itself: a key at another batch, at another length, of a node
    the graph does not have, or in an arithmetic the mode cannot choose fails."""
    w = WORKLOADS["c3"]
    cfg, nodes = _nodes(w)
    n, ts, k3, member = nodes["decoder.net.2"]
    assert n.transposed and _conv_t_in(w, n, ts, member) == {(1, 3, False), (1, 3, True)}
    n, ts, k3, member = nodes["decoder.net.3.aligned.branches.0.net.1"]
    assert k3 and (0, 4, False) in _conv_t_in(w, n, ts, member) and (0, 6, True) in _conv_t_in(w, n, ts, member)
    assert (0, 5, True) not in _conv_t_in(w, n, ts, member)
    assert "encoder.encoder.net.0" not in _nodes(WORKLOADS["c5"])[1]
    assert BF16X3 not in MODES["auto"] and SPLIT16 not in MODES["f32_bf3"]
