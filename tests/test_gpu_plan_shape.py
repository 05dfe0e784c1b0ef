"""The shape of the plans the engine builds: op kinds, precisions and labels of the
encode and decode plans, and the launches of a 1-hop stream, against
tests/golden/plan_shape.json (recorded by ``tools/plan_digest.py --shape`` before
the engine's op builders were folded onto one conv emitter and one edge path,
DESIGN.md section 24).  Runs on an MI355X only (``-m gpu``).

Cases, all at batch 2 with a single arithmetic (no choice depends on a timing):
the small v2 config in exact fp32 and in split-f16, the small causal config
(cached transposed convs, residual delays), and full-width v2 in split-f16, the
one whose shapes qualify for both fused path edges (built without fused units:
their cooperative forms are chosen by timing).  The comparison is exact."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "plan_digest.py")
EDGES = "g_v2_split16"


@pytest.fixture(scope="module")
def want():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(os.path.join(REPO, "tests", "golden", "plan_shape.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def got():
    return {}


def _shape(got, name):
    from tools import plan_digest
    if name not in got:
        got[name] = json.loads(json.dumps(plan_digest.shape(name)))    # (tuples -> lists, as the file has them)
    return got[name]


@pytest.mark.parametrize("name", ["a_v2_small_f32", "b_v2_small_split16", "d_causal_small_f32", EDGES])
def test_plan_shape_is_the_recorded_one(want, got, name):
    g = _shape(got, name)
    for part in ("encode", "decode", "stream_1hop"):
        assert g[part] == want[name][part], f"{name}: {part} differs from tests/golden/plan_shape.json"


def test_edges_fused_where_the_shapes_qualify(want, got):
    """Head: split-f16 or ring arithmetic, first conv k=7 into <= 64 channels; tail:
    last conv k=7 from exactly 64 channels.  Exact-fp32-only models have no edge
    arithmetic; capacity 8 qualifies for the head alone; capacity 64 for both."""
    from rave_amd import _native as N
    kinds = {name: ([o[0] for o in _shape(got, name)["encode"]], [o[0] for o in _shape(got, name)["decode"]])
             for name in ("a_v2_small_f32", "b_v2_small_split16", EDGES)}
    enc, dec = kinds[EDGES]
    assert enc[0] == N.OP_HEAD and N.OP_PQMF_ANALYSIS not in enc
    assert dec[-1] == N.OP_TAIL and N.OP_PQMF_SYNTHESIS not in dec
    head, tail = _shape(got, EDGES)["encode"][0], _shape(got, EDGES)["decode"][-1]
    assert head[1:] == [N.PREC_SPLIT16, "encoder_head:pqmf_analysis+encoder.encoder.net.0"]
    assert tail[1] == N.PREC_SPLIT16 and tail[2].startswith("decoder_tail:decoder.net.") \
        and tail[2].endswith("+pqmf_synthesis")
    enc, dec = kinds["b_v2_small_split16"]
    assert enc[0] == N.OP_HEAD and dec[-2:] == [N.OP_CONV, N.OP_PQMF_SYNTHESIS]
    enc, dec = kinds["a_v2_small_f32"]
    assert enc[:2] == [N.OP_PQMF_ANALYSIS, N.OP_CONV] and dec[-2:] == [N.OP_CONV, N.OP_PQMF_SYNTHESIS]
    assert N.OP_HEAD not in enc and N.OP_TAIL not in dec


def test_edges_switch_keeps_the_two_ops(want, tmp_path):
    """RAVE_EDGES=0 (read once per process, hence the child): the PQMF op and the
    conv as separate ops in the fused op's place, every other op as recorded."""
    from rave_amd import _native as N
    out = tmp_path / "shape.json"
    r = subprocess.run([sys.executable, TOOL, "--shape", "--cases", EDGES, "--out", str(out)],
                       env=dict(os.environ, RAVE_EDGES="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as fh:
        off = json.load(fh)[EDGES]
    w = want[EDGES]
    conv0, convw = "encoder.encoder.net.0", w["decode"][-1][2][len("decoder_tail:"):-len("+pqmf_synthesis")]
    assert off["encode"][:2] == [[N.OP_PQMF_ANALYSIS, N.PREC_SPLIT16, "pqmf_analysis"],
                                 [N.OP_CONV, N.PREC_SPLIT16, conv0]]
    assert off["decode"][-2:] == [[N.OP_CONV, N.PREC_SPLIT16, convw],
                                  [N.OP_PQMF_SYNTHESIS, N.PREC_SPLIT16, "pqmf_synthesis"]]
    # the head also wrote the speaker channels: unfused, a fill op ends the plan
    assert off["encode"][2:] == w["encode"][1:] + [[N.OP_FILL, -1, "fill"]]
    assert off["decode"][:-2] == w["decode"][:-1]
    assert off["stream_1hop"] == w["stream_1hop"]      # stream plans never fuse the edges
