"""Per-row target speakers, the parts that need no GPU: the library's new
entry points, the struct mirrors, and the argument checks of the Python
wrappers (rave_amd.model.speaker_arg is what RAVE.set_speaker and
StreamingRAVE.set_speaker validate with before they touch the device)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_library_exports_the_speaker_entries():
    from rave_amd import _native as N
    for name in ("rave_model_set_speaker", "rave_model_set_speakers", "rave_model_set_speaker_row0",
                 "rave_model_speaker_info"):
        assert name in N.EXPORTS
        assert hasattr(N.lib, name), name
    assert N.ABI_VERSION == N.lib.rave_abi_version() == 21


def test_struct_mirrors():
    """The stride fields sit where a zero-initialised struct of an older caller
    has zeros: the fill's in its former padding word, the edge's and the
    config's at the end.  sizeof(PlanOp) does not move."""
    from rave_amd import _native as N
    n = N.lib.rave_struct_sizes(None, 0)
    buf = (N.i64 * n)()
    N.lib.rave_struct_sizes(buf, n)
    assert list(buf) == [C.sizeof(s) for s in N.STRUCTS]
    assert C.sizeof(N.PlanOp) == 248 and C.sizeof(N.EdgeArgs) <= N.PAYLOAD
    assert C.sizeof(N.FillArgs) == 48 and N.FillArgs.values_sb.offset == 12
    assert N.EdgeArgs.fill_vs.offset == C.sizeof(N.EdgeArgs) - 8 == N.EdgeArgs.fill_values.offset + 8
    assert N.ModelConfig.speaker_rows.offset == C.sizeof(N.ModelConfig) - 4
    assert N.FillArgs().values_sb == 0 and N.EdgeArgs().fill_vs == 0


def test_model_config_carries_speaker_rows():
    from rave_amd import _native as N
    from rave_amd import config as rcfg
    assert N.model_config(rcfg.v2()).speaker_rows == 0          # the engine's default, SPEAKER_ROWS
    assert N.SPEAKER_ROWS == 64
    assert N.model_config(rcfg.v2(), 4).speaker_rows == 4
    with pytest.raises(ValueError):
        N.model_config(rcfg.v2(), -1)


def test_fill_refuses_a_stride_inside_a_row():
    """A row stride below the channel count would alias rows: RAVE_ERR_ARG from
    the argument check, which runs before any device call."""
    from rave_amd import _native as N
    a = N.FillArgs(batch=2, channels=5, t_len=7, values_sb=3, y=64, y_sb=35, y_sc=7, values=64)
    assert N.lib.rave_fill_channels(C.byref(a), None) == N.RAVE_ERR_ARG
    assert b"values_sb" in N.lib.rave_last_error()


@pytest.mark.parametrize("as_tensor", [False, True])
def test_speaker_arg_accepts_both_forms(as_tensor):
    from rave_amd.model import speaker_arg
    conv = torch.from_numpy if as_tensor else (lambda a: a)
    v = np.arange(256, dtype=np.float32)
    kind, src = speaker_arg(conv(v), 256, 64)
    assert kind == "shared" and tuple(src.shape) == (256,)
    E = np.arange(3 * 256, dtype=np.float32).reshape(3, 256)
    kind, src = speaker_arg(conv(E), 256, 4, row0=1)
    assert kind == "rows" and tuple(src.shape) == (3, 256)
    assert np.array_equal(np.asarray(src), E)
    kind, _ = speaker_arg(conv(E[:1]), 256, 4, row0=3)          # the last row alone
    assert kind == "rows"


@pytest.mark.parametrize("as_tensor", [False, True])
def test_speaker_arg_refusals(as_tensor):
    from rave_amd.model import speaker_arg
    conv = torch.from_numpy if as_tensor else (lambda a: a)
    z = lambda *s: conv(np.zeros(s, np.float32))
    for bad, kw in [(z(255), {}),                     # wrong width, 1-D
                    (z(3, 255), {}),                  # wrong width, 2-D
                    (z(0, 256), {}),                  # no rows
                    (z(1, 3, 256), {}),               # wrong rank
                    (z(), {}),                        # wrong rank (0-D)
                    (z(3, 256), {"row0": 2}),         # rows [2, 5) of a 4-row table
                    (z(5, 256), {}),                  # more rows than the table
                    (z(1, 256), {"row0": 4}),         # row0 past the end
                    (z(1, 256), {"row0": -1}),
                    (z(256), {"row0": 1})]:           # row0 with the shared vector
        with pytest.raises(ValueError):
            speaker_arg(bad, 256, 4, **kw)


def test_speaker_arg_wants_float32_rows():
    """The table takes a device tensor as it is, so a tensor of another dtype is
    refused rather than converted behind the caller's back; numpy input and the
    shared vector convert as they always did."""
    from rave_amd.model import speaker_arg
    with pytest.raises(ValueError):
        speaker_arg(torch.zeros(3, 256, dtype=torch.float64), 256, 4)
    with pytest.raises(ValueError):
        speaker_arg(torch.zeros(3, 256, dtype=torch.float16), 256, 4)
    kind, src = speaker_arg(np.zeros((3, 256), np.float64), 256, 4)
    assert kind == "rows" and src.dtype == np.float32
    kind, src = speaker_arg(torch.zeros(256, dtype=torch.float64), 256, 4)
    assert kind == "shared" and src.dtype == torch.float32
