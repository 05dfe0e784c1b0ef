"""YIN pitch tracking and the f0 one-hot on the GPU (rave_yin / rave_f0_onehot /
rave_pitch_onehot, rave_amd/csrc/pitch.hip) against the float64 restatement of
rave/pitch_utils.py on the CPU (tests/pitch_ref.py, which
tests/golden/make_pitch_check.py checks against the reference's own functions
on these same inputs).

Shapes (tests/pitch_ref.py CASES): est (3, 5000) at stride 0.01 s, 27 frames;
short (1, 1000), shorter than L = 1260, one zero-padded frame; wave sr 16000 at
200-2000 Hz, L = 160, one wave per frame and 75 frames for workgroups of four;
block get_pitch on (2, 1, 16384) with block 1024; max L = 4410, the longest
frame the op accepts.

Bounds: the sliced cmdf within 4 e_ref, e_ref the max-abs error of the fp32 CPU
run of the restatement against float64 on the same input (the rule of the
spectrogram tests); idx equal to float64's on every frame whose deciding
comparisons all have a float64 margin of at least that bound, at most 2 % of a
shape's frames excused; f0 within 1 ulp of float32(sr / period).

Measured on an MI355X (kernel cmdf error / e_ref, excused frames):
est 0.15 / 0, short 0.34 / 0, wave 0.21 / 0, block 0.12 / 0, max 0.01 / 0;
one-hot table: 0 of 520 periods differ, 0 within 1e-6 of an edge."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import pitch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MULTI = [c for c in R.CASES if c != "short"]


def _yin(case):
    from rave_amd.pitch import Yin
    c = R.CASES[case]
    return Yin(c["sr"], c["pmin"], c["pmax"], R.THRESHOLD)


@functools.lru_cache(maxsize=None)
def _gpu(case):
    """(f0, cmdf) of the kernel on the case's input, on the CPU, computed once."""
    x = torch.tensor(R.inputs(case), device=DEV)
    c = R.CASES[case]
    if "block" in c:
        f0 = _yin(case).get_pitch(x, c["block"])
        f0b, cmdf = _yin(case).estimate(x, R.frame_stride(case), return_cmdf=True)
        assert torch.equal(f0, f0b)
    else:
        f0, cmdf = _yin(case).estimate(x, c["stride"], return_cmdf=True)
    torch.cuda.synchronize()
    return f0.cpu(), cmdf.cpu()


@functools.lru_cache(maxsize=None)
def _bound(case):
    """(cmdf64, idx64, e_ref, excused mask): the bound is 4 e_ref."""
    c64, i64, _ = R.reference(case)
    c32, _, _ = R.reference(case, "float32")
    e_ref = float((c32.double() - c64).abs().max())
    idx, margin = R.margins(c64.reshape(-1, c64.shape[-1]).numpy())
    assert np.array_equal(idx, i64.reshape(-1).numpy())
    return c64, i64, e_ref, torch.from_numpy(margin < 4 * e_ref).reshape(i64.shape)


@pytest.mark.parametrize("case", list(R.CASES))
def test_shapes(case):
    tau_min, tau_max, L, stride, frames = R.geometry(case)
    f0, cmdf = _gpu(case)
    shape = R.CASES[case]["shape"]
    assert tuple(f0.shape) == shape[:-1] + (frames,) and f0.dtype == torch.float32
    assert tuple(cmdf.shape) == shape[:-1] + (frames, tau_max - 1 - tau_min)
    g = _yin(case).shape(shape[-1], R.frame_stride(case))
    assert (g["tau_min"], g["tau_max"], g["frame_length"], g["stride"], g["frames"]) == (tau_min, tau_max, L, stride, frames)
    if "block" in R.CASES[case]:
        assert frames == shape[-1] // R.CASES[case]["block"]


@pytest.mark.parametrize("case", list(R.CASES))
def test_cmdf_within_four_e_ref(case):
    c64, _, e_ref, _ = _bound(case)
    err = float((_gpu(case)[1].double() - c64).abs().max())
    print(f"cmdf case {case}: e_ref {e_ref:.3e} kernel {err:.3e} ratio {err / e_ref:.2f}")
    assert err <= 4 * e_ref


@pytest.mark.parametrize("case", list(R.CASES))
def test_period_decisions_and_f0(case):
    c = R.CASES[case]
    tau_min = R.geometry(case)[0]
    _, i64, e_ref, excused = _bound(case)
    f0 = _gpu(case)[0]
    want = torch.where(i64 > 0, (c["sr"] / (i64 + tau_min + 1).double()), torch.zeros(())).float()
    ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float("inf"))) - want)
    agree = (f0 - want).abs() <= ulp           # 1 ulp of f0 is far below the step between two periods
    n_exc = int(excused.sum())
    print(f"decisions case {case}: {i64.numel()} frames, {int((i64 > 0).sum())} voiced, "
          f"{n_exc} excused, {int((~agree).sum())} differ")
    assert n_exc <= R.EXCUSED_CAP * i64.numel()
    assert bool((agree | excused).all()), (f0[~agree], want[~agree])
    assert bool(((f0 == 0) == (i64 == 0))[~excused].all())
    if case in MULTI:
        assert bool((i64 > 0).any()) and bool((i64 == 0).any())
        assert bool((f0 > 0).any()) and bool((f0 == 0).any())


def test_silence_is_unvoiced_and_lands_in_the_last_class():
    from rave_amd.pitch import F0OneHot, Yin
    x = torch.zeros(2, 1, 8192, device=DEV)
    f0, cmdf = Yin().estimate(x, 0.01, return_cmdf=True)
    assert bool((f0 == 0).all()) and bool((cmdf == 0).all())      # 0 * tau / 1e-5
    y = F0OneHot()(f0.reshape(2, -1))
    assert bool((y[:, 256] == 1).all()) and bool((y[:, :256] == 0).all())


@functools.lru_cache(maxsize=None)
def _table():
    from rave_amd.pitch import F0OneHot
    f0 = torch.from_numpy(R.table_f0())
    y = F0OneHot()(f0.to(DEV).reshape(1, -1))
    torch.cuda.synchronize()
    return f0, y.cpu()[0]                       # (257, n)


def test_onehot_table_classes():
    f0, y = _table()
    v = R.f0_norm(f0.double())
    want = R.f0_classes(f0.double())
    near = ((v * 256 - (v * 256).round()).abs() / 256 < R.ONEHOT_EDGE)[:-3]
    got = y.argmax(0)
    differ = got != want
    print(f"one-hot table: {len(f0) - 3} periods, {int(differ.sum())} differ, {int(near.sum())} near an edge")
    assert int(near.sum()) <= R.ONEHOT_CAP * (len(f0) - 3)
    assert bool((~differ[:-3] | near).all())
    assert got[-3:].tolist() == want[-3:].tolist() == [256, 256, 256]     # f0 = 0, v < 0, v >= 1
    assert int(want[:-3].min()) >= 0 and int(want[:-3].max()) < 256


def test_onehot_table_is_exactly_one_hot():
    _, y = _table()
    assert y.shape[0] == 257
    assert bool((y.sum(0) == 1).all())
    assert bool(((y == 0) | (y == 1)).all())
    want = R.f0_one_hot(torch.from_numpy(R.table_f0()).double().reshape(1, -1))[0].T
    near = int((y != want).any(0).sum())
    assert near <= R.ONEHOT_CAP * y.shape[1]


def _zx():
    x = torch.tensor(R.inputs("block"), device=DEV)                      # (2, 1, 16384)
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 5, 16, generator=g).to(DEV)
    return z, x


def test_conditioner_writes_behind_z_and_nowhere_else():
    from rave_amd import config as rcfg
    from rave_amd.pitch import F0OneHot, PitchConditioner, Yin
    cond = PitchConditioner(rcfg.v2())
    z, x = _zx()
    out = cond(z, x)
    f0 = Yin().get_pitch(x, 1024).reshape(2, 16)
    hot = F0OneHot()(f0)
    assert tuple(out.shape) == (2, 5 + 257, 16)
    assert torch.equal(out, torch.cat([z, hot], 1))
    assert torch.equal(out[:, :5], z)
    # a guard band before and after the one-hot's channels
    buf = torch.full((2, 5 + 257 + 3, 16), -7.0, device=DEV)
    cond.pitch_onehot(x, buf, 5)
    assert torch.equal(buf[:, 5:262], hot)
    assert bool((buf[:, :5] == -7).all()) and bool((buf[:, 262:] == -7).all())
    buf2 = torch.full((2, 5 + 257 + 3, 16), -7.0, device=DEV)
    F0OneHot()(f0, out=buf2, channel_offset=5)
    assert torch.equal(buf2, buf)
    # the reference's one-hot of the float64 contour, frames last
    want = R.f0_one_hot(R.reference("block")[2].reshape(2, 16)).permute(0, 2, 1)
    assert torch.equal(hot.cpu(), want)


def test_fused_equals_composed_bitwise_and_reruns():
    from rave_amd import config as rcfg
    from rave_amd.pitch import PitchConditioner
    cond = PitchConditioner(rcfg.v2())
    z, x = _zx()
    f0 = torch.full((2, 16), -1.0, device=DEV)
    a = cond.pitch_onehot(x, torch.empty(2, 257, 16, device=DEV), f0=f0)
    assert torch.equal(f0.cpu(), _gpu("block")[0].reshape(2, 16))
    assert torch.equal(a, cond.onehot(f0))
    assert torch.equal(a, cond.pitch_onehot(x, torch.empty(2, 257, 16, device=DEV)))
    xe = torch.tensor(R.inputs("est"), device=DEV)
    first = _yin("est").estimate(xe, 0.01, return_cmdf=True)
    second = _yin("est").estimate(xe, 0.01, return_cmdf=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_graph_capture_replays_the_eager_result():
    from rave_amd import config as rcfg
    from rave_amd.pitch import PitchConditioner
    cond = PitchConditioner(rcfg.v2())
    z, x = _zx()
    eager = cond(z, x).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cond(z, x)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def _refused(fn, exc, text):
    """fn raises exc before any launch: the message names the cause and
    rave_last_error holds it."""
    from rave_amd import _native as N
    with pytest.raises(exc) as info:
        fn()
    last = N.lib.rave_last_error().decode()
    assert text in str(info.value) and text in last, (str(info.value), last)


def test_refusals():
    from rave_amd import _native as N
    from rave_amd.pitch import F0OneHot, Yin
    x = torch.zeros(2, 4096, device=DEV)
    _refused(lambda: Yin(44100, 19.9, 400.0).estimate(x), NotImplementedError, "exceeds 4410")
    _refused(lambda: Yin(44100, 400.0, 400.0).estimate(x), ValueError, "pitch_max must exceed pitch_min")
    _refused(lambda: Yin(44100, 401.0, 400.0).estimate(x), ValueError, "pitch_max must exceed pitch_min")
    _refused(lambda: Yin(44100, 399.0, 400.0).estimate(x), ValueError, "no lag left to search")     # 110 >= 110 - 1
    _refused(lambda: Yin(44100, 396.0, 400.0).estimate(x), ValueError, "no lag left to search")     # 110 >= 111 - 1
    _refused(lambda: Yin().estimate(x, 0.0), ValueError, "stride 0")
    _refused(lambda: Yin().estimate(x, 1e-5), ValueError, "stride 0")                               # int(0.441)
    wide = torch.zeros(2, 8192, device=DEV)
    _refused(lambda: Yin().estimate(wide[:, :4096]), ValueError, "rows of x must be contiguous")
    _refused(lambda: Yin().estimate(wide[:, ::2]), ValueError, "rows of x must be contiguous")
    _refused(lambda: F0OneHot(255)(torch.zeros(1, 4, device=DEV)), NotImplementedError, "power of two")
    # null pointers, at the C boundary
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f0 = torch.full((2, 7), -1.0, device=DEV)
    a = Yin().args(2, 4096, 0.01)
    for ptrs, text in [((0, f0.data_ptr()), "null x"), ((x.data_ptr(), 0), "null f0")]:
        a.x, a.f0 = ptrs
        _refused(lambda: N.check(N.lib.rave_yin(C.byref(a), stream)), ValueError, text)
    _refused(lambda: N.check(N.lib.rave_yin(None, stream)), ValueError, "null arguments")
    h = N.F0OneHotArgs(batch=2, frames=7, bins=256, log_lo=1.0, log_span=1.0, y_sb=257 * 7, y_sc=7)
    for ptrs, text in [((0, f0.data_ptr()), "null y"), ((f0.data_ptr(), 0), "null f0")]:
        h.y, h.f0 = ptrs
        _refused(lambda: N.check(N.lib.rave_f0_onehot(C.byref(h), stream)), ValueError, text)
    a.x, a.f0 = x.data_ptr(), 0
    h.y = 0
    _refused(lambda: N.check(N.lib.rave_pitch_onehot(C.byref(a), C.byref(h), stream)), ValueError, "null y")
    _refused(lambda: N.check(N.lib.rave_pitch_onehot(C.byref(a), None, stream)), ValueError, "null one-hot arguments")
    torch.cuda.synchronize()
    assert bool((f0 == -1).all())               # nothing was launched
