"""The YIN and f0 one-hot kernels (rave_yin / rave_f0_onehot / rave_pitch_onehot,
rave_amd/csrc/pitch.hip) swept at their edges through the C boundary, against
the exact float64 sums of tests/pitch_ref.py (d_truth: YIN's definition, no
cancellation) and the bound derived there (cmdf_bound: the worst case of any
double evaluation of the kernel's three-sum formula).  tests/test_pitch_host.py
checks the reference, the bound and every constructed situation on the CPU.

Cases (tests/pitch_ref.py SWEEP, sr 16000):
  sweep  tau_max in 3 4 5 63 64 65 66 254 255 256 257 258 259 260 513 1023 2205
         (both launch forms and their border, every tau_max % 4 in each, L % 4
         == 2, frames with fewer lags than threads), tau_min in 0, 1,
         tau_max // 5, tau_max - 2; 2-3 glide rows plus silence, glide + 10 DC,
         an impulse, a cosine of period tau_min + 1 (index 0 below the
         threshold), one of period tau_max - 1 (the last searched index), a
         sine still falling at the end, and a row with one NaN / one inf; 50 or
         55 frames (never whole workgroups of four); 2205 runs two frames
  frame  tau_max 5 / 64 / 257, t_len in 1, L - 1, L, L + 1, L + stride - 1,
         L + stride (and 5 and 7 frames of one row), stride 1, 3, L, L + 5
  thr    thresholds 0, -1, 2, +inf and 0.1 on one geometry per launch form
Every call reads x from an interior view of a NaN buffer at a base 4 bytes off
16-byte alignment and writes f0 / cmdf / y inside guarded buffers: the guards
keep their bits, x is unchanged and a second call repeats the first bit for bit.
The fused op runs on every geometry, without and with f0 and cmdf, into a y
with padded channel and batch strides, and equals rave_yin + rave_f0_onehot.

Bounds: |cmdf - truth| <= cmdf_bound + 2^-23 |truth| per element (the second
term the fp32 store), and on the sweep's glide rows also the older 4 e_ref;
idx equal to the truth's on every frame whose margin reaches the frame's
largest bound (EXCUSED_CAP of a case's frames may fall below it); f0 within 1
ulp of float32(sr / period); a frame holding a NaN or inf gives f0 = 0 and an
all-NaN cmdf, as the float64 restatement does.  One-hot: classes of float64
f0_classes; tests/test_pitch_host.py shows float64 itself puts a rounded edge
and its fp32 neighbours out to +-2 ulp within ONEHOT_EDGE of the edge (one ulp
of f0 moves v by 1e-8 to 2e-8), so those are excused but must land in one of
the edge's two classes; at +-128 ulp the class must be right; a log-uniform
sample carries ONEHOT_CAP.

Measured on an MI355X, one run of this module.  Per group: the worst err /
(bound + 2^-23 |truth|) of each row kind (for the NaN / inf rows over their clean
frames; no row kind of any group had a frame excused or differing), the worst
err / e_ref on the glide rows, frames, voiced frames, excused and differing
frames, and on the DC rows the distance to the truth of the kernel (one fp32
rounding of a cmdf of order 1) beside the float64 FFT restatement's.  Nothing
exceeds 0.5: the kernel's cmdf is the truth rounded to fp32, its double error
never shows next to the store's.  Where e_ref is 0 (one-sample signals, cmdf 1
at every lag) the kernel is exact too.  sil = silence, imp = impulse, smin /
slast = period tau_min + 1 / tau_max - 1, fall = falling to the end.
  group       glide   sil    dc   imp  smin slast  fall   nan   inf  e_ref frames voiced exc dif  dc: kernel / fft64
  sweep    3 0.447 0.000 0.430 0.250 0.000 0.000 0.312 0.427 0.427  0.791    105      5   0   0  5.36e-08 / 3.11e-13
  sweep    4 0.494 0.000 0.274 0.333 0.000 0.178 0.426 0.319 0.319  0.552    160     10   0   0  2.89e-08 / 2.52e-13
  sweep    5 0.392 0.000 0.403 0.333 0.000 0.376 0.250 0.389 0.389  0.352    155     14   0   0  4.53e-08 / 2.56e-13
  sweep   63 0.492 0.000 0.494 0.455 0.422 0.456 0.495 0.460 0.460  0.285    210     76   0   0  5.93e-08 / 8.55e-12
  sweep   64 0.488 0.000 0.495 0.478 0.406 0.473 0.482 0.480 0.480  0.320    210     73   0   0  5.95e-08 / 3.01e-12
  sweep   65 0.494 0.000 0.478 0.478 0.388 0.474 0.474 0.491 0.491  0.235    210     75   0   0  5.94e-08 / 3.58e-12
  sweep   66 0.490 0.000 0.479 0.478 0.450 0.451 0.473 0.490 0.490  0.287    210     71   0   0  5.95e-08 / 3.29e-12
  sweep  254 0.496 0.000 0.494 0.488 0.482 0.488 0.486 0.478 0.478  0.230    210     49   0   0  1.18e-07 / 8.86e-11
  sweep  255 0.493 0.000 0.486 0.488 0.482 0.488 0.488 0.477 0.477  0.289    210     63   0   0  1.14e-07 / 7.91e-11
  sweep  256 0.494 0.000 0.488 0.472 0.456 0.490 0.489 0.480 0.480  0.563    210     83   0   0  1.19e-07 / 2.24e-10
  sweep  257 0.497 0.000 0.495 0.472 0.495 0.492 0.494 0.492 0.492  0.527    210     60   0   0  1.19e-07 / 1.80e-10
  sweep  258 0.497 0.000 0.483 0.472 0.483 0.480 0.484 0.485 0.485  0.244    210     69   0   0  1.18e-07 / 1.59e-10
  sweep  259 0.494 0.000 0.490 0.469 0.483 0.485 0.492 0.493 0.493  0.328    210     65   0   0  1.18e-07 / 1.57e-10
  sweep  260 0.488 0.000 0.490 0.469 0.466 0.494 0.488 0.479 0.479  0.376    210     61   0   0  1.14e-07 / 2.09e-10
  sweep  513 0.495 0.000 0.494 0.475 0.486 0.480 0.480 0.494 0.494  0.218    210     60   0   0  1.19e-07 / 1.96e-10
  sweep 1023 0.497 0.000 0.491 0.484 0.484 0.489 0.490 0.496 0.496  0.200    210     70   0   0  1.19e-07 / 1.21e-10
  sweep 2205 0.493     -     -     -     -     -     -     -     -  0.239      8      3   0   0  -
  frame    5 0.458     -     -     -     -     -     -     -     -  0.886     75     21   0   0  - (4 cases e_ref 0)
  frame   64 0.492     -     -     -     -     -     -     -     -  1.000     75     35   0   0  - (2 cases e_ref 0)
  frame  257 0.497     -     -     -     -     -     -     -     -  1.000     75     28   0   0  - (1 cases e_ref 0)
  thr     64 0.483     -     -     -     -     -     -     -     -  0.109     75     14   0   0  -
  thr    257 0.493     -     -     -     -     -     -     -     -  0.183     75      9   0   0  -
One-hot (edge values are the rounded edges and their neighbours; all that differ
from float64 within 2 ulp are in the edge's other class):
  bins 1: 14 values, 3 of the 10 within 2 ulp differ, 0 of the 4 at 128 ulp; sample 771: 0 near, 0 differ
  bins 2: 21 values, 3 of the 15 within 2 ulp differ, 0 of the 6 at 128 ulp; sample 771: 0 near, 0 differ
  bins 256: 1799 values, 353 of the 1285 within 2 ulp differ, 0 of the 514 at 128 ulp; sample 771: 1 near, 0 differ
  bins 4096: 3584 values, 724 of the 2560 within 2 ulp differ, 0 of the 1024 at 128 ulp; sample 771: 5 near, 0 differ
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import pitch_ref as R
from tests.test_gpu_aux_kernels import DEV, NAN, _N, _st, guarded, put, same_bits, untouched

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
FUSED_BINS = {"sweep": 256, "frame": 64, "thr": 2}


def _group(kind, tau_max):
    return [n for n, c in R.SWEEP.items() if c["kind"] == kind and c["tau_max"] == tau_max]


def _args(c, rows, x=0, f0=0, cmdf=0, **over):
    a = _N().YinArgs(rows=rows, t_len=c["T"], sample_rate=c["sr"], pitch_min=c["pmin"], pitch_max=c["pmax"],
                     frame_stride=c["stride_s"], threshold=c["threshold"], x_sr=c["T"], x=x, f0=f0, cmdf=cmdf)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _hot_args(batch, frames, bins, ybuf, yview, f0=0):
    return _N().F0OneHotArgs(batch=batch, frames=frames, bins=bins, log_lo=R.LOG_LO, log_span=R.LOG_SPAN,
                             y_sb=ybuf.stride(0), y_sc=ybuf.stride(1), f0=f0, y=yview.data_ptr())


def _y(batch, bins, frames):
    """A one-hot target with two sentinel channels before and one after, five
    sentinel floats behind every row, so y_sc > frames and y_sb > bins y_sc + frames."""
    return guarded((batch, bins + 1, frames), [(0, 0), (2, 1), (0, 5)], fill=SENTINEL)


def _outputs(rows, F, m):
    return guarded((rows * F,), [(5, 7)]), guarded((rows * F * m,), [(5, 7)])


def _one_hot_ok(y):
    return bool(((y == 0) | (y == 1)).all()) and bool((y.sum(1) == 1).all())


@functools.lru_cache(maxsize=None)
def _run(name):
    """(f0 (rows, F), cmdf (rows, F, m)) of rave_yin on the case, on the CPU as
    float64 numpy, computed once; the guards, the rerun and the fused op in its
    forms are checked on the way."""
    N = _N()
    c, x = R.SWEEP[name], R.sweep_input(name)
    rows, F, m, bins = len(x), c["frames"], c["m"], FUSED_BINS[c["kind"]]
    shape = (N.i32 * 5)()
    N.check(N.lib.rave_yin_shape(C.byref(_args(c, rows)), shape))
    assert list(shape) == [c["tau_min"], c["tau_max"], c["L"], c["stride"], F], name
    xbuf, xv, xmask = put(x.reshape(-1), [(1, 11)])
    assert xv.data_ptr() % 16 == 4
    x_dev = xv.clone()

    def call(fn, *guards):
        N.check(fn())
        torch.cuda.synchronize()
        assert untouched(xbuf, xmask) and same_bits(xv, x_dev), name
        for buf, mask, fill in guards:
            assert untouched(buf, mask, fill), name

    outs = []
    for _ in range(2):
        (fb, fv, fm), (cb, cv, cm) = _outputs(rows, F, m)
        a = _args(c, rows, xv.data_ptr(), fv.data_ptr(), cv.data_ptr())
        call(lambda: N.lib.rave_yin(C.byref(a), _st()), (fb, fm, NAN), (cb, cm, NAN))
        outs.append((fv, cv))
    (f0, cmdf), (f0_2, cmdf_2) = outs
    assert same_bits(f0, f0_2) and same_bits(cmdf, cmdf_2), name
    assert not bool(torch.isnan(f0).any()), name

    # the one-hot of that contour, then the fused op: y alone; y with f0 and cmdf
    yb, yv, ym = _y(rows, bins, F)
    h = _hot_args(rows, F, bins, yb, yv, f0.data_ptr())
    call(lambda: N.lib.rave_f0_onehot(C.byref(h), _st()), (yb, ym, SENTINEL))
    assert _one_hot_ok(yv), name
    yb1, yv1, ym1 = _y(rows, bins, F)
    h1 = _hot_args(rows, F, bins, yb1, yv1)
    a1 = _args(c, rows, xv.data_ptr())
    call(lambda: N.lib.rave_pitch_onehot(C.byref(a1), C.byref(h1), _st()), (yb1, ym1, SENTINEL))
    assert same_bits(yv1, yv), name
    yb2, yv2, ym2 = _y(rows, bins, F)
    (fb, fv, fm), (cb, cv, cm) = _outputs(rows, F, m)
    h2 = _hot_args(rows, F, bins, yb2, yv2)
    a2 = _args(c, rows, xv.data_ptr(), fv.data_ptr(), cv.data_ptr())
    call(lambda: N.lib.rave_pitch_onehot(C.byref(a2), C.byref(h2), _st()),
         (yb2, ym2, SENTINEL), (fb, fm, NAN), (cb, cm, NAN))
    assert same_bits(yv2, yv) and same_bits(fv, f0) and same_bits(cv, cmdf), name
    return f0.cpu().double().numpy().reshape(rows, F), cmdf.cpu().double().numpy().reshape(rows, F, m)


def _judge(name, stats):
    """The cmdf and the decisions of one case against the truth, row by row."""
    c, t = R.SWEEP[name], R.sweep_truth(name)
    f0, cmdf = _run(name)
    sr, tau_min, m, thr = c["sr"], c["tau_min"], c["m"], c["threshold"]
    p = t["poisoned"]
    assert np.isnan(cmdf[p]).all() and np.isfinite(cmdf[~p]).all(), name
    assert np.isnan(t["fft64"][p]).all() and (f0[p] == 0).all(), name
    err = np.abs(cmdf - t["cmdf"])
    tol = t["bound"] + 2.0 ** -23 * np.abs(t["cmdf"])
    with np.errstate(all="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    glide = [r for r, row in enumerate(c["rows"]) if row == "glide"]
    e_ref = float(np.abs(t["fft32"][glide] - t["fft64"][glide]).max())
    for r, row in enumerate(c["rows"]):
        ok = ~p[r]
        worst = float(ratio[r][ok].max())
        e = float(err[r][ok].max())
        fft = float(np.abs(t["fft64"][r][ok] - t["cmdf"][r][ok]).max())
        print(f"{name} row {r} {row}: err {e:.3e} err/bound {worst:.3f} fft64 off the truth {fft:.2e}")
        s = stats.setdefault(row, dict(ratio=0.0, err=0.0, fft=0.0))
        s["ratio"], s["err"], s["fft"] = max(s["ratio"], worst), max(s["err"], e), max(s["fft"], fft)
        assert worst <= 1.0, (name, row, worst)
    g_err = float(err[glide].max())
    print(f"{name}: glide rows err {g_err:.3e} e_ref {e_ref:.3e} err/e_ref {g_err / max(e_ref, 1e-300):.3f}")
    # the older yardstick, on every case.  Where the fp32 restatement is exact (e_ref == 0: the one-sample
    # signals of the framing cases, whose cmdf is 1 at every lag) this asks the kernel to be exact as well.
    assert g_err <= 4 * e_ref, (name, g_err, e_ref)
    stats["e_ref"] = max(stats.get("e_ref", 0.0), g_err / e_ref if e_ref > 0 else 0.0)
    stats["e_ref_zero"] = stats.get("e_ref_zero", 0) + (e_ref == 0)

    # decisions
    with np.errstate(all="ignore"):
        got_idx = np.where(f0 > 0, np.rint(sr / f0) - tau_min - 1, 0).astype(np.int64)
    want = np.where(t["idx"] > 0, sr / (t["idx"] + tau_min + 1.0), 0.0).astype(np.float32)
    ulp = np.abs(np.nextafter(want, np.float32(np.inf)) - want)
    agree = np.abs(f0 - want.astype(np.float64)) <= ulp
    excused = t["margin"] < t["limit"]
    stats["frames"] = stats.get("frames", 0) + excused.size
    stats["excused"] = stats.get("excused", 0) + int(excused.sum())
    stats["differ"] = stats.get("differ", 0) + int((~agree).sum())
    stats["voiced"] = stats.get("voiced", 0) + int((f0 > 0).sum())
    for r, row in enumerate(c["rows"]):
        stats[row]["excused"] = stats[row].get("excused", 0) + int(excused[r].sum())
        stats[row]["differ"] = stats[row].get("differ", 0) + int((~agree[r]).sum())
    assert excused.sum() <= R.EXCUSED_CAP * excused.size, name
    assert (agree | excused).all(), (name, f0[~agree], want[~agree])
    assert ((f0 == 0) == (t["idx"] == 0))[~excused].all(), name
    assert ((got_idx >= 0) & (got_idx < m)).all(), name
    assert (got_idx == t["idx"])[~excused].all(), name
    # the constructed rows, on the kernel's own output
    for r, row in enumerate(c["rows"]):
        what = R.intended(name).get(row)
        if what == "last":
            assert (got_idx[r] == m - 1).all() and m > 1 and (cmdf[r][:, 0] >= thr).all(), (name, row, got_idx[r])
        elif what == "first0":
            assert (f0[r] == 0).all() and (cmdf[r][:, 0] < thr).all(), (name, row)
        elif what == "unvoiced":
            hit = cmdf[r].any(-1)
            assert (f0[r] == 0).all() and hit.any() and (cmdf[r][hit] >= thr).all(), (name, row)
        if row == "silence":
            assert (cmdf[r] == 0).all(), name


def _report(tag, stats):
    rows = " ".join(f"{k} {v['ratio']:.3f}/{v['excused']}/{v['differ']}"
                    for k, v in stats.items() if isinstance(v, dict))
    print(f"MEASURED {tag}: err/bound/excused/differ by row: {rows}; glide err/e_ref {stats['e_ref']:.3f} "
          f"({stats['e_ref_zero']} cases with e_ref 0); "
          f"{stats['frames']} frames, {stats['voiced']} voiced, {stats['excused']} excused, {stats['differ']} differ"
          + (f"; dc row: kernel off the truth by {stats['dc']['err']:.2e}, fft64 by {stats['dc']['fft']:.2e}"
             if "dc" in stats else ""))


@pytest.mark.parametrize("tau_max", R.SWEEP_TAU_MAX)
def test_sweep(tau_max):
    stats = {}
    names = _group("sweep", tau_max)
    assert len(names) >= 2
    for name in names:
        _judge(name, stats)
    _report(f"sweep tau_max {tau_max}", stats)
    if tau_max >= 63:
        assert stats["voiced"] > 0


@pytest.mark.parametrize("tau_max", R.FRAME_TAU_MAX)
def test_framing(tau_max):
    stats = {}
    names = _group("frame", tau_max)
    assert {len(R.SWEEP[n]["rows"]) * R.SWEEP[n]["frames"] for n in names} >= {1, 2, 3, 5, 7}
    for name in names:
        _judge(name, stats)
    _report(f"frame tau_max {tau_max}", stats)


@pytest.mark.parametrize("tau_max", [64, 257])
def test_thresholds(tau_max):
    stats = {}
    for name in _group("thr", tau_max):
        _judge(name, stats)
        thr = R.SWEEP[name]["threshold"]
        f0 = _run(name)[0]
        if thr != R.THRESHOLD:
            assert (f0 == 0).all(), name           # none below 0 and -1; index 0 below 2 and +inf
        else:
            assert (f0 > 0).any() and (f0 == 0).any(), name
    _report(f"thr tau_max {tau_max}", stats)


# ------------------------------------------------------------------ one-hot
def _onehot(values, batch, frames, bins):
    """Classes (batch * frames) the kernel gives `values`, through a strided y."""
    N = _N()
    fb, fv, fm = put(values, [(3, 5)])
    yb, yv, ym = _y(batch, bins, frames)
    h = _hot_args(batch, frames, bins, yb, yv, fv.data_ptr())
    got = []
    for _ in range(2):
        yv.fill_(SENTINEL)
        N.check(N.lib.rave_f0_onehot(C.byref(h), _st()))
        torch.cuda.synchronize()
        assert untouched(yb, ym, SENTINEL) and untouched(fb, fm)
        assert same_bits(fv, torch.as_tensor(values).to(DEV))
        assert _one_hot_ok(yv), (batch, frames, bins)
        got.append(yv.clone())
    assert same_bits(*got)
    return got[0].argmax(1).reshape(-1).cpu().numpy()


@pytest.mark.parametrize("bins", [1, 2, 256, 4096])
def test_onehot_edges_specials_and_geometries(bins):
    edge, k, off = R.onehot_edges(bins)
    special = np.float32(R.ONEHOT_SPECIAL)
    sample = R.onehot_sample(771)
    pool = np.concatenate([edge, special, sample])
    kind = np.concatenate([np.zeros(len(edge), int), np.ones(len(special), int), np.full(len(sample), 2)])
    want = R.f0_classes(torch.from_numpy(pool).double(), bins).numpy()
    vs = R.f0_norm(torch.from_numpy(sample).double()).numpy() * bins
    near = np.abs(vs - np.round(vs)) / bins < R.ONEHOT_EDGE
    assert near.sum() <= R.ONEHOT_CAP * len(sample)
    got = np.full(len(pool), -1)
    # the whole pool at (3, 257), then every other geometry on a window of it that holds edges, specials and sample
    for at in range(0, len(pool), 3 * 257):
        sl = np.arange(at, at + 3 * 257) % len(pool)
        got[sl] = _onehot(pool[sl], 3, 257, bins)
    assert (got >= 0).all()
    for batch in (1, 3):
        for frames in (1, 255, 256, 257):
            sl = (len(edge) - (batch * frames) // 2 + np.arange(batch * frames)) % len(pool)
            again = _onehot(pool[sl], batch, frames, bins)
            assert np.array_equal(again, got[sl]), (batch, frames)
    e, s, p = kind == 0, kind == 1, kind == 2
    assert (got[s] == bins).all() and (want[s] == bins).all(), got[s]
    above, below = np.where(k < bins, k, bins), np.where(k > 0, k - 1, bins)
    far = np.abs(off) == R.ONEHOT_FAR
    assert np.array_equal(got[e][far], want[e][far])
    assert ((got[e] == above) | (got[e] == below)).all()
    differ_p = got[p] != want[p]
    assert not (differ_p & ~near).any(), (sample[differ_p], got[p][differ_p], want[p][differ_p])
    print(f"MEASURED one-hot bins {bins}: {len(edge)} edge values, {int((got[e] != want[e]).sum())} of the "
          f"{int((~far).sum())} within 2 ulp differ from float64, 0 of the {int(far.sum())} at 128 ulp; "
          f"sample {len(sample)}: {int(near.sum())} near an edge, {int(differ_p.sum())} differ")


# ------------------------------------------------------------------ refusals
def _refused(fn, exc, text):
    N = _N()
    with pytest.raises(exc) as info:
        fn()
    last = N.lib.rave_last_error().decode()
    assert text in str(info.value) and text in last, (str(info.value), last)


def test_refusals_leave_the_outputs_alone():
    N = _N()
    from rave_amd import config as rcfg
    from rave_amd.pitch import PitchConditioner, _audio
    c = dict(R.SWEEP["sweep-64-12"])
    x = torch.zeros(2 * c["T"], device=DEV)
    F = c["frames"]
    f0 = torch.full((2 * F,), SENTINEL, device=DEV)
    cmdf = torch.full((2 * F * c["m"],), SENTINEL, device=DEV)
    y = torch.full((2, 257 + 3, F + 3), SENTINEL, device=DEV)

    def yin(**over):
        a = _args(c, 2, x.data_ptr(), f0.data_ptr(), cmdf.data_ptr(), **over)
        return lambda: N.check(N.lib.rave_yin(C.byref(a), _st()))

    def hot(**over):
        h = N.F0OneHotArgs(batch=2, frames=F, bins=256, log_lo=R.LOG_LO, log_span=R.LOG_SPAN, y_sb=y.stride(0),
                           y_sc=y.stride(1), f0=f0.data_ptr(), y=y.data_ptr())
        for k, v in over.items():
            setattr(h, k, v)
        return h

    _refused(yin(pitch_min=c["sr"] / 2206.5), NotImplementedError, "exceeds 4410")            # tau_max 2206
    N.check(N.lib.rave_yin_shape(C.byref(_args(c, 2, pitch_min=c["sr"] / 2205.5, t_len=5000)), (N.i32 * 5)()))
    for bins in (0, 3, 8192):
        h = hot(bins=bins)
        _refused(lambda: N.check(N.lib.rave_f0_onehot(C.byref(h), _st())), NotImplementedError, "power of two")
    for over, text in [(dict(y_sc=F - 1), "y_sc below frames"),
                       (dict(y_sb=256 * y.stride(1) + F - 1), "y_sb overlaps batches")]:
        h = hot(**over)
        _refused(lambda: N.check(N.lib.rave_f0_onehot(C.byref(h), _st())), ValueError, text)
        a = _args(c, 2, x.data_ptr())
        _refused(lambda: N.check(N.lib.rave_pitch_onehot(C.byref(a), C.byref(h), _st())), ValueError, text)
    a = _args(c, 2, x.data_ptr())
    for over in (dict(batch=3), dict(frames=F + 1, y_sc=F + 3), dict(frames=F - 1)):
        h = hot(**over)
        _refused(lambda: N.check(N.lib.rave_pitch_onehot(C.byref(a), C.byref(h), _st())), ValueError, "the contour (")
    # layouts the wrapper cannot hand over as rows at one stride
    cond = PitchConditioner(rcfg.v2())
    T = 4096
    frames = cond.yin.shape(T, cond.yin.block_stride(T, cond.block_size))["frames"]
    base = torch.zeros(2, 3, 2 * T, device=DEV)
    bad = [torch.zeros(1, T, device=DEV).expand(2, T), base[0, :2, ::2], base[:, :2, :T]]
    assert [_audio(b)[2] for b in bad] == [0, 0, 0]
    assert _audio(base[0, :2, :T])[2] == 2 * T and _audio(base[:, :, :T])[2] == 2 * T      # nested, not contiguous
    for b in bad:
        rows = b.numel() // T
        out = torch.full((rows, 257, frames), SENTINEL, device=DEV)
        f0w = torch.full((rows, frames), SENTINEL, device=DEV)
        _refused(lambda: cond.pitch_onehot(b, out, f0=f0w), ValueError, "rows of x must be contiguous")
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((f0w == SENTINEL).all())
    torch.cuda.synchronize()
    for t in (f0, cmdf, y):
        assert bool((t == SENTINEL).all())             # nothing was launched
