"""The spectral kernels at their edges (rave_amd/csrc/stft.hip: rave_stft_mag,
rave_audio_distance; stft_loss.hip: rave_stft_loss_forward / _backward; the FFT
of stft_fft.h), called through rave_amd._native at the C boundary, against
tests/spectral_ref.py (numpy float64 from the definition, which
tests/test_spectral_ref_host.py pins to the torch.stft restatements) and, for
gradients and e_ref, the torch autograd of tests/stft_loss_ref.py.

Every input block (signals, tables, grad_out) sits inside a wider NaN-filled
buffer, so an over-read shows as a NaN in the result; every output (y, out,
saved, grad_value, and the workspace beyond its queried size) sits inside one
too.  Every call asserts: the result is finite, the surroundings are untouched,
the inputs are unchanged, the workspace query is exactly what the kernels write
(every float of it is written, none beyond), and a second run gives equal bits.

Shapes (tests/spectral_ref.py: seam_lengths): per scale n, frame counts F in
{3, kConc-1, kConc, kConc+1, kTile-1, kTile, kTile+1, 2 kTile+1} (kConc =
max(1, 1024 / n) frames per pass, kTile = kConc x 4 up to n = 1024 and x 2
above per workgroup), for stft_mag -- whose workgroup owns 2 kTile frames --
also {2 kConc +- 1, 2 kTile - 1, 2 kTile, 2 kTile + 1, 4 kTile + 1}, each at
T = (F-1) hop and (F-1) hop + hop - 1 where T > n/2, plus T = n/2 + 1 (and
n/2 + 2 for the losses: both reflect images land on the same samples), all
seven scales, rows 1 and 3.

Bounds.  Magnitudes: K e_ref, e_ref the max-abs error of fp32 CPU torch.stft
against float64 on the same input.  Distance and loss values: 1e-4 relative,
the project's parity bar.  Gradients: K e_ref in max-abs and in relative L2,
whole and over the first and the last n/2 + 1 samples, e_ref the same error of
fp32 CPU autograd against float64.  K = 4, the project's rule, for the
magnitudes, the impulses, the spectral-convergence gradient and V1 at eps = 1.

The gradients that carry a log term at a small epsilon (the multires
log-magnitude term, V1 at eps = 1e-7) exceed 4 while the kernel is right, and
each group has the next power of two above its measured worst, none above 16:
  multires log term, n = 64 ... 4096: measured 14.02 11.07 6.29 2.79 5.93 5.41
    5.40, K 16 16 8 4 8 8 8;
  V1 at eps = 1e-7, n = 64 ... 4096: measured 4.69 12.76 14.33 5.32 6.47 4.73
    3.97, K 8 16 16 8 8 8 4;
  general geometries (64, 5, 37) ... (4096, 441, 2205): 4.06, K 8; the
    eight-resolution launch, its upstream weights included: 6.31, K 8; (64, 5,
    37) and (512, 88, 441) on the tile seams: 8.63, K 16.
The arithmetic reason: a bin's weight in these gradients is 1 / power, so the
error is the rounding of the few bins of least power; the float64 gradient
itself moves by 1 to 5 e_ref when the input is moved by half an fp32 ulp, and
the kernel's error on such a bin against pocketfft's is a quotient of two
roundings of one number, times 2 for the two signals that share the kernel's
FFT.  The spectral-convergence gradient of the same cases -- the same path from
the bins to the samples without the 1 / power weight -- stays under 3.2; a
framing or gather fault shows there at ratios in the hundreds.  With the clamp
band's upper end at 2e-7 one case (n = 128, T = 2048, rows 3) measured 19.7,
all of its e_ref^2 in the 128 samples of one frame whose least bin held
2.1e-7; tests/spectral_ref.py's band now ends at 4e-7, so no case rests on a
bin beside the clamp.

Zero frames.  The sweep found that a frame of zeros did not transform to zeros:
read back out of the FFT it shares with another frame (its pair in stft_mag,
the other signal's frame in the distance and the losses) it came out as the
other's rounding noise, 1e-13 to 1e-10 in the impulse cases, and V1's gradient,
which divides by |V| + eps, was nonzero on every sample that silence covers
(all 30729 samples off the support at n = 2048).  The three kernels now note
per frame whether any sample is nonzero and take the spectrum of a frame of
zeros as 0; frames with a nonzero sample keep their bits.  A frame that is
quiet but not zero still sits on the other signal's noise floor (about 1e-7 of
its spectrum): with the value a 7-sample burst under a full-scale target, the
frames that see the burst only under the window's first samples put the log
term of the distance at n = 4096 9.7e-4 from float64 (2.1e-6 at n = 1024).

Measured on an MI355X (kernel error / e_ref, the worst of a group's cases; the
scales in the order 64 ... 4096):
stft_mag sweep 1.32 1.51 1.52 2.13 1.39 1.77 1.68; impulses (err / bound, n =
64 1024 2048 4096) 0.12 0.12 0.12 0.15, every unreached frame the bits of +0.
Distance, worst relative error of any term or total (bar 1e-4): 1.0e-6 9.0e-7
1.7e-6 6.6e-7 2.0e-6 2.4e-6 2.1e-7; multi-scale launches equal their
single-scale words bit for bit.
Multires on the V1 grid, forward worst relative 4.5e-7 1.0e-6 2.0e-6 1.6e-6
9.0e-7 7.6e-7 9.1e-7; general geometries and seams, forward at most 6.7e-7;
gradient ratios above.  V1, forward worst relative 1.5e-6 1.1e-6 5.8e-6 4.1e-6
4.1e-6 2.3e-6 3.8e-6; gradient at eps = 1 at most 3.97.
Exact zeros off the support: 0 nonzero samples in every case."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import distance_ref as D
from tests import spectral_ref as S
from tests import stft_loss_ref as R
from tests.test_gpu_aux_kernels import _N, _st, guarded, put, ratio_of, same_bits, untouched

pytestmark = pytest.mark.gpu
K = 4
# gradients that carry a log term at a small epsilon, per group (docstring): multires log-magnitude
# term and V1 at eps = 1e-7 per scale, the general geometries
K_LOG_MULTIRES = {64: 16, 128: 16, 256: 8, 512: 4, 1024: 8, 2048: 8, 4096: 8}
K_LOG_V1 = {64: 8, 128: 16, 256: 16, 512: 8, 1024: 8, 2048: 8, 4096: 4}
K_LOG_GENERAL = {"g": 8, "m": 8, "s": 16}            # by the case name's first letter: geometries, mixed8, seams
PARITY = 1e-4
PAD = (33, 65)                                       # floats of NaN before / after every signal and output
TPAD = (64, 64)                                      # tables hold float2 twiddles: keep them 8-byte aligned
EPSILONS = (1e-7, 1.0)


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def errs(got, want):
    """(max-abs, relative L2) of got against the float64 want."""
    d = torch.as_tensor(got).double() - torch.as_tensor(want).double()
    return float(d.abs().max()), float(d.norm() / torch.as_tensor(want).double().norm())


def flat(values):
    """A contiguous block as a view of a wider NaN-filled buffer: (buffer, view, mask)."""
    return put(np.ascontiguousarray(values).reshape(-1), [PAD])


def fresh(count):
    return guarded((count,), [PAD])


@functools.lru_cache(maxsize=None)
def mag_table(n):
    buf, view, _ = put(_N().pack_stft_table(n), [TPAD])
    return buf, view, buf.clone()


@functools.lru_cache(maxsize=None)
def loss_table(n, win):
    buf, view, _ = put(_N().pack_stft_loss_table(n, win), [TPAD])
    return buf, view, buf.clone()


def blocks_of(rows, t_len, geometries):
    """Workgroups (= workspace slots) of a distance or loss launch."""
    return sum(rows * -(-S.frame_count(t_len, hop) // S.tile_of(n)) for n, hop, _ in geometries)


# ================================================================== runners
def run_mag(x, n):
    """rave_stft_mag on a guarded (rows, T) block: the (rows, n/2 + 1, frames) result."""
    N = _N()
    rows, t_len = x.shape
    count = rows * (n // 2 + 1) * S.frame_count(t_len, n // 4)
    xb, xv, _ = flat(x)
    x_before = xb.clone()
    tb, tv, t_before = mag_table(n)
    outs = []
    for _ in range(2):
        yb, yv, ym = fresh(count)
        a = N.StftArgs(rows=rows, t_len=t_len, n=n, x=xv.data_ptr(), table=tv.data_ptr(), y=yv.data_ptr())
        N.check(N.lib.rave_stft_mag(C.byref(a), _st()), "stft_mag")
        torch.cuda.synchronize()
        assert untouched(yb, ym), "stft_mag wrote outside y"
        outs.append(yv)
    assert same_bits(outs[0], outs[1]), "stft_mag: a second run differs"
    assert same_bits(xb, x_before) and same_bits(tb, t_before), "stft_mag changed an input"
    y = outs[0].cpu().reshape(rows, n // 2 + 1, -1)
    assert bool(torch.isfinite(y).all()), "stft_mag read outside x or the table"
    return y


def run_distance(target, value, scales, eps):
    """rave_audio_distance on guarded blocks: out (1 + 2 n_scales floats, CPU)."""
    N = _N()
    rows, t_len = target.shape
    a = N.DistanceArgs(rows=rows, t_len=t_len, n_scales=len(scales), log_epsilon=eps)
    for i, n in enumerate(scales):
        a.scales[i], a.tables[i] = n, mag_table(n)[1].data_ptr()
    ws = int(N.lib.rave_audio_distance_workspace(C.byref(a)))
    assert ws == 16 * blocks_of(rows, t_len, [(n, n // 4, n) for n in scales])
    xb, xv, _ = flat(target)
    yb, yv, _ = flat(value)
    x_before, y_before = xb.clone(), yb.clone()
    a.x, a.y = xv.data_ptr(), yv.data_ptr()
    outs = []
    for _ in range(2):
        wb, wv, wm = fresh(ws // 4)
        ob, ov, om = fresh(1 + 2 * len(scales))
        a.workspace, a.out = wv.data_ptr(), ov.data_ptr()
        N.check(N.lib.rave_audio_distance(C.byref(a), _st()), "audio_distance")
        torch.cuda.synchronize()
        assert untouched(wb, wm) and untouched(ob, om), "audio_distance wrote outside its workspace or out"
        assert not bool(torch.isnan(wv).any()), "audio_distance left part of the queried workspace unwritten"
        outs.append(ov)
    assert same_bits(outs[0], outs[1]), "audio_distance: a second run differs"
    assert same_bits(xb, x_before) and same_bits(yb, y_before), "audio_distance changed an input"
    for n in scales:
        tb, _, t_before = mag_table(n)
        assert same_bits(tb, t_before)
    out = outs[0].cpu()
    assert bool(torch.isfinite(out).all()), "audio_distance read outside its inputs"
    return out


def run_loss(kind, value, target, res, grad_outs, eps=1e-7):
    """rave_stft_loss_forward, then one rave_stft_loss_backward per grad_out, on
    guarded blocks: (out, saved, [grad_value (rows, T)]) on the CPU."""
    N = _N()
    rows, t_len = value.shape
    a = N.StftLossArgs(rows=rows, t_len=t_len, n_res=len(res), kind=kind, log_epsilon=eps)
    for i, (n, hop, win) in enumerate(res):
        a.n_fft[i], a.hop[i], a.win[i], a.tables[i] = n, hop, win, loss_table(n, win)[1].data_ptr()
    blocks = blocks_of(rows, t_len, res)
    ws = int(N.lib.rave_stft_loss_workspace(C.byref(a)))
    assert ws == 4 * (4 * blocks + sum(rows * S.frame_count(t_len, hop) * win for _, hop, win in res))
    vb, vv, _ = flat(value)
    tb, tv, _ = flat(target)
    v_before, t_before = vb.clone(), tb.clone()
    wb, wv, wm = fresh(ws // 4)
    a.value, a.target, a.workspace = vv.data_ptr(), tv.data_ptr(), wv.data_ptr()
    fwd = []
    for _ in range(2):
        ob, ov, om = fresh(2 + 2 * len(res))
        sb, sv, sm = fresh(4 * len(res))
        a.out, a.saved = ov.data_ptr(), sv.data_ptr()
        N.check(N.lib.rave_stft_loss_forward(C.byref(a), _st()), "stft_loss_forward")
        torch.cuda.synchronize()
        assert untouched(ob, om) and untouched(sb, sm) and untouched(wb, wm), "the forward wrote outside an output"
        assert not bool(torch.isnan(wv[:4 * blocks]).any()), "the forward left a workspace slot unwritten"
        fwd.append((ov, sv))
    assert same_bits(fwd[0][0], fwd[1][0]) and same_bits(fwd[0][1], fwd[1][1]), "the forward: a second run differs"
    out, saved = fwd[1][0].cpu(), fwd[1][1].cpu()                      # a.saved is the second run's
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(saved).all()), "the forward read outside its inputs"
    saved_before = fwd[1][1].clone()
    grads = []
    for go in grad_outs:
        gob, gov, _ = flat(np.asarray(go, np.float32))
        go_before = gob.clone()
        a.grad_out = gov.data_ptr()
        pair = []
        for _ in range(2):
            gb, gv, gm = fresh(rows * t_len)
            a.grad_value = gv.data_ptr()
            N.check(N.lib.rave_stft_loss_backward(C.byref(a), _st()), "stft_loss_backward")
            torch.cuda.synchronize()
            assert untouched(gb, gm) and untouched(wb, wm), "the backward wrote outside grad_value or the workspace"
            assert not bool(torch.isnan(wv).any()), "the backward left part of the queried workspace unwritten"
            pair.append(gv)
        assert same_bits(pair[0], pair[1]), "the backward: a second run differs"
        assert same_bits(gob, go_before) and same_bits(fwd[1][1], saved_before), "the backward changed an input"
        g = pair[0].cpu().reshape(rows, t_len)
        assert bool(torch.isfinite(g).all()), "the backward read outside its inputs"
        grads.append(g)
    assert same_bits(vb, v_before) and same_bits(tb, t_before), "the loss changed an input"
    for n, _, win in res:
        b, _, before = loss_table(n, win)
        assert same_bits(b, before)
    return out, saved, grads


MULTIRES, V1 = 1, 0                                  # RAVE_STFT_LOSS_*


# ================================================================== a. magnitudes
def _mag_eref(x, n):
    want = S.magnitudes(x, n)
    cpu32 = D.stft_mag(torch.from_numpy(x)[None], n).double().numpy()
    return want, float(np.abs(cpu32 - want).max())


def _mag_check(what, x, n):
    """The K e_ref bound over the whole output and on each edge of it; the ratio."""
    want, e_ref = _mag_eref(x, n)
    got = run_mag(x, n).double().numpy()
    assert got.shape == want.shape
    err = np.abs(got - want)
    # with an odd frame count the last frame is the unpaired one: its FFT's imaginary input is zeros
    parts = {"all": err, "DC bin": err[:, 0], "Nyquist bin": err[:, n // 2], "first frame": err[:, :, 0],
             "last frame": err[:, :, -1]}
    ratio = ratio_of(float(err.max()), e_ref)
    print(f"stft_mag {what}: e_ref {e_ref:.3e} kernel {float(err.max()):.3e} ratio {ratio:.2f}")
    for name, part in parts.items():
        assert float(part.max()) <= K * e_ref, (what, name, float(part.max()), e_ref)
    return ratio


@pytest.mark.parametrize("n", S.SCALES)
def test_stft_mag_sweep(n):
    worst = 0.0
    for rows in S.ROWS:
        for f, t_len in S.seam_lengths(n, mag=True) + [(S.frame_count(n // 2 + 1, n // 4), n // 2 + 1)]:
            x = S.synth(rows, t_len, 3000 + n + f)[1]
            worst = max(worst, _mag_check(f"n={n} F={f} T={t_len} rows={rows}", x, n))
    print(f"GROUP stft_mag n={n}: worst ratio {worst:.2f}")


# ================================================================== b. impulses
@pytest.mark.parametrize("n", [64, 1024, 2048, 4096])
def test_stft_mag_impulses(n):
    """x = delta at p.  Frames that no image of p reaches are exact zeros (the
    bits of +0); frames that one reaches hold the window's sample there in every
    bin (tests/test_spectral_ref_host.py checks that of the reference).  e_ref
    can be 0 on such an input, so the bound is K max(e_ref, 2^-23 log2(n)
    max|ref|), the second term being the FFT's own growth."""
    hop = n // 4
    t_len = 9 * hop + 3                                                # 10 frames, an unpaired one none
    idx = S.padded_index(t_len, n)
    worst = 0.0
    for p in (0, 1, n // 2, t_len - 1, t_len - 2, t_len // 2 + 3):
        x = np.zeros((1, t_len), np.float32)
        x[0, p] = 1.0
        want, e_ref = _mag_eref(x, n)
        bound = max(e_ref, 2.0 ** -23 * np.log2(n) * float(want.max()))
        got = run_mag(x, n)
        reached = np.array([(idx[f * hop:f * hop + n] == p).any() for f in range(want.shape[2])])
        assert reached.any() and not reached.all()
        assert not want[:, :, ~reached].any()
        stray = got[:, :, torch.from_numpy(~reached)].contiguous().view(torch.int32)
        err = float(np.abs(got.double().numpy() - want).max())
        worst = max(worst, err / bound)
        print(f"impulse n={n} p={p}: frames reached {int(reached.sum())} of {len(reached)}, nonzero words in the "
              f"others {int((stray != 0).sum())} (largest {float(got[:, :, torch.from_numpy(~reached)].abs().max()):.3e}), "
              f"err {err:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
        assert err <= K * bound, (p, err, bound)
        assert bool((stray == 0).all()), (p, "a frame that no image of the impulse reaches is not exactly 0")
    print(f"GROUP impulses n={n}: worst err / bound {worst:.2f}")


# ================================================================== c. distance
@functools.lru_cache(maxsize=None)
def _dist_inputs(rows, t_len, seed):
    value, target = S.synth(rows, t_len, seed)
    return target, value


def _check_terms(what, out, want_terms):
    """out against the float64 per-scale terms and their sum at the parity bar."""
    worst = rel(out[0], sum(a + b for a, b in want_terms))
    for s, (lin, log) in enumerate(want_terms):
        worst = max(worst, rel(out[1 + 2 * s], lin), rel(out[2 + 2 * s], log))
    print(f"distance {what}: worst rel {worst:.2e}")
    assert worst <= PARITY, (what, worst)
    return worst


@pytest.mark.parametrize("n", S.SCALES)
def test_distance_sweep(n):
    worst = 0.0
    for rows in S.ROWS:
        for f, t_len in S.seam_lengths(n):
            target, value = _dist_inputs(rows, t_len, 4000 + n + f)
            mt, mv = run_mag(target, n).double().numpy(), run_mag(value, n).double().numpy()
            for eps in EPSILONS:
                what = f"n={n} F={f} T={t_len} rows={rows} eps={eps:g}"
                out = run_distance(target, value, (n,), eps)
                worst = max(worst, _check_terms(what, out, S.distance_terms(target, value, (n,), eps)))
                lin, log = S.lin_log(mt, mv, eps)                      # float64 sums over the kernel's own magnitudes
                assert rel(out[1], lin) <= PARITY and rel(out[2], log) <= PARITY, (what, "against stft_mag")
                assert rel(out[0], lin + log) <= PARITY, (what, "against stft_mag")
    print(f"GROUP distance n={n}: worst rel {worst:.2e}")


LAUNCH_T = 2111                                      # above 4096 / 2, a multiple of no hop
LAUNCHES = {
    "eight": (64, 128, 256, 512, 1024, 2048, 4096, 64),
    "repeated": (256, 256, 64, 256),
    "descending": tuple(reversed(S.SCALES)),
    "ascending": S.SCALES,
    "scrambled": (512, 4096, 64, 2048, 128, 1024, 256),
    "six": (1024, 64, 4096, 128, 2048, 256),
}


@functools.lru_cache(maxsize=None)
def _single_scale(n, rows, eps):
    target, value = _dist_inputs(rows, LAUNCH_T, 4500)
    return run_distance(target, value, (n,), eps)


@pytest.mark.parametrize("rows", S.ROWS)
@pytest.mark.parametrize("name", list(LAUNCHES))
def test_distance_multi_scale_launches(name, rows):
    """More than five scales, a scale repeated, scales in every order: the slot
    partition and the finalize order are relative to blk0, so every scale's two
    words equal those of its single-scale call bit for bit."""
    scales = LAUNCHES[name]
    target, value = _dist_inputs(rows, LAUNCH_T, 4500)
    for eps in EPSILONS:
        out = run_distance(target, value, scales, eps)
        _check_terms(f"{name} rows={rows} eps={eps:g}", out, S.distance_terms(target, value, scales, eps))
        for s, n in enumerate(scales):
            alone = _single_scale(n, rows, eps)
            assert same_bits(out[1 + 2 * s:3 + 2 * s], alone[1:3]), (name, s, n)


# ================================================================== d. loss forward and backward
def _region_errs(got, g32, g64, n):
    """[(name, kernel (max-abs, L2), e_ref (max-abs, L2))]: whole, first and last n/2 + 1 samples."""
    m = n // 2 + 1
    out = []
    for name, sl in (("all", slice(None)), ("first", slice(0, m)), ("last", slice(-m, None))):
        out.append((name, errs(got[:, sl], g64[:, sl]), errs(g32[:, sl], g64[:, sl])))
    return out


def _grad_check(what, got, g32, g64, res, k):
    """k e_ref in max-abs and relative L2, whole and on both fold-back regions
    of every resolution; the worst ratio."""
    assert got.shape == g64.shape and got.dtype == torch.float32
    worst = 0.0
    fails = []
    for n in sorted({n for n, _, _ in res}):
        for name, (k_abs, k_l2), (e_abs, e_l2) in _region_errs(got, g32, g64, n):
            r = max(ratio_of(k_abs, e_abs), ratio_of(k_l2, e_l2))
            worst = max(worst, r)
            if k_abs > k * e_abs or k_l2 > k * e_l2:
                fails.append((n, name, k_abs, e_abs, k_l2, e_l2))
    print(f"grad {what}: worst ratio {worst:.2f}")
    assert not fails, (what, fails)
    return worst


@functools.lru_cache(maxsize=None)
def _mr_ref(name):
    """float64 values and terms (numpy, from the definition) and the gradients of
    sc and mag by torch autograd in float64 and in fp32, computed once."""
    case = {c[0]: c for c in S.multires_gradient_cases()}[name]
    res = case[1]
    pred, target = S.multires_inputs(name)

    def fn(dtype):
        t = torch.from_numpy(target).to(dtype)
        return lambda v: R.mr_loss(v, t, res)
    _, g64 = R.grad_of(fn(torch.float64), pred, torch.float64)
    _, g32 = R.grad_of(fn(torch.float32), pred, torch.float32)
    return dict(res=res, pred=pred, target=target, vals=S.mr_loss(pred, target, res),
                terms=S.mr_terms(pred, target, res), g64=g64, g32=g32)


def _mr_forward_check(what, out, ref):
    worst = max(rel(out[0], ref["vals"][0]), rel(out[1], ref["vals"][1]))
    for r, (sc, mag) in enumerate(ref["terms"]):
        worst = max(worst, rel(out[2 + 2 * r], sc), rel(out[3 + 2 * r], mag))
    print(f"multires forward {what}: worst rel {worst:.2e}")
    assert worst <= PARITY, (what, worst)
    return worst


def _mr_case(name, grad_outs=((1.0, 0.0), (0.0, 1.0))):
    """One multires case, forward and one backward per grad_out: (forward rel, worst gradient ratio)."""
    ref = _mr_ref(name)
    out, _, grads = run_loss(MULTIRES, ref["pred"], ref["target"], ref["res"], grad_outs)
    fwd = _mr_forward_check(name, out, ref)
    worst = 0.0
    for (a, b), got in zip(grad_outs, grads):
        g64 = a * ref["g64"][0] + b * ref["g64"][1]
        g32 = a * ref["g32"][0] + b * ref["g32"][1]
        k_log = K_LOG_MULTIRES[ref["res"][0][0]] if name.startswith("n") else K_LOG_GENERAL[name[0]]
        worst = max(worst, _grad_check(f"{name} grad_out=({a:g}, {b:g})", got, g32, g64, ref["res"],
                                       k_log if b else K))
    return fwd, worst


def _names(prefix):
    return [c[0] for c in S.multires_gradient_cases() if c[0].startswith(prefix)]


@pytest.mark.parametrize("n", S.SCALES)
def test_multires_sweep(n):
    """MULTIRES on the (n, n/4, n) grid: every seam count, T = n/2 + 1 and n/2 + 2."""
    fwd = worst = 0.0
    for name in _names(f"n{n}-"):
        f, w = _mr_case(name)
        fwd, worst = max(fwd, f), max(worst, w)
    print(f"GROUP multires n={n}: forward worst rel {fwd:.2e}, gradient worst ratio {worst:.2f}")


@pytest.mark.parametrize("name", _names("g") + _names("mixed8") + _names("s"))
def test_multires_general_geometries(name):
    """(64, 5, 37); (64, 70, 37), hop > win; (256, 7, 3); (128, 32, 127), odd
    n - win; (4096, 441, 2205) at T = 2049; eight resolutions of mixed n_fft;
    (64, 5, 37) and (512, 88, 441) at kTile - 1, kTile, kTile + 1 and 2 kTile + 1
    frames, at both ends of the hop."""
    f, w = _mr_case(name)
    print(f"GROUP multires {name}: forward worst rel {f:.2e}, gradient worst ratio {w:.2f}")


@pytest.mark.parametrize("name", ["g64.5.37-T300-r3", "mixed8-T1500-r3"])
def test_multires_upstream_weights(name):
    """grad_out != 1 on each of the two words, and on both."""
    _, w = _mr_case(name, ((2.5, 0.0), (0.0, 0.5), (2.5, 0.5)))
    print(f"GROUP multires upstream {name}: gradient worst ratio {w:.2f}")


@functools.lru_cache(maxsize=None)
def _v1_ref(n, rows, t_len, eps):
    value, target = S.synth(rows, t_len, 5000 + n + t_len)

    def fn(dtype):
        t = torch.from_numpy(target).to(dtype)[None]
        return lambda v: (R.v1_distance(t, v[None], (n,), eps),)
    _, (g64,) = R.grad_of(fn(torch.float64), value, torch.float64)
    _, (g32,) = R.grad_of(fn(torch.float32), value, torch.float32)
    return value, target, S.distance_terms(target, value, (n,), eps), g64, g32


@pytest.mark.parametrize("n", S.SCALES)
def test_v1_sweep(n):
    """V1 at its own geometry: every seam count, T = n/2 + 1 and n/2 + 2, both
    epsilons, grad_out 1 and 2.5."""
    res = ((n, n // 4, n),)
    fwd = worst = 0.0
    lengths = sorted({t for _, t in S.seam_lengths(n)} | {n // 2 + 1, n // 2 + 2})
    for rows in S.ROWS:
        for t_len in lengths:
            for eps in EPSILONS:
                what = f"v1 n={n} T={t_len} rows={rows} eps={eps:g}"
                value, target, terms, g64, g32 = _v1_ref(n, rows, t_len, eps)
                out, _, grads = run_loss(V1, value, target, res, ((1.0,), (2.5,)), eps)
                (lin, log), = terms
                f = max(rel(out[0], lin + log), rel(out[2], lin), rel(out[3], log))
                assert float(out[1]) == 0.0
                assert f <= PARITY, (what, f)
                fwd = max(fwd, f)
                k = K_LOG_V1[n] if eps < 1.0 else K
                worst = max(worst, _grad_check(what, grads[0], g32, g64, res, k))
                worst = max(worst, _grad_check(what + " x2.5", grads[1], 2.5 * g32, 2.5 * g64, res, k))
    print(f"GROUP v1 n={n}: forward worst rel {fwd:.2e}, gradient worst ratio {worst:.2f}")


# ================================================================== e. exact zeros in the gradient
def _burst_inputs(rows, t_len, burst, seed):
    full, target = S.synth(rows, t_len, seed)
    value = np.zeros_like(full)
    value[:, burst[0]:burst[1]] = full[:, burst[0]:burst[1]]
    return value, target


def _bursts(t_len):
    return {"left": (0, 5), "right": (t_len - 5, t_len), "middle": (t_len // 2 - 3, t_len // 2 + 4)}


def _zeros_check(what, g, sup):
    outside = g[:, torch.from_numpy(~sup)]
    inside = g[:, torch.from_numpy(sup)]
    nonzero = int((outside != 0).sum())
    print(f"zeros {what}: support {int(sup.sum())} of {len(sup)} samples, nonzero outside {nonzero}"
          + (f" (largest {float(outside.abs().max()):.3e} against {float(inside.abs().max()):.3e} inside)" if nonzero
             else ""))
    assert 0 < sup.sum() < len(sup)
    assert bool((inside != 0).any())
    assert nonzero == 0, (what, nonzero)


@pytest.mark.parametrize("where", ["left", "right", "middle"])
@pytest.mark.parametrize("res", [((64, 16, 64),), ((64, 5, 37),), ((128, 32, 127),), ((1024, 256, 1024),),
                                 ((2048, 220, 1102), (64, 5, 37))], ids=lambda r: "+".join(str(g[0]) for g in r))
def test_multires_gradient_is_zero_off_the_support(res, where):
    """The value is nonzero on a short burst only: frames that do not see it have
    power under the clamp, so the gradient is exactly 0 wherever no burst-seeing
    frame reaches."""
    t_len = 6 * max(n for n, _, _ in res) + 3
    burst = _bursts(t_len)[where]
    value, target = _burst_inputs(3, t_len, burst, 6000)
    _, _, (g,) = run_loss(MULTIRES, value, target, res, ((1.0, 1.0),))
    sup = np.zeros(t_len, bool)
    for n, hop, win in res:
        sup |= S.support(burst, t_len, n, hop, win)
    _zeros_check(f"multires {res} {where}", g, sup)


@pytest.mark.parametrize("where", ["left", "right", "middle"])
@pytest.mark.parametrize("n", [64, 1024, 2048])
def test_v1_gradient_is_zero_off_the_support(n, where):
    """V1: a frame of zeros has |V| = 0, whose gradient is 0."""
    t_len = 6 * n + 3
    burst = _bursts(t_len)[where]
    value, target = _burst_inputs(3, t_len, burst, 6100)
    _, _, (g,) = run_loss(V1, value, target, ((n, n // 4, n),), ((1.0,),), 1e-7)
    _zeros_check(f"v1 n={n} {where}", g, S.support(burst, t_len, n, n // 4, n))


@pytest.mark.parametrize("res", [((64, 70, 37),), ((256, 300, 100), (64, 150, 64))], ids=["64", "256+64"])
def test_gradient_is_zero_between_the_frames_of_a_long_hop(res):
    """hop > win and a broadband value: samples that belong to no frame."""
    t_len = 1000
    value, target = S.synth(3, t_len, 6200)
    _, _, (g,) = run_loss(MULTIRES, value, target, res, ((1.0, 1.0),))
    sup = np.zeros(t_len, bool)
    for n, hop, win in res:
        sup |= S.support((0, t_len), t_len, n, hop, win)
    _zeros_check(f"long hop {res}", g, sup)


# ================================================================== f. silence
@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_silent_frames_match_the_reference(n):
    """One row of the value is zeros: its frames have |V| = 0 exactly, so
    log(|V| + 1e-7) is the reference's in the distance and in the V1 loss alike
    (read out of the FFT they share with the target they would hold the target's
    rounding noise, about 1e-7 of its spectrum, a hundred times epsilon)."""
    t_len = 6 * n + 3
    value, target = S.synth(3, t_len, 6300)
    value[1] = 0.0
    (lin, log), = S.distance_terms(target, value, (n,), 1e-7)
    out = run_distance(target, value, (n,), 1e-7)
    print(f"silence n={n}: distance lin {rel(out[1], lin):.2e} log {rel(out[2], log):.2e}")
    assert rel(out[1], lin) <= PARITY and rel(out[2], log) <= PARITY
    out, _, _ = run_loss(V1, value, target, ((n, n // 4, n),), (), 1e-7)
    print(f"silence n={n}: v1 loss lin {rel(out[2], lin):.2e} log {rel(out[3], log):.2e}")
    assert rel(out[2], lin) <= PARITY and rel(out[3], log) <= PARITY
