"""The small kernels at their edges (rave_amd/csrc/misc.hip, noise.hip,
adain.hip, speaker.hip), called through rave_amd._native at the C boundary,
against the restatements of tests/aux_ref.py (which tests/test_aux_ref_host.py
checks against the oracle and torch on the CPU).

Every output buffer is filled with NaN (or a sentinel) and is larger than what
the kernel may write; every test checks that the surroundings are untouched and
that the inputs are unchanged.  Inputs are strided views of wider NaN-filled
buffers, so an over-read shows in the result.

Bounds: 4 e_ref, e_ref the max-abs error over the case's output of the fp32 CPU
run of the restatement against its float64 run on the same input (the rule of
the pitch and spectrogram tests).  Exact operations (copy, fill, shift,
max-pool, the RVQ indices with a margin, the decode sum in layer order, the
uniform draw with lo = 0, hi = 1) are compared bitwise.

Measured on an MI355X (kernel error / e_ref, the worst of a group's cases):
AdaIN over the modes, rows and aliasings of one t_len, y / updated statistics:
T=2 2.37 / 1.14, 63 1.13 / 1.48, 64 1.24 / 2.05, 255 1.14 / 1.42, 256 1.05 /
1.48, 257 0.98 / 1.35, 1000 1.12 / 2.03; the DC-offset row's std 0.57.
Noise filter, frames 1 / 127 / 128 / 129: (5, 8) 0.79 0.73 0.90 0.95, (5, 16)
1.00 0.71 0.72 1.03, (9, 16) 0.71 1.00 0.63 0.98.
row_stats, T = 2 255 256 257 700: none 1.00 1.72 1.00 0.46 0.56, leaky 1.00
0.92 0.59 0.49 1.00; attn_pool (__expf and all): none 0.72 0.71 1.28 0.74 0.97,
leaky 0.90 1.56 0.75 0.44 1.00; logits +-80 0.73; the DC row 0.67 (e_ref
1.5e-4: the one-pass formula loses the digits in either arithmetic).
linear, n_in = 1 63 64 65 200: n_out 1 1.00 1.00 0.64 1.00 0.22, n_out 5 1.00
1.00 1.32 0.65 0.61.
RVQ: ties D=128 / 64 (float64 margins 102.4 / 41.7) 0 of 180 indices differ;
k40, k65, strided: 0 differ, 0 excused (the float64 run alone: 0 low gaps).
Uniform, 2^20 draws: mean - 0.5 = -5.9e-5 (5 sigma 1.4e-3), var - 1/12 =
2.8e-6 (5 sigma 3.6e-4), most repeats 4 (cap 8).  Engine schedule: max |xcorr|
0.0120 / 0.0117 against the bound 0.0234, 0 lag-1 equalities (cap 1.38); before
the seed was hashed: 1.0000 and 65535 of 65535.
Model level, max |xcorr| of consecutive noise residuals over lags -64..64:
one-shot decode device-drawn 0.0279 against host-drawn 0.0341 (ratio 0.82; 0.3539,
ratio 10.4, before the seed was hashed); streaming blocks 0.0289 against 0.0343
(0.84; 0.3502, ratio 10.2, before)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import aux_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _N():
    from rave_amd import _native as N
    return N


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def guarded(shape, pads, fill=NAN, dtype=torch.float32):
    """A buffer of ``fill`` wider than ``shape`` by pads [(before, after), ...];
    returns (buffer, the view of ``shape`` inside it, the mask of the rest)."""
    full = [lo + s + hi for s, (lo, hi) in zip(shape, pads)]
    buf = torch.full(full, fill, dtype=dtype, device=DEV)
    sl = tuple(slice(lo, lo + s) for s, (lo, hi) in zip(shape, pads))
    mask = torch.ones(full, dtype=torch.bool, device=DEV)
    mask[sl] = False
    return buf, buf[sl], mask


def put(values, pads):
    """``values`` (numpy or CPU tensor) as a strided view of a NaN-filled buffer."""
    v = torch.as_tensor(values)
    buf, view, mask = guarded(tuple(v.shape), pads, NAN if v.dtype.is_floating_point else -(1 << 40), v.dtype)
    view.copy_(v)
    return buf, view, mask


def untouched(buf, mask, fill=NAN):
    rest = buf[mask]
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def refused(call, exc, text):
    """The call is refused before any launch: the exception and rave_last_error
    both name the cause."""
    N = _N()
    with pytest.raises(exc) as info:
        N.check(call())
    last = N.lib.rave_last_error().decode()
    assert text in str(info.value) and text in last, (str(info.value), last)


def ratio_of(err, e_ref):
    return err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))


def report(what, err, e_ref):
    ratio = ratio_of(err, e_ref)
    print(f"{what}: e_ref {e_ref:.3e} kernel {err:.3e} ratio {ratio:.2f}")
    return ratio


def maxerr(got, want64):
    return float((torch.as_tensor(got).double().cpu() - torch.as_tensor(want64).double()).abs().max())


# ================================================================== 1. uniform draw
def _draw(n, seed, lo=0.0, hi=1.0, guard=64):
    N = _N()
    y = torch.full((n + 2 * guard,), NAN, device=DEV)
    N.check(N.lib.rave_fill_uniform(y.data_ptr() + 4 * guard, n, seed, lo, hi, _st()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[:guard]).all()) and bool(torch.isnan(y[guard + n:]).all())
    return y[guard:guard + n].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _long_draw():
    return _draw(600_001, 0x5EED)               # above 2048 x 256: the grid-stride loop wraps


def test_uniform_bitwise_and_geometry_free():
    short = _draw(1000, 0x5EED)
    assert np.array_equal(short.view(np.uint32), R.uniform(0x5EED, 1000).view(np.uint32))
    long = _long_draw()
    assert np.array_equal(long.view(np.uint32), R.uniform(0x5EED, 600_001).view(np.uint32))
    assert np.array_equal(long[:1000].view(np.uint32), short.view(np.uint32))
    assert short[:3].tolist() == [0.07230788469314575, 0.7454074621200562, 0.6282155513763428]
    assert _draw(3, 0).tolist() == [0.6524484753608704, 0.7012121081352234, 0.38712412118911743]
    big = (1 << 64) - 16                         # a seed above 2^63 passes the C boundary whole
    assert np.array_equal(_draw(100, big).view(np.uint32), R.uniform(big, 100).view(np.uint32))


@pytest.mark.parametrize("lo,hi", [(-1.0, 1.0), (0.25, 0.75)])
def test_uniform_ranges_within_one_ulp(lo, hi):
    got, want = _draw(1000, 11, lo, hi), R.uniform(11, 1000, lo, hi)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert bool((np.abs(got.astype(np.float64) - want) <= ulp).all())       # lo + scale u may be one fma
    assert got.min() >= lo and got.max() < hi


def test_uniform_empty_draw_writes_nothing():
    N = _N()
    assert _draw(0, 5).size == 0
    assert N.lib.rave_fill_uniform(None, 0, 5, 0.0, 1.0, _st()) == N.RAVE_ERR_ARG


def test_uniform_moments_and_repeats():
    """2^20 draws: the mean and variance within 5 sigma of U[0,1)'s (sigma of the
    sample mean 0.28868 / 1024, of the sample variance sqrt(1/180) / 1024), and
    no value more often than 24-bit draws allow: the expected number of values
    seen k times is at most n (n / 2^24)^(k-1) / k!, which at n = 2^20 is 9.5e-8
    for k = 8 and 6.6e-10 for k = 9, so 8 is the cap (aux_ref.repeat_cap)."""
    u = _draw(1 << 20, 7)
    assert u.min() >= 0 and u.max() < 1
    mean, var = float(u.mean(dtype=np.float64)), float(u.var(dtype=np.float64))
    most = int(np.unique(u, return_counts=True)[1].max())
    print(f"uniform 2^20: mean - 0.5 = {mean - 0.5:.3e}, var - 1/12 = {var - 1 / 12:.3e}, most repeats {most}")
    assert abs(mean - 0.5) < 5 * 0.28868 / 1024
    assert abs(var - 1 / 12) < 5 * np.sqrt(1 / 180) / 1024
    assert most <= R.repeat_cap(1 << 20) == 8


@pytest.mark.parametrize("base", R.ENGINE_BASES)
def test_uniform_engine_schedule_is_independent(base):
    """Consecutive calls of the engine's seed schedule (base + G c): no lag in
    -8..8 correlates above 6 / sqrt(n) (independent draws: sigma 1 / sqrt(n); a
    shifted copy: 1.0), and call c + 1 equals call c moved by one element at no
    more positions than 24-bit draws collide by chance."""
    n = 65536
    worst, worst_eq = 0.0, 0
    for c in range(1, 5):
        a = _draw(n, R.engine_seed(base, c))
        b = _draw(n, R.engine_seed(base, c + 1))
        worst = max(worst, float(np.abs(R.xcorr(a, b, 8)).max()))
        worst_eq = max(worst_eq, int((b[:-1] == a[1:]).sum()), int((a[:-1] == b[1:]).sum()))
    p = n * 2.0 ** -24
    print(f"engine schedule base {base:#x}: max |xcorr| {worst:.4f} (bound {6 / np.sqrt(n):.4f}), "
          f"lag-1 equal positions {worst_eq} (cap {p + 6 * np.sqrt(p) + 1:.2f})")
    assert worst < 6 / np.sqrt(n)
    assert worst_eq <= p + 6 * np.sqrt(p) + 1


# ------------------------------------------------------------------ model level
def _peak(ra, rb):
    """Max |normalised cross-correlation| over lags -64..64 and the batch rows."""
    return max(float(np.abs(R.xcorr(a, b, 64)).max()) for a, b in zip(ra.reshape(len(ra), -1), rb.reshape(len(rb), -1)))


def _noise_model(causal):
    from rave_amd import config as rcfg
    from rave_amd.model import RAVE
    from rave_amd.weights import init_params, init_speaker
    cfg = rcfg.v3_noise(capacity=8, causal=causal)
    return cfg, RAVE(cfg, init_params(cfg, 1), init_speaker(cfg, 1), device=DEV)


def _pairs(res):
    return [_peak(a, b) for a, b in zip(res[:-1], res[1:])]


def test_model_device_noise_is_fresh_every_call():
    """The noise branch of four decodes of one z with device-drawn noise, as
    residuals against the zero-noise decode (u = 0.5): consecutive residuals
    correlate no more than 3x what eight pairs of host-drawn independent noise
    do through the same decode (filtered noise: a small-sample spread of about
    2x is expected)."""
    cfg, m = _noise_model(False)
    B, Fz = 2, 16
    z = torch.randn(B, cfg.dec_in, Fz, generator=torch.Generator().manual_seed(6)).to(DEV)
    shape = m.noise_shape(B, Fz)
    zero = m.decode(z, torch.full(shape, 0.5, device=DEV)).cpu().numpy().astype(np.float64)
    dev = [m.decode(z).cpu().numpy() - zero for _ in range(4)]
    rng = np.random.default_rng(12)
    host = [m.decode(z, torch.from_numpy(rng.uniform(0, 1, shape).astype(np.float32)).to(DEV)).cpu().numpy() - zero
            for _ in range(9)]
    d, h = max(_pairs(dev)), max(_pairs(host))
    print(f"model noise residuals: rms {np.sqrt((dev[0] ** 2).mean()):.3e}; device pairs max |xcorr| {d:.4f}, "
          f"host pairs {h:.4f}, ratio {d / h:.2f}")
    assert np.sqrt((dev[0] ** 2).mean()) > 0
    assert d <= 3 * h


def test_streaming_device_noise_is_fresh_every_block():
    """The same through StreamingRAVE: four consecutive blocks with device-drawn
    noise against a zero-noise stream fed the same latents; the reference level
    from a stream fed host-drawn independent noise (nine blocks, eight pairs)."""
    from rave_amd.streaming import StreamingRAVE
    cfg, m = _noise_model(True)
    B, Fz = 2, 16
    block = Fz * cfg.hop
    s_dev, s_zero, s_host = (StreamingRAVE(m, batch=B, block=block, direction="decode") for _ in range(3))
    shape = m.noise_shape(B, Fz)
    gen = torch.Generator().manual_seed(8)
    rng = np.random.default_rng(13)
    half = torch.full(shape, 0.5, device=DEV)
    dev, host = [], []
    for i in range(9):
        z = torch.randn(B, cfg.dec_in, Fz, generator=gen).to(DEV)
        zero = s_zero.decode(z, noise_u=half).cpu().numpy().astype(np.float64)
        u = torch.from_numpy(rng.uniform(0, 1, shape).astype(np.float32)).to(DEV)
        host.append(s_host.decode(z, noise_u=u).cpu().numpy() - zero)
        if i < 4:
            dev.append(s_dev.decode(z).cpu().numpy() - zero)
    d, h = max(_pairs(dev)), max(_pairs(host))
    print(f"streaming noise residuals: device pairs max |xcorr| {d:.4f}, host pairs {h:.4f}, ratio {d / h:.2f}")
    assert d <= 3 * h


# ================================================================== 2. RVQ
def _rvq_args(cb, B, T, z=None, idx=None, y=None):
    N = _N()
    nq, K, D = cb.shape
    a = N.RvqArgs(n_q=nq, codebook_size=K, dim=D, batch=B, t_len=T, codebooks=cb.data_ptr())
    if z is not None:
        assert z.stride(2) == 1
        a.z, a.z_sb, a.z_sc = z.data_ptr(), z.stride(0), z.stride(1)
    if idx is not None:
        assert idx.stride(2) == 1
        a.idx, a.i_sb, a.i_sq = idx.data_ptr(), idx.stride(0), idx.stride(1)
    if y is not None:
        assert y.stride(2) == 1
        a.y, a.y_sb, a.y_sc = y.data_ptr(), y.stride(0), y.stride(1)
    return a


def _encode(z_np, cbs, strided=False):
    """Indices of the kernel for z (B, D, T), with guard bands round idx and the
    scratch, inputs checked unchanged."""
    N = _N()
    B, D, T = z_np.shape
    nq = cbs.shape[0]
    cb = torch.from_numpy(cbs).to(DEV)
    zbuf, z, _ = put(z_np, [(0, 0), (3, 4), (2, 3)] if strided else [(0, 0), (0, 0), (0, 0)])
    ibuf, idx, imask = guarded((B, nq, T), [(0, 0), (1, 1), (2, 3)] if strided else [(0, 1), (0, 0), (0, 0)],
                               fill=-1, dtype=torch.int64)
    a = _rvq_args(cb, B, T, z=z, idx=idx)
    n_work = int(N.lib.rave_rvq_workspace(C.byref(a)))
    work = torch.full((n_work + 64,), NAN, device=DEV)
    a.work = work.data_ptr()
    z0, cb0 = zbuf.clone(), cb.clone()
    N.check(N.lib.rave_rvq_encode(C.byref(a), _st()))
    torch.cuda.synchronize()
    assert untouched(ibuf, imask, -1) and bool(torch.isnan(work[n_work:]).all())
    assert same_bits(zbuf, z0) and same_bits(cb, cb0)
    return idx.cpu().numpy()


@pytest.mark.parametrize("D", [128, 64])
def test_rvq_encode_exact_ties_take_the_smaller_index(D):
    """Bitwise duplicated codewords (aux_ref.TIE_PAIRS: across accumulator rows,
    lane halves, waves, splits and into the ragged last split) that win each
    layer by a float64 margin above 1.0 (fp32 error ~1e-4): the index is the
    smaller one of the pair, in both layers."""
    z, cbs, pair_of, want = R.rvq_tie_case(D)
    _, margin = R.rvq_pair_margin(z, cbs, pair_of)
    assert margin.min() > 1.0
    got = _encode(z, cbs)
    wrong = got != want
    print(f"rvq ties D={D}: margin {margin.min():.1f}, {int(wrong.sum())} of {want.size} indices differ")
    assert not wrong.any(), (got[wrong], want[wrong])


def test_rvq_zero_codebooks_give_index_zero_and_decode_zero():
    N = _N()
    rng = np.random.default_rng(1)
    B, D, T, K, nq = 2, 128, 45, 200, 3
    cbs = np.zeros((nq, K, D), np.float32)
    got = _encode(rng.standard_normal((B, D, T)).astype(np.float32), cbs)
    assert not got.any()
    cb = torch.from_numpy(cbs).to(DEV)
    idx = torch.from_numpy(got).to(DEV)
    ybuf, y, ymask = guarded((B, D, T), [(0, 0), (1, 2), (0, 3)])
    N.check(N.lib.rave_rvq_decode(C.byref(_rvq_args(cb, B, T, idx=idx, y=y)), _st()))
    torch.cuda.synchronize()
    assert same_bits(y, torch.zeros_like(y)) and untouched(ybuf, ymask)


@pytest.mark.parametrize("name", list(R.RVQ_CASES))
def test_rvq_encode_small_and_strided_vs_float64(name):
    """K below one split (40), one code into the second split (65), and a z that
    is a channel slice of a wider buffer with a strided idx: the float64 argmin
    wherever its top-2 gap is at least 1e-3 (_rvq_encode_np's rule), at most 1 %
    of the frames excused."""
    from tests.test_gpu_parity import _rvq_encode_np
    z, cbs = R.rvq_case(name)
    got = _encode(z, cbs, strided=name == "strided")
    ref, gap = _rvq_encode_np(z, cbs)
    assert np.array_equal(ref, R.rvq_encode(z, cbs)[0])
    assert got.min() >= 0 and got.max() < cbs.shape[1]
    mism = got != ref
    excused = gap < R.GAP_RULE
    print(f"rvq case {name}: {int(mism.sum())} of {ref.size} differ, {int(excused.sum())} excused")
    assert excused.sum() <= R.EXCUSED_CAP * ref.size
    assert (gap[mism] < R.GAP_RULE).all()


def test_rvq_decode_clamps_wraps_and_sums_in_layer_order():
    """D T = 268800 > 1024 x 256 (the grid-stride loop wraps), strided y and idx,
    indices -5 and K + 3 among them: bitwise the fp32 numpy sum in layer order."""
    N = _N()
    rng = np.random.default_rng(2)
    B, D, T, K, nq = 2, 128, 2100, 65, 3
    cbs = rng.standard_normal((nq, K, D)).astype(np.float32)
    idx_np = rng.integers(0, K, (B, nq, T))
    idx_np[:, :, ::7] = -5
    idx_np[:, :, 3::11] = K + 3
    idx_np[0, 1, -1], idx_np[1, 2, 0] = -5, K + 3
    cb = torch.from_numpy(cbs).to(DEV)
    ibuf, idx, _ = put(idx_np, [(0, 0), (1, 1), (2, 3)])
    ybuf, y, ymask = guarded((B, D, T), [(0, 0), (2, 1), (1, 5)])
    i0 = ibuf.clone()
    N.check(N.lib.rave_rvq_decode(C.byref(_rvq_args(cb, B, T, idx=idx, y=y)), _st()))
    torch.cuda.synchronize()
    assert same_bits(y.cpu(), torch.from_numpy(R.rvq_decode(idx_np, cbs)))
    assert untouched(ybuf, ymask) and torch.equal(ibuf, i0)


def test_rvq_encode_refuses_other_dims():
    N = _N()
    cb = torch.zeros(1, 8, 96, device=DEV)
    z = torch.zeros(1, 96, 4, device=DEV)
    idx = torch.full((1, 1, 4), -1, dtype=torch.int64, device=DEV)
    a = _rvq_args(cb, 1, 4, z=z, idx=idx)
    work = torch.zeros(int(N.lib.rave_rvq_workspace(C.byref(a))), device=DEV)
    a.work = work.data_ptr()
    refused(lambda: N.lib.rave_rvq_encode(C.byref(a), _st()), NotImplementedError, "dim must be 64 or 128")
    torch.cuda.synchronize()
    assert bool((idx == -1).all())


# ================================================================== 3. AdaIN
ADA_C, ADA_B, ADA_MB = 5, 3, 8


def _adain_call(x, y, stats, counters, ticket, mode, row0, max_batch=ADA_MB):
    N = _N()
    B, Cc, T = x.shape
    a = N.AdainArgs(batch=B, channels=Cc, t_len=T, mode=mode, max_batch=max_batch, row0=row0,
                    x=x.data_ptr(), x_sb=x.stride(0), x_sc=x.stride(1),
                    y=y.data_ptr(), y_sb=y.stride(0), y_sc=y.stride(1),
                    stats=stats.data_ptr(), counters=counters.data_ptr(),
                    ticket=0 if ticket is None else ticket.data_ptr())
    return N.lib.rave_adain(C.byref(a), _st())


@pytest.mark.parametrize("t_len", [2, 63, 64, 255, 256, 257, 1000])
def test_adain_modes_rows_and_aliasing(t_len):
    """Modes 0 / 2 / 1 / 0 / 1 / 2 in sequence from the reference's fresh
    buffers, at row0 0 and 4, with y aliased to x and as a separate strided
    buffer: y and the updated rows within 4 e_ref of the float64 restatement
    run from the same fp32 state; every other row and the other statistic's two
    planes bitwise unchanged; the counter bumped once and the ticket back at 0."""
    N = _N()
    rng = np.random.default_rng(t_len)
    worst_y = worst_s = 0.0
    for row0 in (0, 4):
        for alias in (True, False):
            stats = torch.zeros(4, ADA_MB, ADA_C, device=DEV)
            stats[1] = stats[3] = 1.0
            counters = torch.zeros(2, device=DEV)
            ticket = torch.zeros(4, dtype=torch.int32, device=DEV)
            for step, mode in enumerate((0, 2, 1, 0, 1, 2)):
                x_np = (rng.standard_normal((ADA_B, ADA_C, t_len)) * 1.7 + 0.3).astype(np.float32)
                xbuf, x, _ = put(x_np, [(0, 1), (1, 2), (3, 2)])
                if alias:
                    ybuf, y, ymask = xbuf, x, None
                else:
                    ybuf, y, ymask = guarded(x_np.shape, [(1, 0), (0, 3), (2, 5)])
                x0, s0, c0 = xbuf.clone(), stats.cpu(), counters.cpu().tolist()
                N.check(_adain_call(x, y, stats, counters, ticket, mode, row0))
                torch.cuda.synchronize()
                xt = torch.from_numpy(x_np)
                y64, s64, c64 = R.adain(xt.double(), s0.double(), c0, mode, row0)
                y32, s32, _ = R.adain(xt, s0, c0, mode, row0)
                assert counters.cpu().tolist() == c64 and not ticket.any()
                s1 = stats.cpu()
                rows = slice(row0, row0 + ADA_B)
                if mode == 0:
                    assert same_bits(s1, s0)
                else:
                    o = 0 if mode == 1 else 2
                    keep = s0.clone()
                    keep[o:o + 2, rows] = s1[o:o + 2, rows]
                    assert same_bits(s1, keep)                      # only this statistic's rows moved
                    e_ref = float((s32[o:o + 2, rows].double() - s64[o:o + 2, rows]).abs().max())
                    err = maxerr(s1[o:o + 2, rows], s64[o:o + 2, rows])
                    worst_s = max(worst_s, ratio_of(err, e_ref))
                    assert err <= 4 * e_ref, (row0, alias, step, mode, err, e_ref)
                transfer = mode != 2 and c64[0] != 0 and c64[1] != 0
                if transfer:
                    e_ref = float((y32.double() - y64).abs().max())
                    err = maxerr(y, y64)
                    worst_y = max(worst_y, ratio_of(err, e_ref))
                    assert err <= 4 * e_ref, (row0, alias, step, mode, err, e_ref)
                else:
                    assert same_bits(y.cpu(), xt)                  # pass-through is a copy
                if alias:
                    if not transfer:
                        assert same_bits(xbuf, x0)
                    else:
                        keep = x0.clone()
                        keep[:ADA_B, 1:1 + ADA_C, 3:3 + t_len] = x
                        assert same_bits(xbuf, keep)
                else:
                    assert same_bits(xbuf, x0) and untouched(ybuf, ymask)
    print(f"adain T={t_len}: worst ratio y {worst_y:.2f}, stats {worst_s:.2f}")


@pytest.mark.parametrize("Cc,B", [(ADA_C, ADA_B), (512, 8)])
def test_adain_counter_bumped_once_per_call(Cc, B):
    """Six alternating learn calls; 512 x 8 is 4096 workgroups, more than are
    resident at once, so the last-arrival ticket is taken across waves of them."""
    N = _N()
    x = torch.randn(B, Cc, 64, generator=torch.Generator().manual_seed(0)).to(DEV)
    y = torch.empty_like(x)
    stats = torch.zeros(4, B, Cc, device=DEV)
    counters = torch.zeros(2, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i in range(6):
        N.check(_adain_call(x, y, stats, counters, ticket, 1 + i % 2, 0, max_batch=B))
        torch.cuda.synchronize()
        assert counters.cpu().tolist() == [(i + 2) // 2, (i + 1) // 2] and int(ticket[0]) == 0
    mean = x.double().mean(-1).cpu()
    assert maxerr(stats[0], mean) < 1e-5 and maxerr(stats[2], mean) < 1e-5      # every row was updated each time


def test_adain_transfer_with_a_zero_counter_is_a_copy():
    N = _N()
    rng = np.random.default_rng(5)
    x_np = rng.standard_normal((ADA_B, ADA_C, 100)).astype(np.float32)
    stats = torch.from_numpy(rng.standard_normal((4, ADA_MB, ADA_C)).astype(np.float32)).to(DEV)
    s0 = stats.clone()
    for cnt in ([0.0, 2.0], [3.0, 0.0], [0.0, 0.0]):
        counters = torch.tensor(cnt, device=DEV)
        xbuf, x, _ = put(x_np, [(0, 0), (0, 1), (0, 4)])
        x0 = xbuf.clone()
        N.check(_adain_call(x, x, stats, counters, None, 0, 0))                 # y == x: nothing to write
        ybuf, y, ymask = guarded(x_np.shape, [(0, 0), (1, 1), (2, 2)])
        N.check(_adain_call(x, y, stats, counters, None, 0, 2))
        torch.cuda.synchronize()
        assert same_bits(xbuf, x0) and same_bits(y, x) and untouched(ybuf, ymask)
        assert same_bits(stats, s0) and counters.cpu().tolist() == cnt


def test_adain_dc_offset_row_keeps_its_std():
    """x = 100 + 0.01 N(0, 1): a one-pass variance (E x^2 - mean^2) loses the
    std entirely in fp32; the two-pass one keeps it within 4 e_ref."""
    N = _N()
    rng = np.random.default_rng(6)
    x_np = (100 + 0.01 * rng.standard_normal((ADA_B, ADA_C, 1000))).astype(np.float32)
    x = torch.from_numpy(x_np).to(DEV)
    stats = torch.zeros(4, ADA_MB, ADA_C, device=DEV)
    counters = torch.zeros(2, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    N.check(_adain_call(x, x, stats, counters, ticket, 2, 0))
    torch.cuda.synchronize()
    xt, s0 = torch.from_numpy(x_np), torch.zeros(4, ADA_MB, ADA_C)
    _, s64, _ = R.adain(xt.double(), s0.double(), [0.0, 0.0], 2, 0)
    _, s32, _ = R.adain(xt, s0, [0.0, 0.0], 2, 0)
    e_ref = float((s32[3, :ADA_B].double() - s64[3, :ADA_B]).abs().max())
    err = maxerr(stats[3, :ADA_B], s64[3, :ADA_B])
    report("adain DC row std", err, e_ref)
    assert 0.009 < float(s64[3, :ADA_B].min()) and err <= 4 * e_ref
    assert maxerr(stats[2, :ADA_B], s64[2, :ADA_B]) < 1e-4                      # the mean, to fp32 at 100


def test_adain_refusals():
    x = torch.zeros(ADA_B, ADA_C, 16, device=DEV)
    y = torch.full_like(x, NAN)
    stats = torch.zeros(4, ADA_MB, ADA_C, device=DEV)
    counters = torch.ones(2, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    refused(lambda: _adain_call(x, y, stats, counters, ticket, 1, ADA_MB - ADA_B + 1), ValueError,
            "batch exceeds the statistics buffers")
    refused(lambda: _adain_call(x, y, stats, counters, ticket, 3, 0), ValueError, "mode must be")
    for mode in (1, 2):
        refused(lambda: _adain_call(x, y, stats, counters, None, mode, 0), ValueError, "need the ticket word")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and not stats.any() and counters.cpu().tolist() == [1.0, 1.0]


# ================================================================== 4. noise filter stage
def _noise_call(amp, u, y, n_band, nb, tgt, frames):
    N = _N()
    a = N.NoiseArgs(batch=amp.shape[0], frames=frames, n_band=n_band, noise_bands=nb, target=tgt,
                    amp=amp.data_ptr(), a_sb=amp.stride(0), a_sc=amp.stride(1),
                    u=u.data_ptr(), u_sb=u.stride(0),
                    y=y.data_ptr(), y_sb=y.stride(0), y_sc=y.stride(1))
    return N.lib.rave_noise_synth(C.byref(a), _st())


@pytest.mark.parametrize("frames", [1, 127, 128, 129])
@pytest.mark.parametrize("nb,tgt", [(5, 8), (5, 16), (9, 16)])
def test_noise_synth_all_pairs_vs_float64(nb, tgt, frames):
    """Every compiled (noise_bands, target) pair at frame counts round the
    128-thread workgroup, strided amp (a_sc > frames) and y, amplitudes that
    saturate the sigmoid at both ends (-40, 40) beside 0, 5 and Gaussian ones,
    u at both ends of [0, 1)."""
    N = _N()
    n_band, B = 3, 2
    rng = np.random.default_rng(100 * nb + tgt + frames)
    amp_np = (rng.standard_normal((B, n_band * nb, frames)) * 4 + 3).astype(np.float32)
    flat = amp_np.reshape(-1)
    flat[::5] = np.resize(np.array([-40, 0, 5, 40], np.float32), len(flat[::5]))
    u_np = rng.uniform(0, 1, (B, frames, n_band, tgt)).astype(np.float32)
    uf = u_np.reshape(-1)
    uf[::9], uf[4::9] = 0.0, np.float32(1 - 2.0 ** -24)
    abuf, amp, _ = put(amp_np, [(0, 0), (1, 1), (2, 3)])
    ubuf2 = torch.full((B, u_np[0].size + 5), NAN, device=DEV)           # a batch stride above the row
    ubuf2[:, :u_np[0].size] = torch.from_numpy(u_np.reshape(B, -1)).to(DEV)
    ybuf, y, ymask = guarded((B, n_band, frames * tgt), [(0, 0), (1, 1), (3, 4)])
    a0, u0 = abuf.clone(), ubuf2.clone()
    N.check(_noise_call(amp, ubuf2, y, n_band, nb, tgt, frames))
    torch.cuda.synchronize()
    want = R.noise_synth(amp_np, u_np, n_band, nb, tgt)
    e_ref = maxerr(R.noise_synth(amp_np, u_np, n_band, nb, tgt, np.float32), want)
    err = maxerr(y, want)
    report(f"noise ({nb}, {tgt}) frames {frames}", err, e_ref)
    assert err <= 4 * e_ref
    assert untouched(ybuf, ymask) and same_bits(abuf, a0) and same_bits(ubuf2, u0)


def test_noise_synth_refusals():
    amp = torch.zeros(1, 3 * 9, 4, device=DEV)
    u = torch.zeros(1, 4, 3, 16, device=DEV)
    y = torch.full((1, 3, 64), NAN, device=DEV)
    refused(lambda: _noise_call(amp, u, y, 3, 9, 8, 4), ValueError, "target must be >= 2*(noise_bands-1)")
    refused(lambda: _noise_call(amp, u, y, 3, 5, 7, 4), ValueError, "target must be >= 2*(noise_bands-1)")
    refused(lambda: _noise_call(amp, u, y, 3, 5, 12, 4), NotImplementedError, "supported (noise_bands, target)")
    refused(lambda: _noise_call(amp, u, y, 3, 7, 16, 4), NotImplementedError, "supported (noise_bands, target)")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ================================================================== 5. speaker pooling head
SPK_B, SPK_CH = 2, 7
VAR_MIN, VAR_MAX = 1e-4, 1e4


def _pool_call(kind, x, logits, y, act, var_min=VAR_MIN, var_max=VAR_MAX):
    N = _N()
    B, Ch, T = x.shape
    kw = dict(batch=B, channels=Ch, t_len=T, act=N.ACT[act], leaky_slope=0.2, var_min=var_min, var_max=var_max,
              x=x.data_ptr(), x_sb=x.stride(0), x_sc=x.stride(1), y=y.data_ptr(), y_sb=y.stride(0))
    if kind == "row":
        return N.lib.rave_row_stats(C.byref(N.RowStatsArgs(**kw)), _st())
    return N.lib.rave_attn_pool(C.byref(N.AttnPoolArgs(logits=logits.data_ptr(), l_sb=logits.stride(0),
                                                       l_sc=logits.stride(1), **kw)), _st())


def _pool(kind, x_np, lg_np, act, var_min=VAR_MIN, var_max=VAR_MAX):
    """The kernel's (B, 2 Ch) on strided inputs, guards and inputs checked."""
    N = _N()
    xbuf, x, _ = put(x_np, [(0, 0), (1, 1), (2, 1)])
    lbuf, lg, _ = put(lg_np, [(0, 1), (0, 2), (0, 5)])
    ybuf, y, ymask = guarded((SPK_B, 2 * SPK_CH), [(0, 0), (0, 5)])          # y_sb > 2 Ch
    x0, l0 = xbuf.clone(), lbuf.clone()
    N.check(_pool_call(kind, x, lg, y, act, var_min, var_max))
    torch.cuda.synchronize()
    assert untouched(ybuf, ymask) and same_bits(xbuf, x0) and same_bits(lbuf, l0)
    return y.cpu()


def _pool_check(what, kind, x_np, lg_np, act, **kw):
    xt, lt = torch.from_numpy(x_np), torch.from_numpy(lg_np)
    if kind == "row":
        fn = lambda x: R.row_stats(x, act, 0.2, VAR_MIN, VAR_MAX)
        want, e_ref = R.e_ref_of(fn, xt)
    else:
        fn = lambda x, l: R.attn_pool(x, l, act, 0.2, VAR_MIN, VAR_MAX)
        want, e_ref = R.e_ref_of(fn, xt, lt)
    got = _pool(kind, x_np, lg_np, act, **kw)
    err = maxerr(got, want)
    report(what, err, e_ref)
    assert err <= 4 * e_ref
    return got, want


@pytest.mark.parametrize("act", ["none", "leaky"])
@pytest.mark.parametrize("t_len", [2, 255, 256, 257, 700])
def test_row_stats_and_attn_pool_vs_float64(t_len, act):
    rng = np.random.default_rng(t_len)
    x = rng.standard_normal((SPK_B, SPK_CH, t_len)).astype(np.float32)
    lg = (3 * rng.standard_normal((SPK_B, SPK_CH, t_len))).astype(np.float32)
    _pool_check(f"row_stats T={t_len} {act}", "row", x, lg, act)
    _pool_check(f"attn_pool T={t_len} {act}", "attn", x, lg, act)


@pytest.mark.parametrize("offset", [80.0, -80.0])
def test_attn_pool_needs_its_max_subtraction(offset):
    """Logits round +-80: exp of them over- or underflows fp32 unless the row
    maximum is subtracted first."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((SPK_B, SPK_CH, 257)).astype(np.float32)
    lg = (offset + 3 * rng.standard_normal((SPK_B, SPK_CH, 257))).astype(np.float32)
    got, _ = _pool_check(f"attn_pool logits {offset:+.0f}", "attn", x, lg, "leaky")
    assert bool(torch.isfinite(got).all())


def test_attn_pool_clamps_at_both_ends():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((SPK_B, SPK_CH, 300)).astype(np.float32)
    lg = rng.standard_normal((SPK_B, SPK_CH, 300)).astype(np.float32)
    lg[:, :, 17] += 60.0                       # one frame takes all the weight: the variance collapses
    got = _pool("attn", x, lg, "none")
    assert np.array_equal(got[:, SPK_CH:].numpy(), np.full((SPK_B, SPK_CH), np.sqrt(np.float32(VAR_MIN))))
    assert maxerr(got[:, :SPK_CH], x[:, :, 17]) < 1e-6
    lg = rng.standard_normal((SPK_B, SPK_CH, 300)).astype(np.float32)
    got = _pool("attn", 1000 * x, lg, "none")  # variance ~1e6 > var_max
    assert np.array_equal(got[:, SPK_CH:].numpy(), np.full((SPK_B, SPK_CH), np.float32(100.0)))
    got = _pool("row", 1000 * x, lg, "none")
    assert np.array_equal(got[:, SPK_CH:].numpy(), np.full((SPK_B, SPK_CH), np.float32(100.0)))
    got = _pool("row", np.full_like(x, 3.0), lg, "none")
    assert np.array_equal(got[:, SPK_CH:].numpy(), np.full((SPK_B, SPK_CH), np.sqrt(np.float32(VAR_MIN))))
    assert np.array_equal(got[:, :SPK_CH].numpy(), np.full((SPK_B, SPK_CH), np.float32(3.0)))


def test_attn_pool_dc_offset_row():
    """Mean 10, std 0.1: the reference's formula is one-pass (sum a^2 w - mu^2),
    so its fp32 run loses digits too and e_ref says how many."""
    rng = np.random.default_rng(9)
    x = (10 + 0.1 * rng.standard_normal((SPK_B, SPK_CH, 700))).astype(np.float32)
    lg = rng.standard_normal((SPK_B, SPK_CH, 700)).astype(np.float32)
    _pool_check("attn_pool DC row", "attn", x, lg, "none")


@pytest.mark.parametrize("n_out", [1, 5])
@pytest.mark.parametrize("n_in", [1, 63, 64, 65, 200])
def test_linear_vs_float64(n_in, n_out):
    N = _N()
    rng = np.random.default_rng(10 * n_in + n_out)
    x_np = rng.standard_normal((SPK_B, n_in)).astype(np.float32)
    w_np = rng.standard_normal((n_out, n_in)).astype(np.float32)
    b_np = rng.standard_normal(n_out).astype(np.float32)
    xbuf, x, _ = put(x_np, [(0, 0), (0, 3)])
    w, b = torch.from_numpy(w_np).to(DEV), torch.from_numpy(b_np).to(DEV)
    x0, w0, b0 = xbuf.clone(), w.clone(), b.clone()
    got, want, ref32 = [], [], []
    for bias in (b, None):
        ybuf, y, ymask = guarded((SPK_B, n_out), [(0, 1), (0, 2)])
        a = N.LinearArgs(batch=SPK_B, n_in=n_in, n_out=n_out, x=x.data_ptr(), x_sb=x.stride(0), w=w.data_ptr(),
                         bias=0 if bias is None else bias.data_ptr(), y=y.data_ptr(), y_sb=y.stride(0))
        N.check(N.lib.rave_linear(C.byref(a), _st()))
        torch.cuda.synchronize()
        assert untouched(ybuf, ymask)
        args = [torch.from_numpy(x_np), torch.from_numpy(w_np)] + ([] if bias is None else [torch.from_numpy(b_np)])
        got.append(y.cpu())
        want.append(R.linear(*[t.double() for t in args]))
        ref32.append(R.linear(*args).double())
    assert same_bits(xbuf, x0) and same_bits(w, w0) and same_bits(b, b0)
    want = torch.cat(want)
    e_ref = float((torch.cat(ref32) - want).abs().max())
    err = maxerr(torch.cat(got), want)
    report(f"linear n_in={n_in} n_out={n_out}", err, e_ref)
    assert err <= 4 * e_ref


@pytest.mark.parametrize("kernel,t_in", [(2, 101), (3, 101), (3, 99), (2, 75001)])
def test_maxpool_bitwise(kernel, t_in):
    """t_in no multiple of the kernel (the tail is dropped); 7 x 37500 outputs
    exceed 1024 x 256, so the grid-stride loop wraps."""
    N = _N()
    rng = np.random.default_rng(t_in + kernel)
    x_np = rng.standard_normal((SPK_B, SPK_CH, t_in)).astype(np.float32)
    t_out = t_in // kernel
    xbuf, x, _ = put(x_np, [(0, 0), (1, 0), (1, 2)])
    ybuf, y, ymask = guarded((SPK_B, SPK_CH, t_out), [(0, 0), (0, 2), (3, 1)])
    x0 = xbuf.clone()
    a = N.MaxPoolArgs(batch=SPK_B, channels=SPK_CH, t_out=t_out, kernel=kernel, x=x.data_ptr(), x_sb=x.stride(0),
                      x_sc=x.stride(1), y=y.data_ptr(), y_sb=y.stride(0), y_sc=y.stride(1))
    N.check(N.lib.rave_maxpool(C.byref(a), _st()))
    torch.cuda.synchronize()
    assert same_bits(y.cpu(), torch.from_numpy(R.maxpool(x_np, kernel)))
    assert untouched(ybuf, ymask) and same_bits(xbuf, x0)


# ================================================================== 6. copy, fill, shift
@pytest.mark.parametrize("channels,t_len", [(3, 100_000), (5, 1), (4, 257)])
def test_copy_and_fill_bitwise(channels, t_len):
    """3 x 100000 elements exceed the 1024 x 256 grid (the loop wraps)."""
    N = _N()
    B = 2
    rng = np.random.default_rng(channels)
    x_np = rng.standard_normal((B, channels, t_len)).astype(np.float32)
    xbuf, x, _ = put(x_np, [(0, 0), (2, 1), (1, 3)])
    ybuf, y, ymask = guarded(x_np.shape, [(0, 1), (1, 0), (4, 2)])
    x0 = xbuf.clone()
    a = N.CopyArgs(batch=B, channels=channels, t_len=t_len, x=x.data_ptr(), x_sb=x.stride(0), x_sc=x.stride(1),
                   y=y.data_ptr(), y_sb=y.stride(0), y_sc=y.stride(1))
    N.check(N.lib.rave_copy(C.byref(a), _st()))
    torch.cuda.synchronize()
    assert same_bits(y.cpu(), torch.from_numpy(x_np)) and untouched(ybuf, ymask) and same_bits(xbuf, x0)
    vals = torch.from_numpy(rng.standard_normal(channels + 2).astype(np.float32)).to(DEV)
    ybuf, y, ymask = guarded(x_np.shape, [(0, 1), (1, 0), (4, 2)])
    f = N.FillArgs(batch=B, channels=channels, t_len=t_len, y=y.data_ptr(), y_sb=y.stride(0), y_sc=y.stride(1),
                   values=vals.data_ptr())
    v0 = vals.clone()
    N.check(N.lib.rave_fill_channels(C.byref(f), _st()))
    torch.cuda.synchronize()
    assert same_bits(y, vals[:channels, None].expand(B, channels, t_len)) and untouched(ybuf, ymask)
    assert same_bits(vals, v0)


@pytest.mark.parametrize("t_new", [1, 7, 2048])
@pytest.mark.parametrize("hist", [1, 63, 64, 65, 300])
def test_shift_history_single_buffer(hist, t_new):
    """In place, both t_new < hist (the move overlaps itself) and t_new > hist;
    3 x 3 rows (no multiple of the four rows of a workgroup)."""
    from tests.test_gpu_parity import _shift_ref
    N = _N()
    B, Cc = 3, 3
    rng = np.random.default_rng(hist * 10000 + t_new)
    a_np = rng.standard_normal((B, Cc, hist + t_new)).astype(np.float32)
    buf, view, mask = put(a_np, [(0, 0), (1, 1), (2, 3)])
    s = N.ShiftArgs(batch=B, channels=Cc, hist=hist, t_new=t_new, buf=view.data_ptr(), sb=view.stride(0),
                    sc=view.stride(1))
    N.check(N.lib.rave_shift_history(C.byref(s), _st()))
    torch.cuda.synchronize()
    want = _shift_ref(a_np, hist, t_new)
    assert np.array_equal(want, R.shift_history(a_np, hist, t_new))
    assert same_bits(view.cpu(), torch.from_numpy(want)) and untouched(buf, mask)
