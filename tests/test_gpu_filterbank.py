"""The filterbank kernels at their edges (rave_amd/csrc/pqmf.hip: the fp32 and
split-f16 analysis and synthesis; fir_kernel of rave_amd/csrc/speaker.hip),
called through rave_amd._native at the C boundary, against the restatements of
tests/filterbank_ref.py (which tests/test_filterbank_ref_host.py pins against
the oracle and the fixtures on the CPU).

Every input is a strided view inside a NaN-filled buffer, so an over-read
reaches the result; every output is a view inside a NaN-filled buffer with
guard rows and columns.  After each call the guards are still NaN and the
inputs (filters included) are bit for bit what they were.

Bounds.  fp32 kernels and the FIR: 4 e_ref, e_ref the max-abs error over the
case's outputs of the restatement's fp32 run (one chain in the kernel's
documented order) against its float64 run.  Split-f16 kernels: 4 e_ref + 2e-6
max(1, max|ref|), the second term being what test_pqmf_split16_matches_f32
allows them against the fp32 kernels.  Where the fp32 arithmetic is exact (a
unit impulse leaves one non-zero product in the chain; a streamed block runs
the same chain as the one-shot call; a rerun) values are compared for equality.

Measured on an MI355X (kernel error / e_ref for the fp32 kernels and the FIR;
kernel error / bound for the split-f16 ones; the worst case of each group):
Analysis, every frame count, band count, batch, pad and input length, the
remapped grid of 8 and the probe filter: fp32 1.00 in every case (the kernel's
error is the restatement's fp32 error to all printed digits: the MFMA chain is
the fma chain), split-f16 at most 0.08 of its bound (probe filter 0.10).
Synthesis, t_in = 1 15 16 17 127 128 129 257, the worst of the modes and forms:
fp32 1.39 1.37 1.33 1.51 1.11 1.15 1.11 1.25 (mode 0 is 1.00 throughout; modes
1 and 2 carry __expf and tanhf), split-f16 0.10 0.11 0.12 0.13 0.13 0.15 0.13
0.12; x_len = 1: 1.52 / 0.10; 511 frames cached on the remapped grid 1.09 /
0.08; saturated logits and carriers 1.00 / 0.08; streamed blocks 1.00 / 0.10.
Unit impulses: fp32 equal to the taps; split-f16 3.7e-9 (analysis) and 1.2e-7
(synthesis) against the bound 2e-6.
Range guard, scale 3e6 / one 1e5 sample: analysis fp32 1.00 1.00, split-f16
0.09 0.11; synthesis fp32 1.00 1.00, split-f16 0.08 0.07.
FIR, all sixteen geometries and every t_out: 1.00 (the fmaf chain itself)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import filterbank_ref as R
from tests.test_gpu_aux_kernels import DEV, guarded, maxerr, put, refused, report, same_bits, untouched

pytestmark = pytest.mark.gpu
PRECS = ("f32", "split16")
SPLIT_REL = 2e-6                    # test_pqmf_split16_matches_f32's bound, relative to max(1, max|ref|)
FRAME_COUNTS = [1, 15, 16, 17, 127, 128, 129, 257]      # a wave block is 16 frames, a workgroup 128


def _N():
    from rave_amd import _native as N
    return N


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _filters():
    from rave_amd.pqmf import kernels
    from tests.conftest import GOLDEN
    hkf, hki = kernels(np.load(os.path.join(GOLDEN, "pqmf.npz"))["hk"])
    assert hkf.shape == (16, 513) and hki.shape == (16, 16, 33)
    return hkf, hki


def _bound(prec, e_ref, ref):
    return 4 * e_ref + (SPLIT_REL * max(1.0, float(np.abs(ref).max())) if prec == "split16" else 0.0)


def _held(what, prec, got, ref, e_ref):
    """Print the figures, then assert the bound; returns the group's ratio
    (error / e_ref for fp32, error / bound for split-f16)."""
    err = maxerr(got, ref)
    bound = _bound(prec, e_ref, ref)
    if prec == "f32":
        ratio = report(f"{what} f32", err, e_ref)
    else:
        ratio = err / bound
        print(f"{what} split16: e_ref {e_ref:.3e} kernel {err:.3e} bound {bound:.3e} ratio {ratio:.2f}")
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), what
    assert err <= bound, (what, prec, err, e_ref, bound)
    return ratio


# ================================================================== 1. analysis
def _analysis(x_np, pad_left, t_out, n_out, prec, taps=513, hkf=None, n_band=16, precision=None, t_out_arg=None):
    """The kernel's (B, n_out, t_out) for x (B, t_in): x_sb > t_in, the output a
    16-row view with y_sc > t_out and y_sb > 16 y_sc; guards (rows n_out..15
    among them) and inputs checked.  The keyword overrides are the refusals'."""
    N = _N()
    B, t_in = x_np.shape
    h = torch.from_numpy(_filters()[0] if hkf is None else hkf).to(DEV)
    xbuf, x, _ = put(x_np, [(0, 1), (3, 5)])
    ybuf, y, ymask = guarded((B, 16, t_out), [(0, 1), (1, 2), (2, 3)])
    assert x.stride(0) > t_in and y.stride(1) > t_out and y.stride(0) > 16 * y.stride(1)
    x0, h0 = xbuf.clone(), h.clone()
    a = N.AnalysisArgs(n_band=n_band, taps=taps, n_out_bands=n_out, batch=B, t_in=t_in, pad_left=pad_left,
                       t_out=t_out if t_out_arg is None else t_out_arg,
                       precision=N.PRECISION[prec] if precision is None else precision,
                       x=x.data_ptr(), x_sb=x.stride(0), y=y.data_ptr(), y_sb=y.stride(0), y_sc=y.stride(1),
                       hkf=h.data_ptr())
    rc = N.lib.rave_pqmf_analysis(C.byref(a), _st())
    torch.cuda.synchronize()
    assert untouched(ybuf, ymask) and same_bits(xbuf, x0) and same_bits(h, h0)
    if rc != N.RAVE_OK:
        assert bool(torch.isnan(ybuf).all())
        return rc
    assert bool(torch.isnan(y[:, n_out:]).all())                    # the 6-band guard: rows 6..15 stay NaN
    return y[:, :n_out].cpu().numpy()


def _analysis_t_in(pad_left, t_out, short):
    """The input length of a case.  The window of the last frame ends at sample
    16 (t_out - 1) + 513 - pad_left; ``short`` stops well before it (the right
    edge is zero-filled) and off a multiple of 16."""
    full = 16 * (t_out - 1) + 513 - pad_left
    return max(1, full - 200 - 7) if short else full + 3


@pytest.mark.parametrize("t_out", FRAME_COUNTS)
def test_analysis_vs_float64(t_out):
    """6 and 16 bands, B 1 and 3, the centred, causal and cached pads, inputs
    that cover the last window and inputs that stop short of it (B = 3 at 257
    frames is a grid of 9: no XCD remap)."""
    hkf, _ = _filters()
    worst = {p: 0.0 for p in PRECS}
    for n_out in (6, 16):
        for B in (1, 3):
            for pad_left in (256, 512, 0):
                t_in = _analysis_t_in(pad_left, t_out, short=B == 3)
                rng = np.random.default_rng(t_out * 100 + B + pad_left)
                x = (0.5 * rng.standard_normal((B, t_in))).astype(np.float32)
                ref, e_ref = R.with_e_ref(R.analysis, x, hkf, pad_left, t_out, n_out)
                for prec in PRECS:
                    got = _analysis(x, pad_left, t_out, n_out, prec)
                    what = f"analysis t_out={t_out} n_out={n_out} B={B} pad={pad_left} t_in={t_in}"
                    worst[prec] = max(worst[prec], _held(what, prec, got, ref, e_ref))
    print(f"analysis t_out={t_out}: worst ratio f32 {worst['f32']:.2f}, split16 {worst['split16']:.2f}")


@pytest.mark.parametrize("B,t_out,t_in", [(2, 511, 16 * 511), (2, 511, 8000), (2, 3, 1), (1, 1, 1)])
def test_analysis_remapped_grid_and_one_sample(B, t_out, t_in):
    """B = 2, 511 frames: 4 x 2 = 8 workgroups, the grid xcd_major remaps.  And
    t_in = 1: every window read but one is out of range."""
    hkf, _ = _filters()
    x = (0.5 * np.random.default_rng(t_in).standard_normal((B, t_in))).astype(np.float32)
    for n_out, pad_left in ((6, 256), (16, 512), (16, 0)):
        ref, e_ref = R.with_e_ref(R.analysis, x, hkf, pad_left, t_out, n_out)
        for prec in PRECS:
            got = _analysis(x, pad_left, t_out, n_out, prec)
            _held(f"analysis B={B} t_out={t_out} t_in={t_in} n_out={n_out} pad={pad_left}", prec, got, ref, e_ref)


ANA_T_IN, ANA_T_OUT = 16 * 257, 257
# sample 0, the last one, and round the workgroup boundary (frame 128 = sample 2048).  With pad 256 the
# impulse at s meets tap s + 256 - 16 t: 2047 meets taps 15..511, 2048 taps 0..512, 2049 taps 1..497.
ANA_IMPULSES = (0, 2047, 2048, 2049, ANA_T_IN - 1)


@pytest.mark.parametrize("pad_left", [256, 512, 0])
@pytest.mark.parametrize("n_out", [6, 16])
def test_analysis_unit_impulses(n_out, pad_left):
    """One row per impulse.  The fp32 MFMA chain has one non-zero product, so
    the kernel returns the tap itself, signed: equal values (np.array_equal, -0
    equal to 0).  The split-f16 kernel within its bound (e_ref = 0)."""
    hkf, _ = _filters()
    x = np.zeros((len(ANA_IMPULSES), ANA_T_IN), np.float32)
    for row, s in enumerate(ANA_IMPULSES):
        x[row, s] = 1.0
    want = np.stack([R.analysis_impulse(hkf, s, pad_left, ANA_T_OUT, n_out) for s in ANA_IMPULSES])
    if pad_left == 256:
        hit = {int(j) for s in ANA_IMPULSES for j in s + pad_left - 16 * np.arange(ANA_T_OUT) if 0 <= j < 513}
        assert {0, 511, 512} <= hit
    assert np.array_equal(R.analysis(x, hkf, pad_left, ANA_T_OUT, n_out, np.float32), want)
    got = _analysis(x, pad_left, ANA_T_OUT, n_out, "f32")
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    _held(f"analysis impulses n_out={n_out} pad={pad_left}", "split16",
          _analysis(x, pad_left, ANA_T_OUT, n_out, "split16"), want.astype(np.float64), 0.0)


def test_analysis_last_tap_with_a_probe_filter():
    """The prototype's 513th tap is zero, so a filter with every entry distinct
    and non-zero shows whether tap 512 (behind the padding to 516 / 544) and
    tap 0 land where they belong: impulses through the fp32 kernel, bitwise."""
    rng = np.random.default_rng(513)
    probe = rng.uniform(0.5, 1.5, (16, 513)).astype(np.float32)
    probe = probe * np.where(rng.random((16, 513)) < 0.5, -1, 1).astype(np.float32)
    x = np.zeros((3, 16 * 40), np.float32)
    x[0, 0] = x[1, 15] = x[2, 16 * 33] = 1.0
    for pad_left in (512, 256):
        want = np.stack([R.analysis_impulse(probe, s, pad_left, 40, 16) for s in (0, 15, 16 * 33)])
        if pad_left == 512:                 # sample 0 meets tap 512 at frame 0, sample 15 tap 511 at frame 1
            assert np.array_equal(np.abs(want[0][:, 0]), np.abs(probe[:, 512]))
            assert np.array_equal(want[1][:, 1], probe[:, 511])
        got = _analysis(x, pad_left, 40, 16, "f32", hkf=probe)
        assert np.array_equal(got, want), (pad_left, np.argwhere(got != want)[:8])
    xr = (0.5 * rng.standard_normal((2, 16 * 40))).astype(np.float32)
    ref, e_ref = R.with_e_ref(R.analysis, xr, probe, 512, 40, 16)
    for prec in PRECS:
        _held("analysis probe filter", prec, _analysis(xr, 512, 40, 16, prec, hkf=probe), ref, e_ref)


# ================================================================== 2. synthesis
def _synthesis(x_np, noise_np, pad_left, mode, frame0, x_len, t_in, prec, taps=33, y_shift=0, y_extra=0,
               n_band=16):
    """The kernel's (B, 16 t_in).  x (B, 16 or 32, x_len or t_in) sits in a
    NaN buffer with x_sc > x_len and NaN rows above row 16 / 32; the noise
    likewise; y_sb > 16 t_in with NaN between the rows.  y_shift / y_extra
    (floats) break the alignment rules for the refusals."""
    N = _N()
    B, rows, xl = x_np.shape
    assert xl == (x_len if x_len > 0 else t_in) and rows == (32 if mode == 1 else 16)
    h = torch.from_numpy(_filters()[1]).to(DEV)
    xbuf, x, _ = put(x_np, [(0, 1), (1, 2), (3, 4)])
    nbuf = nz = None
    if noise_np is not None:
        nbuf, nz, _ = put(noise_np, [(0, 1), (2, 1), (1, 6)])
    ybuf, y, ymask = guarded((B, 16 * t_in), [(0, 1), (4 + y_shift, 8 - y_shift + y_extra)])
    assert x.stride(1) > xl and y.stride(0) > 16 * t_in
    x0, h0, n0 = xbuf.clone(), h.clone(), None if nbuf is None else nbuf.clone()
    a = N.SynthesisArgs(n_band=n_band, taps=taps, batch=B, t_in=t_in, pad_left=pad_left, mode=mode, frame0=frame0,
                        x_len=x_len, x=x.data_ptr(), x_sb=x.stride(0), x_sc=x.stride(1),
                        noise=None if nz is None else nz.data_ptr(),
                        n_sb=0 if nz is None else nz.stride(0), n_sc=0 if nz is None else nz.stride(1),
                        y=y.data_ptr(), y_sb=y.stride(0), hki=h.data_ptr(), precision=N.PRECISION[prec])
    rc = N.lib.rave_pqmf_synthesis(C.byref(a), _st())
    torch.cuda.synchronize()
    assert untouched(ybuf, ymask) and same_bits(xbuf, x0) and same_bits(h, h0)
    assert nbuf is None or same_bits(nbuf, n0)
    if rc != N.RAVE_OK:
        assert bool(torch.isnan(ybuf).all())
        return rc
    return y.cpu().numpy()


SYN_MODES = [(0, False), (1, True), (1, False), (2, True)]                     # (mode, noise given)
# (pad_left, x_len - t_in or None for x_len = 0, frame0)
SYN_FORMS = [(16, None, 0), (32, None, 7), (0, 32, -32), (0, 32, -31), (0, 5, 7), (16, 5, -31), (32, 32, 0)]


def _syn_inputs(rng, B, mode, xl, with_noise):
    x = rng.standard_normal((B, 32 if mode == 1 else 16, xl)).astype(np.float32)
    nz = (0.1 * rng.standard_normal((B, 16, xl))).astype(np.float32) if with_noise else None
    return x, nz


@pytest.mark.parametrize("t_in", FRAME_COUNTS)
def test_synthesis_vs_float64(t_in):
    """Every mode (mode 1 with the noise and with noise = NULL) in every form:
    offline centred and causal, the cached form with even and odd frame0, an
    x_len that ends inside the window, and x_len > 0 with a pad."""
    _, hki = _filters()
    worst = {p: 0.0 for p in PRECS}
    for mi, (mode, with_noise) in enumerate(SYN_MODES):
        for fi, (pad_left, extra, frame0) in enumerate(SYN_FORMS):
            B = 1 + (mi + fi) % 3
            x_len = 0 if extra is None else t_in + extra
            x, nz = _syn_inputs(np.random.default_rng(1000 * t_in + 10 * mi + fi), B, mode, x_len or t_in, with_noise)
            ref, e_ref = R.with_e_ref(R.synthesis, x, hki, pad_left, mode, frame0, x_len, nz, t_in)
            for prec in PRECS:
                got = _synthesis(x, nz, pad_left, mode, frame0, x_len, t_in, prec)
                what = (f"synthesis t_in={t_in} mode={mode} noise={with_noise} pad={pad_left} x_len={x_len} "
                        f"frame0={frame0} B={B}")
                worst[prec] = max(worst[prec], _held(what, prec, got, ref, e_ref))
    print(f"synthesis t_in={t_in}: worst ratio f32 {worst['f32']:.2f}, split16 {worst['split16']:.2f}")


@pytest.mark.parametrize("t_in", [1, 17, 129])
def test_synthesis_one_input_column(t_in):
    """x_len = 1: the clamp max(x_len - 1, 0) is all that keeps the staging
    reads inside the one column there is."""
    _, hki = _filters()
    for mode, with_noise in SYN_MODES:
        for pad_left, frame0 in ((16, 0), (0, -31), (32, 7)):
            x, nz = _syn_inputs(np.random.default_rng(t_in + mode), 2, mode, 1, with_noise)
            ref, e_ref = R.with_e_ref(R.synthesis, x, hki, pad_left, mode, frame0, 1, nz, t_in)
            for prec in PRECS:
                got = _synthesis(x, nz, pad_left, mode, frame0, 1, t_in, prec)
                _held(f"synthesis x_len=1 t_in={t_in} mode={mode} pad={pad_left} frame0={frame0}", prec, got, ref, e_ref)


def test_synthesis_remapped_grid():
    """B = 2, 511 frames: 8 workgroups, the grid xcd_major remaps."""
    _, hki = _filters()
    x, nz = _syn_inputs(np.random.default_rng(511), 2, 1, 511 + 32, True)
    ref, e_ref = R.with_e_ref(R.synthesis, x, hki, 0, 1, -31, 511 + 32, nz, 511)
    for prec in PRECS:
        _held("synthesis B=2 t_in=511 cached", prec, _synthesis(x, nz, 0, 1, -31, 511 + 32, 511, prec), ref, e_ref)


def test_synthesis_saturated_epilogue():
    """Amplitude logits of +-100 (__expf overflows to inf or flushes to 0) and
    carriers of +-50 (tanh saturates): finite and within the bound."""
    _, hki = _filters()
    rng = np.random.default_rng(50)
    t_in = 129
    for mode, with_noise in ((1, True), (1, False), (2, True)):
        x, nz = _syn_inputs(rng, 2, mode, t_in, with_noise)
        carrier = np.ascontiguousarray(x[:, :16])
        carrier.reshape(-1)[::3] = np.resize(np.array([50, -50], np.float32), carrier.reshape(-1)[::3].size)
        x[:, :16] = carrier
        if mode == 1:
            amp = np.ascontiguousarray(x[:, 16:])
            amp.reshape(-1)[::5] = np.resize(np.array([100, -100, 100], np.float32), amp.reshape(-1)[::5].size)
            x[:, 16:] = amp
            assert (x[:, 16:] == 100).any() and (x[:, 16:] == -100).any()
        assert (x[:, :16] == 50).any() and (x[:, :16] == -50).any()
        ref, e_ref = R.with_e_ref(R.synthesis, x, hki, 16, mode, 0, 0, nz, t_in)
        for prec in PRECS:
            _held(f"synthesis saturated mode={mode}", prec, _synthesis(x, nz, 16, mode, 0, 0, t_in, prec), ref, e_ref)


SYN_T = 257
SYN_IMPULSE_CHANNELS = (0, 1, 14, 15)


@pytest.mark.parametrize("pad_left,x_extra", [(16, None), (32, None), (0, 32)])
@pytest.mark.parametrize("frame0", [0, 7])
def test_synthesis_unit_impulses(frame0, pad_left, x_extra):
    """One row per (channel, column): columns 0, the last, and round the
    workgroup boundary (127, 128, 129; 128 +- 1 have the other parity), channels
    of both parities, frame0 of both.  Column f meets tap f - t + pad_left: the
    first tap at t = f + pad_left, tap 31 (the last non-zero one) and the zero
    tap 32 further left.  fp32: 16 x the tap, signed, equal values."""
    _, hki = _filters()
    x_len = 0 if x_extra is None else SYN_T + x_extra
    xl = x_len or SYN_T
    cols = (0, 127, 128, 129, xl - 1)
    cases = [(c, f) for c in SYN_IMPULSE_CHANNELS for f in cols]
    x = np.zeros((len(cases), 16, xl), np.float32)
    for row, (c, f) in enumerate(cases):
        x[row, c, f] = 1.0
    want = np.stack([R.synthesis_impulse(hki, c, f, pad_left, frame0, SYN_T) for c, f in cases])
    assert np.abs(want).max() > 0 and (want < 0).any()
    assert np.array_equal(R.synthesis(x, hki, pad_left, 0, frame0, x_len, None, SYN_T, np.float32), want)
    got = _synthesis(x, None, pad_left, 0, frame0, x_len, SYN_T, "f32")
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    _held(f"synthesis impulses pad={pad_left} frame0={frame0}", "split16",
          _synthesis(x, None, pad_left, 0, frame0, x_len, SYN_T, "split16"), want.astype(np.float64), 0.0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_synthesis_streaming_blocks_equal_one_shot_bitwise(mode, prec):
    """The host test's signal in the cached form ([32 history | block], pad 0,
    x_len = 32 + T, frame0 = start - 32; blocks 1, 37, 128, 134): every output
    is the same (tap, channel) chain over the same values as in the causal
    one-shot call, whatever workgroup it falls into, so the concatenation is
    bitwise the one-shot output.  For the split-f16 kernel that needs the
    range guard's scale to be 1 in every workgroup: |staged input| <= max|x| <
    2^15 (asserted), and the filter's scale is the filter's alone."""
    _, hki = _filters()
    x, noise = R.stream_signal()
    assert np.abs(x).max() < 2 ** 15
    pick = (lambda a: a) if mode == 1 else (lambda a: np.ascontiguousarray(a[:, :16]))
    nz = None if mode == 0 else noise
    whole = _synthesis(pick(x), nz, 32, mode, 0, 0, R.STREAM_FRAMES, prec)
    parts = [_synthesis(pick(xb), None if mode == 0 else nb, 0, mode, s - R.STREAM_HIST, R.STREAM_HIST + T, T, prec)
             for s, T, xb, nb in R.stream_blocks(x, noise)]
    got = np.concatenate(parts, -1)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), np.argwhere(got != whole)[:8]
    ref, e_ref = R.with_e_ref(R.synthesis, pick(x), hki, 32, mode, 0, 0, nz, R.STREAM_FRAMES)
    _held(f"synthesis streamed mode={mode}", prec, got, ref, e_ref)


def test_reruns_are_bitwise_equal():
    hkf, _ = _filters()
    rng = np.random.default_rng(9)
    xa = (0.5 * rng.standard_normal((3, 16 * 257 + 5))).astype(np.float32)
    xs, nz = _syn_inputs(rng, 3, 1, 257 + 32, True)
    for prec in PRECS:
        a, b = (_analysis(xa, 256, 257, 6, prec) for _ in range(2))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        a, b = (_synthesis(xs, nz, 0, 1, -31, 257 + 32, 257, prec) for _ in range(2))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    h = rng.standard_normal((2, 21)).astype(np.float32)
    a, b = (_fir(xa, h, 1, 10, 600) for _ in range(2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ================================================================== 3. the split-f16 range guard
def _loud_and_spiked(rng, shape):
    """A signal of scale 3e6 (test_gpu_edges.py's HEAD_CASES), and one quiet
    but for a single 1e5 inside the second workgroup's window, so that
    neighbouring workgroups pick different scales."""
    loud = (3e6 * 0.3 * rng.standard_normal(shape)).astype(np.float32)
    spiked = (1e-2 * rng.standard_normal(shape)).astype(np.float32)
    return loud, spiked


def test_split16_range_guard_analysis():
    hkf, _ = _filters()
    rng = np.random.default_rng(36)
    t_out = 300
    loud, spiked = _loud_and_spiked(rng, (2, 16 * t_out))
    spiked[:, 16 * 128 + 700] = 1e5                                          # frames 128..255 are workgroup 1
    for name, x in (("3e6", loud), ("spike", spiked)):
        ref, e_ref = R.with_e_ref(R.analysis, x, hkf, 256, t_out, 16)
        for prec in PRECS:
            _held(f"range guard analysis {name}", prec, _analysis(x, 256, t_out, 16, prec), ref, e_ref)


def test_split16_range_guard_synthesis():
    _, hki = _filters()
    rng = np.random.default_rng(37)
    t_in = 300
    loud, spiked = _loud_and_spiked(rng, (2, 16, t_in))
    spiked[:, 3, 128 + 60] = 1e5
    for name, x in (("3e6", loud), ("spike", spiked)):
        ref, e_ref = R.with_e_ref(R.synthesis, x, hki, 16, 0, 0, 0, None, t_in)
        for prec in PRECS:
            _held(f"range guard synthesis {name}", prec, _synthesis(x, None, 16, 0, 0, 0, t_in, prec), ref, e_ref)


# ================================================================== 4. FIR
def _fir(x_np, h_np, stride, pad_left, t_out, y_short=0, taps=None, phases=None):
    """The kernel's (B, t_out P): x_sb > t_in, y_sb > t_out P, guards and
    inputs checked.  y_short / taps / phases are the refusals'."""
    N = _N()
    B, t_in = x_np.shape
    P, K = h_np.shape
    h = torch.from_numpy(h_np).to(DEV)
    xbuf, x, _ = put(x_np, [(0, 1), (3, 5)])
    ybuf, y, ymask = guarded((B, t_out * P), [(0, 1), (2, 3)])
    assert x.stride(0) > t_in and y.stride(0) > t_out * P
    x0, h0 = xbuf.clone(), h.clone()
    a = N.FirArgs(batch=B, t_in=t_in, t_out=t_out, phases=P if phases is None else phases,
                  taps=K if taps is None else taps, stride=stride, pad_left=pad_left, x=x.data_ptr(),
                  x_sb=x.stride(0), y=y.data_ptr(), y_sb=t_out * P - y_short if y_short else y.stride(0),
                  h=h.data_ptr())
    rc = N.lib.rave_fir(C.byref(a), _st())
    torch.cuda.synchronize()
    assert untouched(ybuf, ymask) and same_bits(xbuf, x0) and same_bits(h, h0)
    if rc != N.RAVE_OK:
        assert bool(torch.isnan(ybuf).all())
        return rc
    return y.cpu().numpy()


def _fir_frames(P, K, S):
    """Output frames per workgroup as rave_fir picks them (speaker.hip: 1024
    outputs per workgroup, halved until window + taps fit 16384 LDS floats)."""
    frames = max(1, 1024 // P)
    while frames > 1 and (frames - 1) * S + K + P * K > 16384:
        frames //= 2
    return frames


def _design(ratio):
    from rave_amd.resampler import design
    _, down, up = design(48000 * ratio, 48000)
    return down, up


def _fir_geometries():
    from rave_amd.config import get_padding
    rng = np.random.default_rng(4096)
    out = []
    for ratio in (2, 3):
        down, up = _design(ratio)
        for name, h, S in ((f"r{ratio} down", down, ratio), (f"r{ratio} up", up, 1)):
            K = h.shape[1]
            out.append((name + " offline", h, S, get_padding(K, S, causal=False)[0]))
            out.append((name + " causal", h, S, get_padding(K, S, causal=True)[0]))
            out.append((name + " cached", h, S, 0))
    out.append(("stride 64, 57 taps", rng.standard_normal((1, 57)).astype(np.float32), 64, 28))
    out.append(("1500 phases, 2 taps", rng.standard_normal((1500, 2)).astype(np.float32), 1, 1))
    out.append(("4 x 1024 taps", (rng.standard_normal((4, 1024)) / 32).astype(np.float32), 1, 512))
    out.append(("64 x 64 taps", (rng.standard_normal((64, 64)) / 8).astype(np.float32), 3, 5))
    return out


FIR_GEOMETRIES = ["r2 down offline", "r2 down causal", "r2 down cached", "r2 up offline", "r2 up causal",
                  "r2 up cached", "r3 down offline", "r3 down causal", "r3 down cached", "r3 up offline",
                  "r3 up causal", "r3 up cached", "stride 64, 57 taps", "1500 phases, 2 taps", "4 x 1024 taps",
                  "64 x 64 taps"]


@pytest.mark.parametrize("name", FIR_GEOMETRIES)
def test_fir_vs_float64(name):
    """The product's geometries (resampler.design, ratios 2 and 3, offline in
    both paddings and cached with pad_left 0), a stride of 64 (the launcher
    halves its frames to 128), 1500 phases (one frame per workgroup, six passes
    of the output loop), phases x taps = 4096 two ways; t_out of 1 and round the
    workgroup's frame count; windows that run past both ends of the input
    (pad_left > 0 at the left, an input three samples short at the right)."""
    geo = {g[0]: g for g in _fir_geometries()}
    assert list(geo) == FIR_GEOMETRIES
    _, h, S, pad_left = geo[name]
    P, K = h.shape
    frames = _fir_frames(P, K, S)
    assert frames == {"stride 64, 57 taps": 128, "1500 phases, 2 taps": 1}.get(name, frames)
    worst = 0.0
    for t_out in sorted({1, frames - 1, frames, frames + 1, 2 * frames + 1} - {0}):
        for B in (1, 3):
            t_in = max(1, (t_out - 1) * S + K - pad_left - 3)
            x = np.random.default_rng(t_out + B).standard_normal((B, t_in)).astype(np.float32)
            ref, e_ref = R.with_e_ref(R.fir, x, h, S, pad_left, t_out)
            got = _fir(x, h, S, pad_left, t_out)
            worst = max(worst, _held(f"fir {name} t_out={t_out} B={B}", "f32", got, ref, e_ref))
    print(f"fir {name}: frames {frames}, worst ratio {worst:.2f}")


@pytest.mark.parametrize("name", ["r2 down offline", "r2 up cached", "r3 up causal", "stride 64, 57 taps",
                                  "1500 phases, 2 taps"])
def test_fir_unit_impulses(name):
    """fmaf(h, 1, 0) is h: the kernel returns the tap itself, bitwise.  Impulses
    at sample 0, the last one, and where the window of the workgroup's last
    frame begins and ends."""
    geo = {g[0]: g for g in _fir_geometries()}
    _, h, S, pad_left = geo[name]
    P, K = h.shape
    frames = _fir_frames(P, K, S)
    t_out = 2 * frames + 1
    t_in = (t_out - 1) * S + K - pad_left
    edge = frames * S - pad_left
    spots = sorted({s for s in (0, edge - 1, edge, edge + 1, edge + K - 1, t_in - 1) if 0 <= s < t_in})
    x = np.zeros((len(spots), t_in), np.float32)
    for row, s in enumerate(spots):
        x[row, s] = 1.0
    want = np.stack([R.fir_impulse(h, s, S, pad_left, t_out) for s in spots])
    assert np.abs(want).max() > 0
    got = _fir(x, h, S, pad_left, t_out)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


# ================================================================== 5. refusals
def test_analysis_refusals():
    N = _N()
    x = np.zeros((1, 512), np.float32)
    bad = lambda **kw: (lambda: _analysis(x, 256, 32, kw.pop("n_out", 16), "f32", **kw))
    refused(bad(n_band=8), ValueError, "built for 16 bands")
    refused(bad(n_out=5), ValueError, "n_out_bands must be 6")
    refused(bad(taps=511), NotImplementedError, "513-tap")
    refused(bad(taps=517), NotImplementedError, "513-tap")
    refused(bad(precision=N.PREC_BF16X3), ValueError, "precision must be")
    refused(bad(t_out_arg=0), ValueError, "empty shape")
    assert _analysis(x, 256, 32, 16, "f32", taps=511) == N.RAVE_ERR_UNSUPPORTED


def test_synthesis_refusals():
    N = _N()
    x = np.zeros((1, 16, 32), np.float32)
    bad = lambda mode=0, **kw: (lambda: _synthesis(x, None, 16, mode, 0, 0, 32, "f32", **kw))
    refused(bad(taps=31), NotImplementedError, "33-tap")
    refused(bad(mode=3), ValueError, "mode must be 0, 1 or 2")
    refused(bad(y_shift=1), ValueError, "16-byte aligned")                   # y itself off alignment
    refused(bad(y_extra=1), ValueError, "16-byte aligned")                   # y_sb % 4 != 0
    assert _synthesis(x, None, 16, 0, 0, 0, 32, "f32", taps=31) == N.RAVE_ERR_UNSUPPORTED


def test_fir_refusals():
    x = np.zeros((2, 300), np.float32)
    h = np.zeros((2, 21), np.float32)
    refused(lambda: _fir(x, h, 1, -1, 100), ValueError, "negative pad_left")
    refused(lambda: _fir(x, h, 65, 0, 4), ValueError, "stride above 64")
    refused(lambda: _fir(x, np.zeros((1, 1025), np.float32), 1, 0, 100), ValueError, "too many taps")
    refused(lambda: _fir(x, np.zeros((17, 241), np.float32), 1, 0, 100), ValueError, "too many taps")     # 4097
    refused(lambda: _fir(x, h, 1, 0, 100, y_short=1), ValueError, "output rows overlap")
