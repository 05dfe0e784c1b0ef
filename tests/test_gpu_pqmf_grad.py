"""The PQMF adjoint kernels (rave_amd/csrc/pqmf_grad.hip) at their edges, called
through rave_amd._native at the C boundary against the restatements of
tests/pqmf_grad_ref.py (which tests/test_pqmf_grad_ref_host.py pins against the
forward restatements and torch autograd on the CPU); then the autograd surface
(torch.ops.rave_amd.pqmf_* and cc.CachedPQMF) and the end-to-end gradient of the
multi-resolution STFT loss down to the multiband tensor.

Every input is a strided view inside a NaN-filled buffer and every output a
view inside a NaN-filled buffer with guard rows and columns, as in
tests/test_gpu_filterbank.py; after each call the guards are still NaN and the
inputs are bit for bit what they were.

Bound: 4 e_ref, e_ref the max-abs error over the case's outputs of the
restatement's fp32 run (one chain in the kernel's documented order, the
epilogue factors formed in fp32) against its float64 run.  Where the fp32
arithmetic is exact (a unit cotangent leaves one non-zero product in the chain;
a zero cotangent; a rerun) values are compared for equality.

Measured on an MI355X (kernel error / e_ref, the worst case of each group;
DESIGN.md section 18):
Synthesis backward, t_in = 1 15 16 17 127 128 129 257, the worst of the modes
and forms: 1.53 1.19 1.00 1.00 1.10 1.02 1.00 1.00 (mode 0 is 1.00 throughout:
the MFMA chain is the fma chain; modes 1 and 2 carry expf and tanhf, and the
worst cases are mode 2); 511 frames on the remapped grid 1.00; the saturated
head 1.00.  Analysis backward: 1.00 in every case, both store paths, the
remapped grid and t_in = 1 included.  Unit cotangents return the taps, equal
values.  End to end (sc + mag down to the multiband tensor): 1.18 in max-abs
and 1.26 in relative L2 of e_ref (8.8e-4, 1.5e-3), 9.6e-6 of the bins clamped."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import filterbank_ref as R
from tests import pqmf_grad_ref as G
from tests.test_gpu_aux_kernels import DEV, guarded, maxerr, put, refused, report, same_bits, untouched

pytestmark = pytest.mark.gpu
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


def _held(what, got, ref, e_ref):
    """Print the figures, then assert 4 e_ref; returns kernel error / e_ref."""
    err = maxerr(got, ref)
    ratio = report(what, err, e_ref)
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), what
    assert err <= 4 * e_ref, (what, err, e_ref)
    return ratio


# ================================================================== 1. synthesis backward
def _syn_bwd(gy_np, x_np, noise_np, pad_left, mode, frame0, x_len, t_in, hki=None, precision=None,
             with_gnoise=None, null_x=False):
    """The kernel's stacked rows (B, rows, x_len or t_in) in pqmf_grad_ref.synthesis_backward's
    layout: gx, then gnoise when a noise is given.  gy_sb > 16 t_in, x_sc > x_len
    with NaN rows above the channels, gx and gnoise in guarded buffers."""
    N = _N()
    B = gy_np.shape[0]
    xl = x_len if x_len > 0 else t_in
    rows = 32 if mode == 1 else 16
    h = torch.from_numpy(_filters()[1] if hki is None else hki).to(DEV)
    gbuf, gy, _ = put(gy_np, [(0, 1), (3, 5)])
    xbuf = x = nbuf = nz = None
    if x_np is not None and not null_x:
        assert x_np.shape == (B, rows, xl)
        xbuf, x, _ = put(x_np, [(0, 1), (1, 2), (3, 4)])
    if noise_np is not None:
        nbuf, nz, _ = put(noise_np, [(0, 1), (2, 1), (1, 6)])
    obuf, gx, omask = guarded((B, rows, xl), [(0, 1), (1, 2), (2, 5)])
    with_gnoise = noise_np is not None if with_gnoise is None else with_gnoise
    qbuf = gn = qmask = None
    if with_gnoise:
        qbuf, gn, qmask = guarded((B, 16, xl), [(1, 0), (0, 3), (5, 2)])
    assert gy.stride(0) > 16 * t_in and gx.stride(1) > xl
    saved = [(b, b.clone()) for b in (gbuf, xbuf, nbuf, h) if b is not None]
    a = N.SynthesisBackwardArgs(
        n_band=16, taps=h.shape[2], batch=B, t_in=t_in, pad_left=pad_left, mode=mode, frame0=frame0, x_len=x_len,
        gy=gy.data_ptr(), gy_sb=gy.stride(0),
        x=None if x is None else x.data_ptr(), x_sb=0 if x is None else x.stride(0),
        x_sc=0 if x is None else x.stride(1),
        noise=None if nz is None else nz.data_ptr(), n_sb=0 if nz is None else nz.stride(0),
        n_sc=0 if nz is None else nz.stride(1),
        gx=gx.data_ptr(), gx_sb=gx.stride(0), gx_sc=gx.stride(1),
        gnoise=None if gn is None else gn.data_ptr(), gn_sb=0 if gn is None else gn.stride(0),
        gn_sc=0 if gn is None else gn.stride(1),
        hki=h.data_ptr(), precision=N.PREC_F32 if precision is None else precision)
    rc = N.lib.rave_pqmf_synthesis_backward(C.byref(a), _st())
    torch.cuda.synchronize()
    assert untouched(obuf, omask) and (qbuf is None or untouched(qbuf, qmask))
    assert all(same_bits(b, b0) for b, b0 in saved)
    if rc != N.RAVE_OK:
        assert bool(torch.isnan(obuf).all()) and (qbuf is None or bool(torch.isnan(qbuf).all()))
        return rc
    out = [gx] + ([gn] if gn is not None else [])
    return torch.cat(out, 1).cpu().numpy()


SYN_MODES = [(0, False), (1, True), (1, False), (2, True), (2, False)]           # (mode, noise given)
SYN_FORMS = [(16, None, 0), (0, 32, -32)]         # (pad_left, x_len - t_in or None for x_len = 0, frame0)


def _syn_inputs(rng, B, mode, xl, t_in, with_noise):
    gy = rng.standard_normal((B, 16 * t_in)).astype(np.float32)
    x = None if mode == 0 else rng.standard_normal((B, 32 if mode == 1 else 16, xl)).astype(np.float32)
    nz = (0.1 * rng.standard_normal((B, 16, xl))).astype(np.float32) if with_noise else None
    return gy, x, nz


def _syn_case(what, gy, x, nz, pad_left, mode, frame0, x_len, t_in):
    _, hki = _filters()
    ref, e_ref = R.with_e_ref(G.synthesis_backward, gy, x, hki, pad_left, mode, frame0, x_len, nz, t_in)
    got = _syn_bwd(gy, x, nz, pad_left, mode, frame0, x_len, t_in)
    return _held(what, got, ref, e_ref), got


@pytest.mark.parametrize("t_in", FRAME_COUNTS)
def test_synthesis_backward_vs_float64(t_in):
    """Modes 0, 1 and 2, with and without the noise (mode 0 with x = NULL), in
    the offline form (pad 16) and the cached one (pad 0, 32 history columns,
    frame0 = -32), B = 2, a random cotangent."""
    worst = 0.0
    for mi, (mode, with_noise) in enumerate(SYN_MODES):
        for fi, (pad_left, extra, frame0) in enumerate(SYN_FORMS):
            x_len = 0 if extra is None else t_in + extra
            gy, x, nz = _syn_inputs(np.random.default_rng(1000 * t_in + 10 * mi + fi), 2, mode, x_len or t_in, t_in,
                                    with_noise)
            what = f"synthesis backward t_in={t_in} mode={mode} noise={with_noise} pad={pad_left} x_len={x_len}"
            worst = max(worst, _syn_case(what, gy, x, nz, pad_left, mode, frame0, x_len, t_in)[0])
    print(f"synthesis backward t_in={t_in}: worst ratio {worst:.2f}")


def test_synthesis_backward_remapped_grid():
    """B = 2, 511 + 32 columns: 5 x 2 workgroups are not remapped, B = 2, 511
    frames offline: 4 x 2 = 8 workgroups, the grid xcd_major remaps."""
    for pad_left, extra, frame0 in ((16, None, 0), (0, 32, -31)):
        x_len = 0 if extra is None else 511 + extra
        gy, x, nz = _syn_inputs(np.random.default_rng(511 + pad_left), 2, 1, x_len or 511, 511, True)
        _syn_case(f"synthesis backward B=2 t_in=511 pad={pad_left}", gy, x, nz, pad_left, 1, frame0, x_len, 511)


def test_synthesis_backward_gnoise_is_optional():
    """gnoise = NULL with a noise given: gx is bit for bit the same."""
    gy, x, nz = _syn_inputs(np.random.default_rng(5), 2, 1, 129, 129, True)
    both = _syn_bwd(gy, x, nz, 16, 1, 0, 0, 129)
    only = _syn_bwd(gy, x, nz, 16, 1, 0, 0, 129, with_gnoise=False)
    assert only.shape[1] == 32 and np.array_equal(only.view(np.uint32), both[:, :32].view(np.uint32))


SYN_T = 257


@pytest.mark.parametrize("pad_left,x_extra", [(16, None), (0, 32)])
@pytest.mark.parametrize("frame0", [0, 7])
def test_synthesis_backward_unit_cotangents(frame0, pad_left, x_extra):
    """One row per cotangent sample 16 t + i: frames 0, the last, and round the
    workgroup boundary, phases 0, 6 and 15.  Column f meets tap f - t + pad_left,
    so every row holds taps 0 .. 32 (those that fall on a column): with the
    product's filter (tap 32 is its zero padding) and with a probe filter whose
    entries are all distinct and non-zero.  Mode 0: 16 x the tap, signed, equal
    values."""
    rng = np.random.default_rng(33)
    probe = rng.uniform(0.5, 1.5, (16, 16, 33)).astype(np.float32)
    probe = probe * np.where(rng.random(probe.shape) < 0.5, -1, 1).astype(np.float32)
    x_len = 0 if x_extra is None else SYN_T + x_extra
    xl = x_len or SYN_T
    spots = [16 * t + i for t in (0, 127, 128, 129, SYN_T - 1) for i in (0, 6, 15)]
    gy = np.zeros((len(spots), 16 * SYN_T), np.float32)
    for row, s in enumerate(spots):
        gy[row, s] = 1.0
    for hki in (_filters()[1], probe):
        want = np.stack([G.synthesis_backward_impulse(hki, s, pad_left, frame0, xl) for s in spots])
        assert np.abs(want).max() > 0 and (want < 0).any()
        # the first and the last tap both land on a column
        k = np.arange(xl)[None, :] - np.array([s // 16 for s in spots])[:, None] + pad_left
        assert (k == 0).any() and (k == 32).any()
        assert np.array_equal(G.synthesis_backward(gy, None, hki, pad_left, 0, frame0, x_len, None, SYN_T, np.float32),
                              want)
        got = _syn_bwd(gy, None, None, pad_left, 0, frame0, x_len, SYN_T, hki=hki)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_synthesis_backward_saturated_head():
    """Logits and carriers of +-40 in modes 1 and 2: finite, within the bound,
    and exactly zero wherever tanh's argument is beyond +-12 (1 - t^2 is 0 in
    fp32 from |u| of about 9)."""
    rng = np.random.default_rng(40)
    t_in = 129
    for mode, with_noise in ((1, True), (1, False), (2, True)):
        gy, x, nz = _syn_inputs(rng, 2, mode, t_in, t_in, with_noise)
        carrier = np.ascontiguousarray(x[:, :16])
        carrier.reshape(-1)[::3] = np.resize(np.array([40, -40], np.float32), carrier.reshape(-1)[::3].size)
        x[:, :16] = carrier
        if mode == 1:
            amp = np.ascontiguousarray(x[:, 16:])
            amp.reshape(-1)[::5] = np.resize(np.array([40, -40, 40], np.float32), amp.reshape(-1)[::5].size)
            x[:, 16:] = amp
        _, got = _syn_case(f"synthesis backward saturated mode={mode}", gy, x, nz, 16, mode, 0, 0, t_in)
        u = x[:, :16].astype(np.float64)
        if mode == 1:
            u = u / (1.0 + np.exp(-x[:, 16:].astype(np.float64)))
        u = u + (nz if with_noise else 0.0)
        flat = np.abs(u) > 12
        assert flat.sum() > 100
        gx, gn = G.split(got, mode, with_noise)
        assert not gx[:, :16][flat].any() and (mode != 1 or not gx[:, 16:][flat].any())
        assert gn is None or not gn[flat].any()


def test_synthesis_backward_zero_cotangent():
    for mode, with_noise in SYN_MODES:
        _, x, nz = _syn_inputs(np.random.default_rng(mode), 2, mode, 129 + 32, 129, with_noise)
        got = _syn_bwd(np.zeros((2, 16 * 129), np.float32), x, nz, 0, mode, -32, 129 + 32, 129)
        assert not got.any()


# ================================================================== 2. analysis backward
def _ana_bwd(gy_np, pad_left, t_in, hkf=None, aligned=False, precision=None, taps=None):
    """The kernel's (B, t_in) for gy (B, n_out, t_out): gy_sc > t_out, gx_sb > t_in;
    ``aligned`` puts every row of gx on a 16-byte boundary (the vector store),
    otherwise none is (the scalar tail)."""
    N = _N()
    B, n_out, t_out = gy_np.shape
    h = torch.from_numpy(_filters()[0] if hkf is None else hkf).to(DEV)
    gbuf, gy, _ = put(gy_np, [(0, 1), (1, 2), (3, 4)])
    obuf, gx, omask = guarded((B, t_in), [(0, 1), (4, 4 + (-t_in) % 4) if aligned else (3, 2 + (-t_in) % 4)])
    assert (gx.data_ptr() % 16 == 0 and gx.stride(0) % 4 == 0) if aligned else gx.data_ptr() % 16 != 0
    g0, h0 = gbuf.clone(), h.clone()
    a = N.AnalysisBackwardArgs(n_band=16, taps=h.shape[1] if taps is None else taps, n_out_bands=n_out, batch=B,
                               t_in=t_in, pad_left=pad_left, t_out=t_out,
                               precision=N.PREC_F32 if precision is None else precision,
                               gy=gy.data_ptr(), gy_sb=gy.stride(0), gy_sc=gy.stride(1),
                               gx=gx.data_ptr(), gx_sb=gx.stride(0), hkf=h.data_ptr())
    rc = N.lib.rave_pqmf_analysis_backward(C.byref(a), _st())
    torch.cuda.synchronize()
    assert untouched(obuf, omask) and same_bits(gbuf, g0) and same_bits(h, h0)
    if rc != N.RAVE_OK:
        assert bool(torch.isnan(obuf).all())
        return rc
    return gx.cpu().numpy()


def _ana_t_ins(pad_left, t_out):
    """16 t_out, and an input that stops 207 samples short of the last window."""
    return sorted({16 * t_out, max(1, 16 * (t_out - 1) + 513 - pad_left - 207)})


@pytest.mark.parametrize("t_out", FRAME_COUNTS)
def test_analysis_backward_vs_float64(t_out):
    """6 and 16 bands, the centred, causal and cached pads, t_in = 16 t_out and a
    short input off a multiple of 16 (t_in = 1 among them), B = 2, both store
    paths."""
    hkf, _ = _filters()
    worst = 0.0
    for n_out in (6, 16):
        for pad_left in (256, 512, 0):
            for t_in in _ana_t_ins(pad_left, t_out):
                rng = np.random.default_rng(100 * t_out + n_out + pad_left)
                gy = rng.standard_normal((2, n_out, t_out)).astype(np.float32)
                ref, e_ref = R.with_e_ref(G.analysis_backward, gy, hkf, pad_left, t_in, n_out)
                for aligned in (False, True):
                    got = _ana_bwd(gy, pad_left, t_in, aligned=aligned)
                    what = f"analysis backward t_out={t_out} n_out={n_out} pad={pad_left} t_in={t_in} aligned={aligned}"
                    worst = max(worst, _held(what, got, ref, e_ref))
    print(f"analysis backward t_out={t_out}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("t_out,t_in", [(511, 16 * 511), (511, 8000), (3, 1), (1, 1)])
def test_analysis_backward_remapped_grid_and_one_sample(t_out, t_in):
    """B = 2, 511 frames: 4 x 2 = 8 workgroups, the grid xcd_major remaps.  And
    t_in = 1: one output sample."""
    hkf, _ = _filters()
    for n_out, pad_left in ((6, 256), (16, 512), (16, 0)):
        gy = np.random.default_rng(t_in + n_out).standard_normal((2, n_out, t_out)).astype(np.float32)
        ref, e_ref = R.with_e_ref(G.analysis_backward, gy, hkf, pad_left, t_in, n_out)
        for aligned in (False, True):
            _held(f"analysis backward t_out={t_out} t_in={t_in} n_out={n_out} pad={pad_left} aligned={aligned}",
                  _ana_bwd(gy, pad_left, t_in, aligned=aligned), ref, e_ref)


ANA_T_OUT, ANA_T_IN = 257, 16 * 257


@pytest.mark.parametrize("pad_left", [256, 512, 0])
@pytest.mark.parametrize("n_out", [6, 16])
def test_analysis_backward_unit_cotangents(n_out, pad_left):
    """One row per unit cotangent (band, frame): frames of both parities, the
    first, the last and round the workgroup boundary (output column 128 =
    sample 2048).  The chain has one non-zero product, so the kernel returns
    the taps themselves, signed: equal values.  With the product's filter and
    with a probe filter whose 513 taps are all distinct and non-zero (the
    prototype's last tap is zero)."""
    rng = np.random.default_rng(513)
    probe = rng.uniform(0.5, 1.5, (16, 513)).astype(np.float32)
    probe = probe * np.where(rng.random((16, 513)) < 0.5, -1, 1).astype(np.float32)
    spots = [(k, t) for k in (0, 1, n_out - 1) for t in (0, 7, 128, 143, 144, ANA_T_OUT - 1)]
    gy = np.zeros((len(spots), n_out, ANA_T_OUT), np.float32)
    for row, (k, t) in enumerate(spots):
        gy[row, k, t] = 1.0
    for hkf in (_filters()[0], probe):
        want = np.stack([G.analysis_backward_impulse(hkf, k, t, pad_left, ANA_T_IN) for k, t in spots])
        if pad_left == 256:          # frame 128 meets every tap 0 .. 512 inside the input
            assert np.array_equal(want[2][16 * 128 - 256:16 * 128 + 257], hkf[0])
        assert np.array_equal(G.analysis_backward(gy, hkf, pad_left, ANA_T_IN, n_out, np.float32), want)
        for aligned in (False, True):
            got = _ana_bwd(gy, pad_left, ANA_T_IN, hkf=hkf, aligned=aligned)
            assert np.array_equal(got, want), (aligned, np.argwhere(got != want)[:8])


def test_analysis_backward_zero_cotangent():
    for n_out in (6, 16):
        assert not _ana_bwd(np.zeros((2, n_out, 129), np.float32), 256, 16 * 129 - 5).any()


# ================================================================== 3. reruns and refusals
def test_reruns_are_bitwise_equal():
    rng = np.random.default_rng(9)
    gy, x, nz = _syn_inputs(rng, 2, 1, 257 + 32, 257, True)
    a, b = (_syn_bwd(gy, x, nz, 0, 1, -31, 257 + 32, 257) for _ in range(2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ga = rng.standard_normal((2, 6, 257)).astype(np.float32)
    a, b = (_ana_bwd(ga, 256, 16 * 257 - 3) for _ in range(2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals():
    N = _N()
    gy, x, nz = _syn_inputs(np.random.default_rng(1), 1, 1, 32, 32, True)
    refused(lambda: _syn_bwd(gy, x, nz, 16, 1, 0, 0, 32, precision=N.PREC_SPLIT16), ValueError,
            "precision must be RAVE_PREC_F32")
    refused(lambda: _syn_bwd(gy, x, nz, 16, 1, 0, 0, 32, null_x=True), ValueError, "need the saved input x")
    refused(lambda: _syn_bwd(gy, np.ascontiguousarray(x[:, :16]), nz, 16, 3, 0, 0, 32), ValueError,
            "mode must be 0, 1 or 2")
    ga = np.zeros((1, 16, 32), np.float32)
    refused(lambda: _ana_bwd(ga, 256, 512, precision=N.PREC_SPLIT16), ValueError, "precision must be RAVE_PREC_F32")
    refused(lambda: _ana_bwd(ga, 250, 512), ValueError, "multiple of 16")
    refused(lambda: _ana_bwd(ga, 256, 512, taps=511), NotImplementedError, "513-tap")


# ================================================================== 4. the autograd surface
def _pqmf(cached=False):
    from rave_amd import cc
    from tests.conftest import GOLDEN
    cc.use_cached_conv(cached)
    try:
        return cc.CachedPQMF(hk=np.load(os.path.join(GOLDEN, "pqmf.npz"))["hk"]).to(DEV)
    finally:
        cc.use_cached_conv(False)


def test_new_symbols_and_ops_exist():
    N = _N()
    assert hasattr(N.lib, "rave_pqmf_synthesis_backward") and hasattr(N.lib, "rave_pqmf_analysis_backward")
    _pqmf()
    assert torch.ops.rave_amd.pqmf_synthesis_backward and torch.ops.rave_amd.pqmf_analysis_backward


@pytest.mark.parametrize("mode,with_noise", SYN_MODES)
def test_inverse_is_differentiable(mode, with_noise):
    """grad_fn, x.grad and noise.grad bit for bit the C boundary's results, and
    the output bit for bit the no-grad call's."""
    pq = _pqmf()
    F = 257
    gy, x, nz = _syn_inputs(np.random.default_rng(70 + mode), 2, mode, F, F, with_noise)
    if x is None:
        x = np.random.default_rng(7).standard_normal((2, 16, F)).astype(np.float32)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    nt = torch.from_numpy(nz).to(DEV).requires_grad_(True) if with_noise else None
    y = pq.inverse(xt, mode, nt)
    assert y.grad_fn is not None and y.shape == (2, 1, 16 * F)
    with torch.no_grad():
        y0 = pq.inverse(xt, mode, nt)
    y1 = pq.inverse(xt.detach(), mode, None if nt is None else nt.detach())
    assert y0.grad_fn is None and y1.grad_fn is None and same_bits(y0, y) and same_bits(y1, y)
    y.backward(torch.from_numpy(gy).to(DEV).reshape(2, 1, -1))
    want = _syn_bwd(gy, None if mode == 0 else x, nz, pq.pad_s, mode, 0, 0, F)
    gx, gn = G.split(want, mode, with_noise)
    assert np.array_equal(xt.grad.cpu().numpy().view(np.uint32), gx.view(np.uint32))
    if with_noise:
        assert np.array_equal(nt.grad.cpu().numpy().view(np.uint32), gn.view(np.uint32))


@pytest.mark.parametrize("n_out", [6, 16])
def test_forward_is_differentiable(n_out):
    pq = _pqmf()
    rng = np.random.default_rng(n_out)
    x = (0.5 * rng.standard_normal((2, 1, 16 * 257))).astype(np.float32)
    gy = rng.standard_normal((2, n_out, 257)).astype(np.float32)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = pq(xt, n_out)
    assert y.grad_fn is not None and y.shape == (2, n_out, 257)
    with torch.no_grad():
        y0 = pq(xt, n_out)
    assert y0.grad_fn is None and same_bits(y0, y) and same_bits(pq(xt.detach(), n_out), y)
    y.backward(torch.from_numpy(gy).to(DEV))
    want = _ana_bwd(gy, pq.pad_a, 16 * 257)
    assert np.array_equal(xt.grad[:, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_double_backward_and_other_precisions_raise():
    pq = _pqmf()
    x = torch.randn(2, 16, 64, device=DEV, requires_grad=True)
    with pytest.raises((NotImplementedError, RuntimeError), match="double backward"):
        torch.autograd.grad(pq.inverse(x).sum(), x, create_graph=True)
    a = torch.randn(2, 1, 1024, device=DEV, requires_grad=True)
    with pytest.raises((NotImplementedError, RuntimeError), match="double backward"):
        torch.autograd.grad(pq(a).sum(), a, create_graph=True)
    with pytest.raises(NotImplementedError, match="only the exact fp32 precision"):
        torch.ops.rave_amd.pqmf_synthesis(x, pq.hki, 16, 0, 0, 1, 0, None)
    with pytest.raises(NotImplementedError, match="only the exact fp32 precision"):
        torch.ops.rave_amd.pqmf_analysis(a, pq.hkf, 16, 256, 1)
    # without grad the split-f16 kernels run as before
    assert torch.ops.rave_amd.pqmf_synthesis(x.detach(), pq.hki, 16, 0, 0, 1, 0, None).grad_fn is None


def test_cached_mode_is_as_it_was():
    """The streaming form carries no grad_fn, and its blocks are bit for bit
    those of a module fed detached inputs (the same state history) and of the
    forward kernel on [history | block]."""
    from tests.test_gpu_filterbank import _synthesis
    x, noise = R.stream_signal()
    a, b = _pqmf(cached=True), _pqmf(cached=True)
    assert a.cached and b.cached
    for s, T, xb, nb in R.stream_blocks(x, noise):
        xt = torch.from_numpy(x[..., s:s + T]).to(DEV).contiguous()
        nt = torch.from_numpy(noise[..., s:s + T]).to(DEV).contiguous()
        ya = a.inverse(xt.clone().requires_grad_(True), 1, nt.clone().requires_grad_(True))
        yb = b.inverse(xt, 1, nt)
        assert ya.grad_fn is None and same_bits(ya, yb)
        want = _synthesis(xb, nb, 0, 1, -R.STREAM_HIST, R.STREAM_HIST + T, T, "f32")   # the module's frame0
        assert np.array_equal(ya[:, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    audio = torch.randn(2, 1, 2048, device=DEV)
    ya, yb = a(audio.clone().requires_grad_(True), 6), b(audio, 6)
    assert ya.grad_fn is None and same_bits(ya, yb)


# ================================================================== 5. end to end
E2E_FRAMES = 256


@functools.lru_cache(maxsize=None)
def _e2e_inputs():
    """A multiband tensor whose synthesis is close to tests/stft_loss_ref.py's
    case a prediction (so that, as there, nearly no bin of the reference sits
    under the power clamp): the bands of that prediction through the float64
    analysis restatement, pulled back through the head, tanh(x_w sigmoid(x_a) +
    noise), with random logits and a small noise."""
    from tests import stft_loss_ref as S
    hkf, _ = _filters()
    pred, target = S.mr_inputs("a")
    assert pred.shape == (2, 16 * E2E_FRAMES)
    rng = np.random.default_rng(2024)
    bands = R.analysis(pred, hkf, 256, E2E_FRAMES, 16)
    assert np.abs(bands).max() < 0.9
    xa = rng.standard_normal(bands.shape)
    noise = 0.01 * rng.standard_normal(bands.shape)
    xw = (np.arctanh(bands) - noise) * (1.0 + np.exp(-xa))
    y_mb = np.concatenate([xw, xa], 1).astype(np.float32)
    return y_mb, noise.astype(np.float32), target


@functools.lru_cache(maxsize=None)
def _e2e_ref():
    """CPU autograd of the oracle composition (oracle/torch_cpu.py's inverse
    behind the head in torch, tests/stft_loss_ref.py's loss): the float64
    gradient with respect to the multiband tensor, the fp32 one, and the share
    of clamped bins."""
    from tests import stft_loss_ref as S
    from tests.test_pqmf_grad_ref_host import _head, _oracle_inverse
    _, hki = _filters()
    y_mb, noise, target = _e2e_inputs()
    res = S.fork_resolutions(44100)
    out = {}
    for dtype in (torch.float64, torch.float32):
        v = torch.from_numpy(y_mb).to(dtype).requires_grad_(True)
        audio = _oracle_inverse(_head(v, 1, torch.from_numpy(noise).to(dtype)), torch.from_numpy(hki).to(dtype), False)
        sc, mag = S.mr_loss(audio, torch.from_numpy(target).to(dtype), res)
        (out[dtype],) = torch.autograd.grad(sc + mag, v)
        if dtype == torch.float64:
            out["share"] = S.clamped_share(audio.detach(), res)
    return out


def test_loss_gradient_reaches_the_multiband_tensor():
    """loss = sc + mag of MultiResolutionSTFTLoss.for_sample_rate(44100) on
    pqmf.inverse(y_mb, 1, noise)[:, 0]: y_mb.grad within 4 e_ref of the float64
    CPU gradient in max-abs and in relative L2, e_ref the CPU fp32 autograd
    gradient's error against it."""
    from rave_amd.distance import MultiResolutionSTFTLoss
    ref = _e2e_ref()
    assert ref["share"] < 1e-4, ref["share"]
    g64 = ref[torch.float64]

    def errs(g):
        d = g.double() - g64
        return float(d.abs().max()), float(d.norm() / g64.norm())
    e_abs, e_l2 = errs(ref[torch.float32])
    y_mb, noise, target = _e2e_inputs()
    pq = _pqmf()
    v = torch.from_numpy(y_mb).to(DEV).requires_grad_(True)
    audio = pq.inverse(v, 1, torch.from_numpy(noise).to(DEV))[:, 0]
    assert audio.shape == (2, 4096)
    loss = sum(MultiResolutionSTFTLoss.for_sample_rate(44100)(audio, torch.from_numpy(target).to(DEV)))
    loss.backward()
    k_abs, k_l2 = errs(v.grad.cpu())
    print(f"end to end: clamped share {ref['share']:.2e}; e_ref max-abs {e_abs:.3e} L2 {e_l2:.3e}; "
          f"kernel {k_abs:.3e} {k_l2:.3e}; ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
    assert bool(torch.isfinite(v.grad).all())
    assert k_abs <= 4 * e_abs and k_l2 <= 4 * e_l2
