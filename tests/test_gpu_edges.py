"""The fused path edges (csrc/edge_split.hip) against the float64 oracle and
against the separate ops they replace.

* rave_encoder_head = CachedPQMF.forward + band slice (rave/pqmf.py:269-273,
  rave/model.py:613) -> EncoderV2's first conv (rave/blocks.py:533-536), + the
  speaker concat (rave/model.py:618-620);
* rave_decoder_tail = GeneratorV2's act -> conv -> `x*sigmoid(a) (+noise) ->
  tanh` (rave/blocks.py:691-707) -> CachedPQMF.inverse (rave/pqmf.py:275-284).

Tolerances: layer outputs 2e-5 relative to max|ref| (as the single-layer tests);
model outputs 1e-4 max-abs (north star).  Ragged lengths (frames not a
multiple of the 256-frame tiles) and both padding modes are covered, in both
arithmetics: split-f16 and exact fp32 (precision RAVE_PREC_F32_RING: the
ring weight image and the fp32 filter image).
The tile, halo and option edges, against e_ref: tests/test_gpu_edge_sweep.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def N():
    from rave_amd import _native
    return _native


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _filters(golden):
    from oracle.rave_oracle import pqmf_filters
    hk = golden("pqmf")["hk"]
    return pqmf_filters(hk)


HEAD_CASES = [(600, 2, 1.0, 6), (4096, 3, 1.0, 6), (257, 1, 3e6, 6),
              (600, 2, 1.0, 5), (600, 1, 1.0, 8)]     # odd / full band counts: the fp32 conv's channel pairs


@pytest.mark.parametrize("prec", ["split16", "f32_ring", "bf16x3"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("F,B,scale,nb", HEAD_CASES)
def test_encoder_head(N, dev, golden, causal, F, B, scale, nb, prec):
    """bf16x3 (round 6): the analysis on the bf16 matrix cores (filter and audio
    split exactly into three bf16 parts), the conv in exact fp32 on the ring
    image; held to the fp32-class bound as the bf16x3 tail."""
    from oracle.rave_oracle import conv1d, get_padding, reverse_half
    hkf, _ = _filters(golden)
    rng = np.random.default_rng(F + 7 * causal + nb)
    T = 16 * F
    x = (scale * (0.3 * np.sin(np.arange(T) * 0.05)[None, None] + 0.1 * rng.standard_normal((B, 1, T)))).astype(np.float32)
    co, k = 64, 7
    w = (rng.uniform(-1, 1, (co, nb, k)) / np.sqrt(nb * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(co)).astype(np.float32)
    bands = reverse_half(conv1d(x.astype(np.float64), hkf.astype(np.float64), None, stride=16,
                                pad=get_padding(hkf.shape[-1], causal=causal)))[:, :nb]
    cpad = get_padding(k, causal=causal)
    ref = conv1d(bands, w.astype(np.float64), b.astype(np.float64), pad=cpad)
    P = N.PRECISION[prec]
    wprec = N.PREC_F32_RING if P == N.PREC_BF16X3 else P      # the bf16x3 head's conv: exact fp32, ring image
    packed = torch.from_numpy(N.pack_conv_weight(w, nb, co, k, 1, 1, 0, precision=wprec)).to(dev)
    xd = torch.from_numpy(x).to(dev)
    y = torch.full((B, co, F), float("nan"), device=dev)
    spk = torch.from_numpy(rng.standard_normal(256).astype(np.float32)).to(dev)
    Fz = max(1, F // 64)
    z = torch.full((B, 320, Fz), float("nan"), device=dev)
    hd = torch.from_numpy(N.pack_edge_filter(hkf, head=True, n_out_bands=nb,
                                             f32=P in (N.PREC_F32_RING, N.PREC_BF16X3))).to(dev)
    bd = torch.from_numpy(b).to(dev)
    a = N.EdgeArgs(batch=B, frames=F, conv_c_in=nb, conv_c_out=co, conv_kernel=k, conv_pad_left=cpad[0],
                   pqmf_taps=hkf.shape[-1], pqmf_pad_left=get_padding(hkf.shape[-1], causal=causal)[0],
                   x=xd.data_ptr(), x_sb=T, y=y.data_ptr(), y_sb=co * F, y_sc=F,
                   weight=packed.data_ptr(), bias=bd.data_ptr(), filter=hd.data_ptr(),
                   fill_channels=256, fill_t=Fz, fill_y=z[:, 64:].data_ptr(), f_sb=320 * Fz, f_sc=Fz,
                   fill_values=spk.data_ptr(), precision=P)
    N.check(N.lib.rave_encoder_head(C.byref(a), _st()), "encoder_head")
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    err = maxabs(got, ref)
    assert err <= 2e-5 * float(np.abs(ref).max()), err
    if prec == "bf16x3":                   # fp32-class arithmetic
        assert err <= 2e-6 * max(1.0, float(np.abs(ref).max())), err
    zz = z.cpu().numpy()
    assert np.array_equal(zz[:, 64:], np.broadcast_to(spk.cpu().numpy()[None, :, None], (B, 256, Fz)))
    assert np.isnan(zz[:, :64]).all()            # the latent rows are the encoder's, untouched


@pytest.mark.parametrize("prec", ["split16", "f32_ring", "bf16x3"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("am,act,noise", [(True, "leaky", False), (False, "snake", True), (True, "snake", True)])
@pytest.mark.parametrize("F,B", [(600, 2), (4096, 2), (100, 1)])
def test_decoder_tail(N, dev, golden, causal, am, act, noise, F, B, prec):
    from oracle.rave_oracle import conv1d, get_padding, leaky_relu, reverse_half, snake
    _, hki = _filters(golden)
    rng = np.random.default_rng(F + 3 * am + 5 * causal)
    ci, k = 64, 7
    co = 32 if am else 16
    x = rng.standard_normal((B, ci, F)).astype(np.float32)
    w = (rng.uniform(-1, 1, (co, ci, k)) / np.sqrt(ci * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(co)).astype(np.float32)
    alpha = (1 + 0.1 * rng.standard_normal(ci)).astype(np.float32)
    nz = (0.05 * rng.standard_normal((B, 16, F))).astype(np.float32) if noise else None
    xa = leaky_relu(x.astype(np.float64)) if act == "leaky" else snake(x.astype(np.float64), alpha.reshape(-1, 1))
    cpad = get_padding(k, causal=causal)
    wv = conv1d(xa, w.astype(np.float64), b.astype(np.float64), pad=cpad)
    if am:
        v, amp = np.split(wv, 2, axis=1)
        wv = v * (1.0 / (1.0 + np.exp(-amp)))
    wv = np.tanh(wv + (nz if noise else 0.0))
    spad = get_padding(hki.shape[-1], causal=causal)
    ys = conv1d(reverse_half(wv), hki.astype(np.float64), None, pad=spad) * 16
    ref = ys[:, ::-1, :].transpose(0, 2, 1).reshape(B, 1, F * 16)
    P = N.PRECISION[prec]
    packed = torch.from_numpy(N.pack_conv_weight(w, ci, co, k, 1, 1, 0, precision=P)).to(dev)
    xd = torch.from_numpy(x).to(dev)
    y = torch.full((B, 1, 16 * F), float("nan"), device=dev)
    bd, ad = (torch.from_numpy(v).to(dev) for v in (b, alpha))
    # (bf16x3: the conv on the bf16 matrix cores, the synthesis on the exact-fp32 filter image)
    hd = torch.from_numpy(N.pack_edge_filter(hki, head=False, f32=P in (N.PREC_F32_RING, N.PREC_BF16X3))).to(dev)
    nd = torch.from_numpy(nz).to(dev) if noise else None
    a = N.EdgeArgs(batch=B, frames=F, conv_c_in=ci, conv_c_out=co, conv_kernel=k, conv_pad_left=cpad[0],
                   pqmf_taps=hki.shape[-1], pqmf_pad_left=spad[0], mode=1 if am else 2, act=N.ACT[act],
                   leaky_slope=0.2, x=xd.data_ptr(), x_sb=ci * F, x_sc=F, y=y.data_ptr(), y_sb=16 * F,
                   weight=packed.data_ptr(), bias=bd.data_ptr(), alpha=ad.data_ptr(), filter=hd.data_ptr(),
                   noise=nd.data_ptr() if noise else None, n_sb=16 * F, n_sc=F, precision=P)
    N.check(N.lib.rave_decoder_tail(C.byref(a), _st()), "decoder_tail")
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    err = maxabs(got, ref)
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), err
    if prec != "split16":                  # fp32-class arithmetics
        assert err <= 2e-6 * max(1.0, float(np.abs(ref).max())), err


def _views():
    from tests.test_gpu_aux_kernels import guarded, put, same_bits, untouched
    return guarded, put, same_bits, untouched


@pytest.mark.parametrize("prec", ["split16", "f32_ring", "bf16x3"])
def test_encoder_head_on_guarded_views(N, dev, golden, prec):
    """The head on views inside NaN-filled buffers: x_sb wider than the audio,
    y_sc > frames and y_sb > 64 y_sc, once with rows the 16-byte stores can
    take (y and both strides multiples of 4 floats) and once with rows they
    cannot (the scalar stores); ragged F = 257, B = 2.  The file's bounds; the
    guards still NaN and the input unchanged afterwards."""
    from oracle.rave_oracle import conv1d, get_padding, reverse_half
    guarded, put, same_bits, untouched = _views()
    hkf, _ = _filters(golden)
    F, B, nb, co, k, causal = 257, 2, 6, 64, 7, False
    rng = np.random.default_rng(F)
    T = 16 * F
    x = (0.3 * np.sin(np.arange(T) * 0.05)[None] + 0.1 * rng.standard_normal((B, T))).astype(np.float32)
    w = (rng.uniform(-1, 1, (co, nb, k)) / np.sqrt(nb * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(co)).astype(np.float32)
    ppad = get_padding(hkf.shape[-1], causal=causal)
    bands = reverse_half(conv1d(x[:, None].astype(np.float64), hkf.astype(np.float64), None, stride=16, pad=ppad))[:, :nb]
    cpad = get_padding(k, causal=causal)
    ref = conv1d(bands, w.astype(np.float64), b.astype(np.float64), pad=cpad)
    P = N.PRECISION[prec]
    wprec = N.PREC_F32_RING if P == N.PREC_BF16X3 else P
    packed = torch.from_numpy(N.pack_conv_weight(w, nb, co, k, 1, 1, 0, precision=wprec)).to(dev)
    hd = torch.from_numpy(N.pack_edge_filter(hkf, head=True, n_out_bands=nb,
                                             f32=P in (N.PREC_F32_RING, N.PREC_BF16X3))).to(dev)
    bd = torch.from_numpy(b).to(dev)
    xbuf, xd, _ = put(x, [(0, 1), (5, 3)])
    x0 = xbuf.clone()
    for ypads in ([(0, 1), (1, 2), (4, 3)], [(0, 1), (1, 2), (2, 3)]):      # y_sc = 264 (vector stores), 262 (scalar)
        ybuf, y, ymask = guarded((B, co, F), ypads)
        assert xd.stride(0) > T and y.stride(1) > F and y.stride(0) > co * y.stride(1)
        a = N.EdgeArgs(batch=B, frames=F, conv_c_in=nb, conv_c_out=co, conv_kernel=k, conv_pad_left=cpad[0],
                       pqmf_taps=hkf.shape[-1], pqmf_pad_left=ppad[0],
                       x=xd.data_ptr(), x_sb=xd.stride(0), x_sc=xd.stride(0), y=y.data_ptr(), y_sb=y.stride(0),
                       y_sc=y.stride(1), weight=packed.data_ptr(), bias=bd.data_ptr(), filter=hd.data_ptr(),
                       precision=P)
        N.check(N.lib.rave_encoder_head(C.byref(a), _st()), "encoder_head")
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert np.isfinite(got).all()
        err = maxabs(got, ref)
        assert err <= 2e-5 * float(np.abs(ref).max()), (ypads, err)
        if prec == "bf16x3":
            assert err <= 2e-6 * max(1.0, float(np.abs(ref).max())), (ypads, err)
        assert untouched(ybuf, ymask) and same_bits(xbuf, x0)


@pytest.mark.parametrize("prec", ["split16", "f32_ring", "bf16x3"])
def test_decoder_tail_on_guarded_views(N, dev, golden, prec):
    """The tail on views inside NaN-filled buffers: x_sc > frames with NaN rows
    round the 64 channels, the noise likewise, y_sb > 16 frames (16-byte aligned,
    as the launcher requires; the unaligned view is refused cleanly); ragged
    F = 257, B = 2, amplitude modulation + noise, Snake."""
    from oracle.rave_oracle import conv1d, get_padding, reverse_half, snake
    guarded, put, same_bits, untouched = _views()
    _, hki = _filters(golden)
    F, B, ci, co, k, causal = 257, 2, 64, 32, 7, True
    rng = np.random.default_rng(F + 1)
    x = rng.standard_normal((B, ci, F)).astype(np.float32)
    w = (rng.uniform(-1, 1, (co, ci, k)) / np.sqrt(ci * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(co)).astype(np.float32)
    alpha = (1 + 0.1 * rng.standard_normal(ci)).astype(np.float32)
    nz = (0.05 * rng.standard_normal((B, 16, F))).astype(np.float32)
    cpad = get_padding(k, causal=causal)
    wv = conv1d(snake(x.astype(np.float64), alpha.reshape(-1, 1)), w.astype(np.float64), b.astype(np.float64), pad=cpad)
    v, amp = np.split(wv, 2, axis=1)
    wv = np.tanh(v * (1.0 / (1.0 + np.exp(-amp))) + nz)
    spad = get_padding(hki.shape[-1], causal=causal)
    ys = conv1d(reverse_half(wv), hki.astype(np.float64), None, pad=spad) * 16
    ref = ys[:, ::-1, :].transpose(0, 2, 1).reshape(B, F * 16)
    P = N.PRECISION[prec]
    packed = torch.from_numpy(N.pack_conv_weight(w, ci, co, k, 1, 1, 0, precision=P)).to(dev)
    hd = torch.from_numpy(N.pack_edge_filter(hki, head=False, f32=P in (N.PREC_F32_RING, N.PREC_BF16X3))).to(dev)
    bd, ad = (torch.from_numpy(t).to(dev) for t in (b, alpha))
    xbuf, xd, _ = put(x, [(0, 1), (1, 2), (3, 4)])
    nbuf, nd, _ = put(nz, [(0, 1), (2, 1), (1, 6)])
    x0, n0 = xbuf.clone(), nbuf.clone()

    def call(ypads):
        ybuf, y, ymask = guarded((B, 16 * F), ypads)
        assert xd.stride(1) > F and nd.stride(1) > F and y.stride(0) > 16 * F
        a = N.EdgeArgs(batch=B, frames=F, conv_c_in=ci, conv_c_out=co, conv_kernel=k, conv_pad_left=cpad[0],
                       pqmf_taps=hki.shape[-1], pqmf_pad_left=spad[0], mode=1, act=N.ACT["snake"], leaky_slope=0.2,
                       x=xd.data_ptr(), x_sb=xd.stride(0), x_sc=xd.stride(1), y=y.data_ptr(), y_sb=y.stride(0),
                       weight=packed.data_ptr(), bias=bd.data_ptr(), alpha=ad.data_ptr(), filter=hd.data_ptr(),
                       noise=nd.data_ptr(), n_sb=nd.stride(0), n_sc=nd.stride(1), precision=P)
        rc = N.lib.rave_decoder_tail(C.byref(a), _st())
        torch.cuda.synchronize()
        assert untouched(ybuf, ymask) and same_bits(xbuf, x0) and same_bits(nbuf, n0)
        return rc, ybuf, y

    for ypads in ([(0, 1), (5, 7)], [(0, 1), (4, 9)]):                       # y off 16 bytes; y_sb % 4 != 0
        rc, ybuf, _ = call(ypads)
        assert rc == N.RAVE_ERR_ARG and "16-byte aligned" in N.lib.rave_last_error().decode()
        assert bool(torch.isnan(ybuf).all())
    rc, _, y = call([(0, 1), (4, 8)])
    N.check(rc, "decoder_tail")
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    err = maxabs(got, ref)
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), err
    if prec != "split16":
        assert err <= 2e-6 * max(1.0, float(np.abs(ref).max())), err


def test_edges_refuse_unsupported(N):
    a = N.EdgeArgs(batch=1, frames=64, conv_c_in=96, conv_c_out=32, conv_kernel=7, pqmf_taps=33, mode=1,
                   act=N.ACT["leaky"], x=16, y=16, weight=16, filter=16)
    assert N.lib.rave_decoder_tail(C.byref(a), None) == N.RAVE_ERR_UNSUPPORTED     # capacity 96 (discrete)
    a = N.EdgeArgs(batch=1, frames=64, conv_c_in=16, conv_c_out=64, conv_kernel=7, pqmf_taps=513, x=16, y=16,
                   weight=16, filter=16)
    assert N.lib.rave_encoder_head(C.byref(a), None) == N.RAVE_ERR_UNSUPPORTED     # > 8 bands


@pytest.mark.parametrize("cfg_name,precision", [("v2", "split16"), ("v3_noise", "split16"), ("v2", "f32_tuned"),
                                                ("v3_noise", "f32_tuned"), ("v2", "f32_bf3"),
                                                ("v3_noise", "f32_bf3")])
def test_model_uses_edges_and_matches_oracle(dev, golden, cfg_name, precision):
    """A split16 model lays both fused edges into its plans (an exact-fp32
    f32_tuned model: where they time faster than the separate ops), and its
    forward matches the float64 oracle (the model golden tests cover auto /
    split16 against the reference fixtures)."""
    from oracle.rave_oracle import Oracle
    from rave_amd import _native as N
    from rave_amd import config as rcfg
    from rave_amd.model import DECODE, ENCODE, RAVE
    from rave_amd.weights import init_params, init_speaker
    cfg = rcfg.get_config(cfg_name)
    params = init_params(cfg, seed=3)
    spk = init_speaker(cfg, seed=3)
    m = RAVE(cfg, params, spk, device=dev, hk=golden("pqmf")["hk"], precision=precision)
    B, T = 2, 16384
    Fz = T // cfg.hop
    kinds_e = [o["kind"] for o in m.ops(ENCODE, B, T)]
    kinds_d = [o["kind"] for o in m.ops(DECODE, B, Fz)]
    if precision == "split16":
        assert N.OP_HEAD in kinds_e and N.OP_PQMF_ANALYSIS not in kinds_e and N.OP_FILL not in kinds_e
        assert N.OP_TAIL in kinds_d and N.OP_PQMF_SYNTHESIS not in kinds_d
    else:
        assert (N.OP_HEAD in kinds_e) != (N.OP_PQMF_ANALYSIS in kinds_e)
        assert (N.OP_TAIL in kinds_d) != (N.OP_PQMF_SYNTHESIS in kinds_d)
    rng = np.random.default_rng(4)
    x = (0.3 * np.sin(np.arange(T) * 2 * np.pi * 440 / 48000)[None, None]
         + 0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)
    o = Oracle(cfg, params, spk, hk=golden("pqmf")["hk"])
    z = m.encode(torch.from_numpy(x).to(dev))
    assert maxabs(z.cpu().numpy(), o.encode(x.astype(np.float64))) <= 1e-4
    noise_u = None
    if cfg.noise is not None:
        noise_u = torch.from_numpy(rng.uniform(0, 1, m.noise_shape(B, Fz)).astype(np.float32)).to(dev)
    y = m.decode(z, noise_u=noise_u)
    ref = o.decode(z.cpu().numpy().astype(np.float64),
                   noise_u=noise_u.cpu().numpy().astype(np.float64) if noise_u is not None else None)
    assert maxabs(y.cpu().numpy(), ref) <= 1e-4
