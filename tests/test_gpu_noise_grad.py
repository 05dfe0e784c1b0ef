"""The backwards of the noise filter stage and of eval-mode AdaIN
(rave_noise_synth_backward in rave_amd/csrc/noise.hip, rave_adain_backward in
adain.hip): at the C boundary against the float64 closed forms of
tests/noise_grad_ref.py (which tests/test_noise_grad_ref_host.py checks against
float64 torch autograd on the CPU), then through torch.ops.rave_amd.noise_synth
/ adain under autograd, through a GeneratorV2 with AdaIN and the noise module,
and through RAVEModules(v3_noise) from the spectral loss back to every
parameter.

The helpers and the pattern are tests/test_gpu_aux_kernels.py's: outputs inside
NaN-filled guarded buffers, inputs as strided views of NaN-filled buffers, the
surroundings untouched, the inputs unchanged.

Bounds: 4 e_ref on max-abs, e_ref the fp32 CPU run of the closed form against
its float64 run on the same input.  The identity cases of AdaIN are compared
bitwise.  The module tree is held to 1e-3 of each gradient's max against fp32
torch autograd of the same tree in plain torch on the same GPU (the plumbing
bound of tests/test_gpu_convt_grad.py; the kernels' own bounds are the ones
above).

Measured on an MI355X (kernel error / e_ref):
Noise backward, frames 1 / 127 / 128 / 129: (5, 8) 2.50 0.88 0.63 1.36, (5, 16)
0.55 1.18 1.00 0.98, (9, 16) 1.16 1.04 1.06 1.36; amp in [20, 30] (gradients of
1e-9 and below, e_ref 3e-13): 1.63 1.00 1.26.  Through autograd (frames 129): 1.36
0.98 1.36, the C boundary's bits.
AdaIN backward, every transferring case of t_len 1 / 2 / 255 / 256 / 257: 1.00 (one
correctly rounded division and one product, as the fp32 CPU run does them); through
autograd 1.00.
Module tree, the worst err / max over z and the parameters: train() 1.7e-6, eval()
3.2e-6 (bound 1e-3); the noise branch's share of the trailing Snake's alpha gradient
0.11 of 1.59 in train(), 1.78 of 4.58 in eval()."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import noise_grad_ref as G
from tests.test_gpu_aux_kernels import (ADA_B, ADA_C, ADA_MB, DEV, NAN, _N, _st, guarded, maxerr, put, ratio_of,
                                        refused, report, same_bits, untouched)

pytestmark = pytest.mark.gpu
N_BAND, NOISE_B = 3, 2


# ================================================================== 1. noise backward at the C boundary
def _noise_bwd_call(amp, u, gy, gamp, n_band, nb, tgt, frames):
    N = _N()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    a = N.NoiseBackwardArgs(batch=amp.shape[0] if amp is not None else NOISE_B, frames=frames, n_band=n_band,
                            noise_bands=nb, target=tgt, amp=ptr(amp), u=ptr(u), gy=ptr(gy), gamp=ptr(gamp))
    if amp is not None:
        a.a_sb, a.a_sc = amp.stride(0), amp.stride(1)
    if u is not None:
        a.u_sb = u.stride(0)
    if gy is not None:
        a.gy_sb, a.gy_sc = gy.stride(0), gy.stride(1)
    if gamp is not None:
        a.ga_sb, a.ga_sc = gamp.stride(0), gamp.stride(1)
    return N.lib.rave_noise_synth_backward(C.byref(a), _st())


def _noise_inputs(nb, tgt, frames, lo_hi=None):
    rng = np.random.default_rng(1000 * nb + 10 * tgt + frames + (7 if lo_hi else 0))
    shape = (NOISE_B, N_BAND * nb, frames)
    if lo_hi is None:
        amp = (rng.standard_normal(shape) * 3 + 4).astype(np.float32)          # N(4, 3): both tails of the sigmoid
    else:
        amp = rng.uniform(*lo_hi, shape).astype(np.float32)
    u = rng.uniform(0, 1, (NOISE_B, frames, N_BAND, tgt)).astype(np.float32)
    gy = rng.standard_normal((NOISE_B, N_BAND, frames * tgt)).astype(np.float32)
    return amp, u, gy


def _noise_bwd(amp_np, u_np, gy_np, nb, tgt, frames):
    """The kernel's gamp on strided inputs, guards and inputs checked."""
    N = _N()
    abuf, amp, _ = put(amp_np, [(0, 0), (1, 1), (2, 3)])
    ubuf = torch.full((NOISE_B, u_np[0].size + 5), NAN, device=DEV)           # a batch stride above the row
    ubuf[:, :u_np[0].size] = torch.from_numpy(u_np.reshape(NOISE_B, -1)).to(DEV)
    gbuf, gy, _ = put(gy_np, [(0, 0), (1, 1), (3, 4)])                        # rows off any 16-byte alignment
    obuf, gamp, omask = guarded(amp_np.shape, [(0, 0), (1, 1), (3, 2)])
    a0, u0, g0 = abuf.clone(), ubuf.clone(), gbuf.clone()
    N.check(_noise_bwd_call(amp, ubuf, gy, gamp, N_BAND, nb, tgt, frames))
    torch.cuda.synchronize()
    assert untouched(obuf, omask) and same_bits(abuf, a0) and same_bits(ubuf, u0) and same_bits(gbuf, g0)
    return gamp.cpu()


def _noise_held(what, got, amp_np, u_np, gy_np, nb, tgt):
    want = G.noise_synth_backward(gy_np, amp_np, u_np, N_BAND, nb, tgt)
    e_ref = maxerr(G.noise_synth_backward(gy_np, amp_np, u_np, N_BAND, nb, tgt, np.float32), want)
    err = maxerr(got, want)
    report(what, err, e_ref)
    assert np.abs(want).max() > 0 and err <= 4 * e_ref, (what, err, e_ref)


@pytest.mark.parametrize("frames", [1, 127, 128, 129])
@pytest.mark.parametrize("nb,tgt", G.PAIRS)
def test_noise_backward_all_pairs_vs_float64(nb, tgt, frames):
    """Every compiled pair at frame counts round the 128-thread block."""
    amp, u, gy = _noise_inputs(nb, tgt, frames)
    _noise_held(f"noise backward ({nb}, {tgt}) frames {frames}", _noise_bwd(amp, u, gy, nb, tgt, frames), amp, u, gy,
                nb, tgt)


@pytest.mark.parametrize("nb,tgt", G.PAIRS)
def test_noise_backward_large_amp_keeps_its_digits(nb, tgt):
    """amp in [20, 30]: 1 - s = e^-(amp - 5) to fp32's relative precision only if it is not
    taken by subtraction from s, which rounds to 1 there."""
    amp, u, gy = _noise_inputs(nb, tgt, 129, (20.0, 30.0))
    got = _noise_bwd(amp, u, gy, nb, tgt, 129)
    assert float(got.abs().max()) > 0
    _noise_held(f"noise backward ({nb}, {tgt}) amp in [20, 30]", got, amp, u, gy, nb, tgt)


# ================================================================== 2. reproducibility
@pytest.mark.parametrize("nb,tgt", G.PAIRS)
def test_noise_backward_is_reproducible_and_zero_in_zero_out(nb, tgt):
    amp, u, gy = _noise_inputs(nb, tgt, 129)
    first, second = _noise_bwd(amp, u, gy, nb, tgt, 129), _noise_bwd(amp, u, gy, nb, tgt, 129)
    assert same_bits(first, second)
    zero = _noise_bwd(amp, u, np.zeros_like(gy), nb, tgt, 129)
    assert bool((zero == 0).all())


# ================================================================== 3. refusals
def test_noise_backward_refusals():
    amp = torch.zeros(1, 3 * 9, 4, device=DEV)
    u = torch.zeros(1, 4, 3, 16, device=DEV)
    gy = torch.zeros(1, 3, 64, device=DEV)
    gamp = torch.full((1, 3 * 9, 4), NAN, device=DEV)
    call = lambda nb, tgt, **kw: _noise_bwd_call(kw.get("amp", amp), kw.get("u", u), kw.get("gy", gy),
                                                 kw.get("gamp", gamp), 3, nb, tgt, 4)
    refused(lambda: call(9, 8), ValueError, "target must be >= 2*(noise_bands-1)")
    refused(lambda: call(5, 7), ValueError, "target must be >= 2*(noise_bands-1)")
    refused(lambda: call(5, 12), NotImplementedError, "supported (noise_bands, target)")
    refused(lambda: call(7, 16), NotImplementedError, "supported (noise_bands, target)")
    for name in ("gy", "gamp", "amp", "u"):
        refused(lambda: call(9, 16, **{name: None}), ValueError, "null pointer")
    refused(lambda: _noise_bwd_call(amp, u, gy, gamp, 3, 9, 16, 0), ValueError, "empty shape")
    torch.cuda.synchronize()
    assert bool(torch.isnan(gamp).all())


# ================================================================== 4. AdaIN backward at the C boundary
def _adain_bwd_call(gy, gx, stats, counters, mode, row0, max_batch=ADA_MB, shape=None):
    N = _N()
    B, Cc, T = shape if shape is not None else gy.shape
    ptr = lambda t: 0 if t is None else t.data_ptr()
    a = N.AdainBackwardArgs(batch=B, channels=Cc, t_len=T, mode=mode, max_batch=max_batch, row0=row0,
                            gy=ptr(gy), gx=ptr(gx), stats=ptr(stats), counters=ptr(counters))
    if gy is not None:
        a.gy_sb, a.gy_sc = gy.stride(0), gy.stride(1)
    if gx is not None:
        a.gx_sb, a.gx_sc = gx.stride(0), gx.stride(1)
    return N.lib.rave_adain_backward(C.byref(a), _st())


def _ada_stats(rng):
    st = rng.standard_normal((4, ADA_MB, ADA_C)).astype(np.float32)
    st[1], st[3] = np.abs(st[1]) + 0.1, np.abs(st[3]) + 0.1
    return st


@pytest.mark.parametrize("t_len", [1, 2, 255, 256, 257])
def test_adain_backward_modes_counters_rows_and_aliasing(t_len):
    """Modes 0 / 1 / 2 with the counters (as the forward left them) (0, 0), (1, 0), (0, 1) and
    (3, 2), at row0 0 and 4, gx aliased to gy and as a separate strided buffer: the transferred
    rows within 4 e_ref of the float64 closed form, every other case bitwise gy; the statistics
    and counters unchanged."""
    N = _N()
    rng = np.random.default_rng(t_len)
    st_np = _ada_stats(rng)
    worst, n_transfer = 0.0, 0
    for mode in (0, 1, 2):
        for cnt in ([0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [3.0, 2.0]):
            for row0 in (0, 4):
                for alias in (True, False):
                    stats, counters = torch.from_numpy(st_np).to(DEV), torch.tensor(cnt, device=DEV)
                    gy_np = rng.standard_normal((ADA_B, ADA_C, t_len)).astype(np.float32)
                    gbuf, gy, _ = put(gy_np, [(0, 1), (1, 2), (3, 2)])
                    if alias:
                        obuf, gx, omask = gbuf, gy, None
                    else:
                        obuf, gx, omask = guarded(gy_np.shape, [(1, 0), (0, 3), (2, 5)])
                    g0 = gbuf.clone()
                    N.check(_adain_bwd_call(gy, gx, stats, counters, mode, row0))
                    torch.cuda.synchronize()
                    assert same_bits(stats.cpu(), torch.from_numpy(st_np)) and counters.cpu().tolist() == cnt
                    transfer = G.adain_transfers(cnt, mode)
                    assert transfer == (mode != 2 and cnt == [3.0, 2.0])
                    if transfer:
                        n_transfer += 1
                        want = G.adain_backward(gy_np, st_np, cnt, mode, row0)
                        e_ref = maxerr(G.adain_backward(gy_np, st_np, cnt, mode, row0, np.float32), want)
                        err = maxerr(gx, want)
                        worst = max(worst, ratio_of(err, e_ref))
                        assert err <= 4 * e_ref, (mode, cnt, row0, alias, err, e_ref)
                    else:
                        assert same_bits(gx.cpu(), torch.from_numpy(gy_np))
                    if alias:
                        keep = g0.clone()
                        keep[:ADA_B, 1:1 + ADA_C, 3:3 + t_len] = gx
                        assert same_bits(gbuf, keep)
                    else:
                        assert same_bits(gbuf, g0) and untouched(obuf, omask)
    assert n_transfer == 8
    print(f"adain backward T={t_len}: worst ratio {worst:.2f}")


def test_adain_backward_refusals():
    gy = torch.zeros(ADA_B, ADA_C, 16, device=DEV)
    gx = torch.full_like(gy, NAN)
    stats = torch.zeros(4, ADA_MB, ADA_C, device=DEV)
    counters = torch.ones(2, device=DEV)
    for kw in (dict(gy=None), dict(gx=None), dict(stats=None), dict(counters=None)):
        a = dict(gy=gy, gx=gx, stats=stats, counters=counters)
        a.update(kw)
        refused(lambda: _adain_bwd_call(a["gy"], a["gx"], a["stats"], a["counters"], 0, 0, shape=gy.shape), ValueError,
                "null pointer")
    refused(lambda: _adain_bwd_call(gy, gx, stats, counters, 0, 0, shape=(ADA_B, ADA_C, 0)), ValueError, "empty shape")
    refused(lambda: _adain_bwd_call(gy, gx, stats, counters, 3, 0), ValueError, "mode must be")
    refused(lambda: _adain_bwd_call(gy, gx, stats, counters, 1, ADA_MB - ADA_B + 1), ValueError,
            "batch exceeds the statistics buffers")
    torch.cuda.synchronize()
    assert bool(torch.isnan(gx).all())


# ================================================================== 5. autograd on noise_synth
def _ops():
    from rave_amd import cc  # noqa: F401  (loads the ops)
    return torch.ops.rave_amd


@pytest.mark.parametrize("nb,tgt", G.PAIRS)
def test_noise_synth_is_differentiable(nb, tgt):
    """grad_fn under grad, none under no_grad; the forward's bits those of the non-grad call;
    amp.grad bit for bit the plain backward op's and within 4 e_ref; u as a constant."""
    ops = _ops()
    frames = 129
    amp_np, u_np, gy_np = _noise_inputs(nb, tgt, frames)
    amp = torch.from_numpy(amp_np).to(DEV).requires_grad_(True)
    u, gy = torch.from_numpy(u_np).to(DEV), torch.from_numpy(gy_np).to(DEV)
    y = ops.noise_synth(amp, u, N_BAND, nb)
    assert y.grad_fn is not None and y.shape == (NOISE_B, N_BAND, frames * tgt)
    y0 = ops.noise_synth(amp.detach(), u, N_BAND, nb)
    with torch.no_grad():
        y1 = ops.noise_synth(amp, u, N_BAND, nb)
    assert y0.grad_fn is None and y1.grad_fn is None and same_bits(y0, y) and same_bits(y1, y)
    y.backward(gy.transpose(1, 2).contiguous().transpose(1, 2))               # a cotangent that is not contiguous
    assert amp.grad is not None and amp.grad.shape == amp.shape
    assert same_bits(amp.grad, ops.noise_synth_backward(gy, amp.detach(), u, N_BAND, nb))
    _noise_held(f"noise_synth autograd ({nb}, {tgt})", amp.grad, amp_np, u_np, gy_np, nb, tgt)


def test_noise_synth_refuses_u_grad_and_double_backward():
    ops = _ops()
    amp_np, u_np, _ = _noise_inputs(5, 8, 4)
    amp = torch.from_numpy(amp_np).to(DEV).requires_grad_(True)
    u = torch.from_numpy(u_np).to(DEV)
    with pytest.raises(NotImplementedError, match="u is a constant"):
        ops.noise_synth(amp, u.clone().requires_grad_(True), N_BAND, 5)
    with pytest.raises(NotImplementedError, match="u is a constant"):
        ops.noise_synth(amp.detach(), u.clone().requires_grad_(True), N_BAND, 5)
    with torch.no_grad():                                                       # nothing is differentiated: no refusal
        assert ops.noise_synth(amp, u.clone().requires_grad_(True), N_BAND, 5).grad_fn is None
    with pytest.raises((NotImplementedError, RuntimeError), match="double backward"):
        torch.autograd.grad(ops.noise_synth(amp, u, N_BAND, 5).sum(), amp, create_graph=True)


# ================================================================== 6. autograd on adain
def _ada_buffers(st_np, cnt):
    """The module's buffers: four (max_batch, C, 1) statistics and two (1,) counters."""
    return [torch.from_numpy(st_np[i].copy()).to(DEV).reshape(ADA_MB, ADA_C, 1) for i in range(4)] + \
           [torch.tensor([c], device=DEV) for c in cnt]


@pytest.mark.parametrize("cnt", [(0.0, 0.0), (3.0, 2.0), (0.0, 2.0)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_adain_is_differentiable(mode, cnt):
    """Every mode has a grad_fn and none raises; y, the buffers and the counters after the call
    bit for bit what the non-grad call leaves; x.grad bit for bit the plain backward op's on the
    post-update statistics, within 4 e_ref where the call transferred and bitwise gy elsewhere."""
    ops = _ops()
    rng = np.random.default_rng(10 * mode + int(cnt[0]) + int(cnt[1]))
    st_np = _ada_stats(rng)
    x_np = (rng.standard_normal((ADA_B, ADA_C, 257)) * 1.7 + 0.3).astype(np.float32)
    gy_np = rng.standard_normal(x_np.shape).astype(np.float32)
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    gy = torch.from_numpy(gy_np).to(DEV)
    plain, grad, nograd = _ada_buffers(st_np, cnt), _ada_buffers(st_np, cnt), _ada_buffers(st_np, cnt)
    y0 = ops.adain(x.detach(), *plain, mode)
    y = ops.adain(x, *grad, mode)
    with torch.no_grad():
        y1 = ops.adain(x, *nograd, mode)
    assert y.grad_fn is not None and y0.grad_fn is None and y1.grad_fn is None
    assert same_bits(y, y0) and same_bits(y1, y0)
    for a, b, c in zip(plain, grad, nograd):
        assert same_bits(a, b) and same_bits(a, c) and not a.requires_grad and not b.requires_grad
    after = [float(plain[4]), float(plain[5])]
    assert after == [cnt[0] + (mode == 1), cnt[1] + (mode == 2)]
    y.backward(gy)
    assert x.grad is not None and x.grad.shape == x.shape
    stats_after = torch.stack([b.reshape(ADA_MB, ADA_C) for b in plain[:4]])
    assert same_bits(x.grad, ops.adain_backward(gy, stats_after, torch.cat(plain[4:]), mode))
    transfer = G.adain_transfers(after, mode)
    assert transfer == {0: cnt == (3.0, 2.0), 1: cnt[1] != 0, 2: False}[mode]   # mode 1 counts its own update
    if transfer:
        want = G.adain_backward(gy_np, stats_after.cpu().numpy(), after, mode, 0)
        e_ref = maxerr(G.adain_backward(gy_np, stats_after.cpu().numpy(), after, mode, 0, np.float32), want)
        err = maxerr(x.grad, want)
        report(f"adain autograd mode {mode} counters {cnt}", err, e_ref)
        assert err <= 4 * e_ref
    else:
        assert same_bits(x.grad, gy)
    with pytest.raises((NotImplementedError, RuntimeError), match="double backward"):
        torch.autograd.grad(ops.adain(x, *_ada_buffers(st_np, cnt), mode).sum(), x, create_graph=True)


# ================================================================== 7. the module tree
def _small_generator():
    from rave_amd import cc, config as rcfg, modules as M
    cc.use_transposed_grad(True)
    try:
        gen = M.GeneratorV2(data_size=16, capacity=16, ratios=(2, 4), latent_size=16, kernel_size=3, dilations=[1, 3],
                            activation="snake", adain=True, noise=rcfg.NoiseConfig(hidden_size=16)).to(DEV)
    finally:
        cc.use_transposed_grad(False)
    with torch.no_grad():
        for m in gen.modules():
            if isinstance(m, M.Snake):
                m.alpha.uniform_(0.5, 2.0)
        # band amplitudes round sigmoid's middle (amp - 5 round 0): at the default initialisation they
        # sit at sigmoid(-5)^2.3 and the noise branch's gradients would vanish beside the waveform's
        gen.noise_module.net[4].bias.fill_(5.0)
    return gen


def _plain_torch_generator(gen, zr, u, leaves, detach_noise=False):
    """GeneratorV2.forward of ``gen`` in plain torch over the cloned leaves: Snake and the convs
    as tests/test_gpu_convt_grad.py writes them, AdaIN as the identity in train() and as the
    transfer with the module's buffers as constants in eval(), the noise filter stage as
    tests/noise_grad_ref.noise_synth_torch."""
    import torch.nn.functional as F
    from rave_amd import cc, modules as M
    L = lambda p: None if p is None else leaves[id(p)]

    def act_of(m, h):
        al = L(m.alpha)
        return h + (al + 1e-9).reciprocal() * (al * h).sin().pow(2)            # modules.Snake.forward

    def conv(m, h):
        return F.conv1d(F.pad(h, (m.pad_l, m.pad_r)), L(m.weight), L(m.bias), stride=m.stride, dilation=m.dilation)

    h, seen = zr, 0
    for m in gen.net:
        if isinstance(m, M.Snake):
            h = act_of(m, h)
        elif isinstance(m, cc.ConvTranspose1d):
            assert m.differentiable
            h = F.conv_transpose1d(h, L(m.weight), L(m.bias), stride=m.stride, padding=m.stride // 2)
        elif isinstance(m, M.AdaptiveInstanceNormalization):
            seen += 1
            if not gen.training:
                assert float(m.num_update_x) == 1 and float(m.num_update_y) == 1 and not bool(m.learn_x)
                B = h.shape[0]
                h = (h - m.mean_x[:B]) / (m.std_x[:B] + 1e-5) * m.std_y[:B] + m.mean_y[:B]
        elif isinstance(m, M.Residual):
            net = m.aligned.branches[0].net
            h = h + conv(net[3], act_of(net[2], conv(net[1], act_of(net[0], h))))
        else:
            assert isinstance(m, cc.Conv1d)
            h = conv(m, h)
    assert seen == 4 and isinstance(gen.net[len(gen.net) - 1], M.Snake)        # h: the trailing activation applied
    wave = conv(gen.waveform_module, h)
    a = h
    for m in gen.noise_module.net:
        a = act_of(m, a) if isinstance(m, M.Snake) else conv(m, a)
    noise = G.noise_synth_torch(a, u, 16, gen.noise_module.noise_bands, gen.noise_module.target)
    if detach_noise:
        noise = noise.detach()
    return torch.tanh(wave[:, :16] * torch.sigmoid(wave[:, 16:]) + noise)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_loss_fills_every_parameter_of_a_v3_noise_decoder(mode):
    """A small GeneratorV2 with Snake, AdaIN and the noise module: in train() (AdaIN the identity)
    and in eval() after one learn_x and one learn_y pass (AdaIN transferring), with a fixed draw,
    z and every parameter -- noise_module's convs and Snakes among them -- get a gradient within
    1e-3 of its max of fp32 torch autograd of the same tree.  The trailing Snake's alpha feeds both
    the waveform conv and the noise module's first conv: its gradient is the sum of the two, which
    differs from the waveform branch's half alone."""
    from rave_amd import modules as M
    torch.manual_seed(5)
    gen = _small_generator()
    B, Fz = 2, 33
    u = torch.rand(B, Fz, 16, 8, device=DEV)
    adains = [m for m in gen.modules() if isinstance(m, M.AdaptiveInstanceNormalization)]
    assert len(adains) == 4
    if mode == "eval":
        gen.eval()
        with torch.no_grad():
            for flag in ("learn_x", "learn_y"):
                for m in adains:
                    getattr(m, flag).fill_(1.0)
                gen(torch.randn(B, 16, Fz, device=DEV) * (1.0 if flag == "learn_x" else 1.5), u)
                for m in adains:
                    getattr(m, flag).fill_(0.0)
    else:
        gen.train()
    z = torch.randn(B, 16, Fz, device=DEV, requires_grad=True)
    y = gen(z, u)
    assert y.grad_fn is not None and y.shape == (B, 16, Fz * 8)
    gy = torch.randn_like(y)
    y.backward(gy)

    leaves = {id(p): p.detach().clone().requires_grad_(True) for p in gen.parameters()}
    zr = z.detach().clone().requires_grad_(True)
    ref = _plain_torch_generator(gen, zr, u, leaves)
    assert float((ref - y).detach().abs().max()) < 1e-4
    ref.backward(gy)
    params = dict(gen.named_parameters())
    assert len(params) == len(leaves)
    noise_names = [n for n in params if n.startswith("noise_module.")]
    assert len(noise_names) == 8 and sum("alpha" in n for n in noise_names) == 2   # 3 convs (w, b), 2 Snakes
    for name, p in [("z", z)] + list(params.items()):
        want = zr.grad if name == "z" else leaves[id(p)].grad
        assert p.grad is not None and p.grad.shape == want.shape, name
        err, top = float((p.grad - want).abs().max()), float(want.abs().max())
        print(f"GeneratorV2 v3_noise {mode} {name}: max {top:.3e} err {err:.3e}")
        assert top > 0 and err <= 1e-3 * top, (name, err, top)
    # the shared trailing activation: the sum of both branches, not the waveform conv's half
    tail = gen.net[len(gen.net) - 1].alpha
    half = {id(p): p.detach().clone().requires_grad_(True) for p in gen.parameters()}
    _plain_torch_generator(gen, z.detach(), u, half, detach_noise=True).backward(gy)
    full, wave_only = leaves[id(tail)].grad, half[id(tail)].grad
    gap = float((full - wave_only).abs().max())
    print(f"trailing alpha {mode}: sum max {float(full.abs().max()):.3e}, noise branch's share {gap:.3e}")
    assert gap > 10 * 1e-3 * float(full.abs().max())                          # a missing half would miss the bound
    assert float((tail.grad - full).abs().max()) <= 1e-3 * float(full.abs().max())


# ================================================================== 8. end to end
def test_spectral_loss_fills_every_parameter_of_v3_noise():
    """RAVEModules(v3_noise(capacity=8)) in train(): the spectral loss of forward(x, noise_u)
    against x fills every encoder and decoder parameter with finite values.  B = 2, two hops
    (2048 samples): the 16 kHz resolutions (n_fft 512 / 1024 / 256), since reflect padding at
    44.1 kHz's n_fft 4096 needs more than 2048 samples."""
    from rave_amd import cc, config as rcfg, modules as M
    from rave_amd.distance import MultiResolutionSTFTLoss
    torch.manual_seed(6)
    cfg = rcfg.v3_noise(capacity=8)
    cc.use_transposed_grad(True)
    try:
        model = M.RAVEModules(cfg).to(DEV).train()
    finally:
        cc.use_transposed_grad(False)
    B, T = 2, 2 * cfg.hop
    assert T == 2048
    x = 0.3 * torch.randn(B, 1, T, device=DEV)
    frames = T // cfg.n_band // 8                                               # the noise module's three stride-2 convs
    u = torch.rand(B, frames, cfg.n_band, 8, device=DEV)
    y = model(x, u)
    assert y.shape == x.shape and y.grad_fn is not None
    loss = sum(MultiResolutionSTFTLoss.for_sample_rate(16000)(y[:, 0], x[:, 0]))
    loss.backward()
    names = [n for n, _ in model.named_parameters()]
    assert any(n.startswith("decoder.noise_module.") for n in names) and any(n.startswith("encoder.") for n in names)
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        assert bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
