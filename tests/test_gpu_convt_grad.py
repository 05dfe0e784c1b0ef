"""The conv_transpose1d backward kernels (rave_conv_transpose1d_backward_data / _weight,
conv_grad.hip) and cc.ConvTranspose1d's opt-in autograd over them, against
tests/convt_grad_ref.py.

Bar: per output (gx, gweight, gbias, galpha), kernel max-abs error <= 4 e_ref,
e_ref the reference's own float32 run against its float64 run.  Every call
goes through NaN-guarded strided views of x, gy and gx, NaN-filled tails on
gweight / gbias / galpha and a never-zeroed NaN workspace.

Measured on the MI355X, worst kernel / e_ref over this file's cases: gx 1.80,
gweight 1.79, gbias 1.08, galpha 1.40.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import conv_grad_harness as H, convt_grad_ref as G
from tests.conv_grad_harness import native as _N
from tests.test_gpu_aux_kernels import DEV, same_bits
from tests.test_gpu_conv_grad import E2E_CASES, _e2e_inputs as _conv_inputs

pytestmark = pytest.mark.gpu
T_INS = [1, 2, 31, 32, 33, 63, 64, 65, 129, 257]
# channel pairs from {16, 40, 64, 136}, on and off the kernels' 16 / 32 / 64 tiles; the two
# last (small) ones go with the long t_in so that the reference's Python loops stay short
PAIRS = [(16, 16), (40, 16), (16, 40), (64, 40), (40, 64), (136, 16), (16, 136), (64, 64), (40, 40), (16, 64)]
ACTS = [G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE]


def _case(r, act, B, c_in, c_out, t_in, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c_in, t_in)).astype(np.float32)
    x[0, 0, : min(3, t_in)] = 0.0                           # exact zeros beside the negatives
    w = (rng.standard_normal((c_in, c_out, 2 * r)) / np.sqrt(c_in * 2)).astype(np.float32)
    gy = rng.standard_normal((B, c_out, t_in * r)).astype(np.float32)
    alpha = rng.uniform(0.1, 3.0, c_in).astype(np.float32)
    alpha[-1] = 0.0
    return dict(x=x, w=w, gy=gy, alpha=alpha, r=r, act=act, slope=0.2, t_in=t_in, t_out=t_in * r, B=B, c_in=c_in,
                c_out=c_out)


def _args(c, **kw):
    N = _N()
    a = N.ConvBackwardArgs()
    a.c_in, a.c_out, a.kernel, a.stride, a.dilation = c["c_in"], c["c_out"], 2 * c["r"], c["r"], 1
    a.transposed, a.out_shift, a.act, a.leaky_slope = 1, c["r"] // 2, c["act"], c["slope"]
    a.batch, a.t_in, a.t_out, a.precision = c["B"], c["t_in"], c["t_out"], N.PREC_F32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd(c, **kw):
    """One data + one weight call on guarded views; returns (dict of outputs, workspace floats)."""
    return H.bwd("rave_conv_transpose1d_backward", (c["c_in"], c["c_out"], 2 * c["r"]), _args, c, **kw)


def _ref(c):
    return G.with_e_ref(c["gy"], c["x"], c["w"], c["alpha"], c["r"], c["act"], c["slope"])


def _held(what, out, c):
    """Print every figure, then assert 4 e_ref per output; returns the worst ratio."""
    return H.held(what, out, _ref(c))


# ================================================================== 1. the edge sweep
def _sweep():
    for f, r in enumerate(G.STRIDES):
        for i, t_in in enumerate(T_INS):
            c_in, c_out = PAIRS[(i + 3 * f) % 8] if i < 8 else PAIRS[8 + (i + f) % 2]
            yield pytest.param(r, ACTS[(i + f) % 3], 1 + 2 * ((i + f) % 2), c_in, c_out, t_in, id=f"r{r}-t{t_in}")


@pytest.mark.parametrize("r,act,B,c_in,c_out,t_in", list(_sweep()))
def test_backward_vs_float64(r, act, B, c_in, c_out, t_in):
    c = _case(r, act, B, c_in, c_out, t_in, seed=t_in)
    out, _ = _bwd(c)
    _held(f"r {r} act {act} B {B} {c_in}->{c_out} t_in {t_in}", out, c)


@pytest.mark.parametrize("r", G.STRIDES)
def test_every_activation(r):
    """The activations the rotation of the sweep leaves out at one stride, at one odd shape."""
    for act in ACTS:
        c = _case(r, act, 2, 40, 16, 33, seed=5)
        _held(f"r {r} act {act}", _bwd(c)[0], c)


# ================================================================== 2. split and unsplit
@pytest.mark.parametrize("r", G.STRIDES)
def test_split_and_unsplit_paths(r):
    split = _case(r, G.ACT_LEAKY, 3, 16, 16, 700, seed=11)       # 33 chunks of 64 input columns, one tile
    out, nws = _bwd(split)
    assert nws > 0
    _held(f"r {r} split-K", out, split)
    again, _ = _bwd(split)
    assert all(same_bits(out[k], again[k]) for k in out)
    one = _case(r, G.ACT_LEAKY, 1, 16, 16, 129, seed=12)         # 3 chunks: below four per split
    out, nws = _bwd(one)
    assert nws == 0
    _held(f"r {r} unsplit", out, one)
    snake = _case(r, G.ACT_SNAKE, 1, 16, 16, 129, seed=13)       # alpha partials only
    assert _bwd(snake)[1] > 0 and _bwd(snake, want=("gx", "gw", "gb"))[1] == 0


# ================================================================== 3. unit cotangents
@pytest.mark.parametrize("r", G.STRIDES)
def test_unit_cotangents(r):
    k, P, t_in = 2 * r, r // 2, 65
    c = _case(r, G.ACT_LEAKY, 2, 40, 16, t_in, seed=21)
    c["w"] = (1.0 + np.arange(40 * 16 * k, dtype=np.float32).reshape(40, 16, k))      # every tap distinct
    b0, m0 = 1, 5
    a_ref = np.where(c["x"] > 0, c["x"], c["x"] * np.float32(0.2)).astype(np.float32)
    for t0 in (0, r - 1, (t_in * r) // 2, t_in * r - 1):
        c["gy"] = np.zeros((2, 16, t_in * r), np.float32)
        c["gy"][b0, m0, t0] = 1.0
        hot = dict(c, act=G.ACT_NONE)
        ga = _bwd(hot, want=("gx",))[0]["gx"].cpu().numpy()
        gw = _bwd(c, want=("gw",))[0]["gw"].cpu().numpy()
        want_ga = np.zeros_like(ga)
        want_gw = np.zeros_like(gw)
        hits = 0
        for j in range(k):                                  # u r + j - P = t0; the taps off either end are absent
            if (t0 + P - j) % r == 0 and 0 <= (t0 + P - j) // r < t_in:
                u = (t0 + P - j) // r
                want_ga[b0, :, u] = c["w"][:, m0, j]
                want_gw[:, m0, j] = a_ref[b0, :, u]
                hits += 1
        assert hits == (1 if t0 in (0, t_in * r - 1) else 2)
        assert np.array_equal(ga.view(np.uint32), want_ga.view(np.uint32))
        assert np.array_equal(gw.view(np.uint32), want_gw.view(np.uint32))


# ================================================================== 4. NULL outputs, zeros, reruns, refusals
@pytest.mark.parametrize("r", G.STRIDES)
def test_null_outputs_zero_cotangent_and_reruns(r):
    c = _case(r, G.ACT_SNAKE, 3, 40, 64, 257, seed=31)
    full, nws = _bwd(c)
    assert nws > 0
    again, _ = _bwd(c)
    assert all(same_bits(full[k], again[k]) for k in full)
    for drop in ("gx", "gw", "gb", "ga"):
        rest = tuple(k for k in ("gx", "gw", "gb", "ga") if k != drop)
        part, _ = _bwd(c, want=rest)
        assert set(part) == set(rest) and all(same_bits(part[k], full[k]) for k in rest), drop
    bias_only, _ = _bwd(c, want=("gb",), null_x=True)
    assert same_bits(bias_only["gb"], full["gb"])
    z = dict(c, gy=np.zeros_like(c["gy"]))
    out, _ = _bwd(z)
    assert all(bool((v == 0).all()) for v in out.values())


def test_refusals_and_the_missing_x():
    N = _N()
    c = _case(2, G.ACT_NONE, 1, 16, 16, 32)
    out, _ = _bwd(c, want=("gx", "gb"), null_x=True)                       # neither needs x
    full, _ = _bwd(c)
    assert same_bits(out["gx"], full["gx"]) and same_bits(out["gb"], full["gb"])

    def refused(status, word, cc_=c, **kw):
        assert _bwd(cc_, check=False, **kw)[0] == status
        assert word in N.lib.rave_last_error().decode(), (word, N.lib.rave_last_error().decode())

    refused(N.RAVE_ERR_ARG, "needs the input x", want=("gw",), null_x=True)
    refused(N.RAVE_ERR_ARG, "needs the input x", cc_=dict(c, act=G.ACT_LEAKY), want=("gx",), null_x=True)
    refused(N.RAVE_ERR_ARG, "transposed", transposed=0)
    refused(N.RAVE_ERR_ARG, "kernel", kernel=3)
    refused(N.RAVE_ERR_ARG, "pad_left", pad_left=1, out_shift=0, t_in=33)
    refused(N.RAVE_ERR_ARG, "out_shift", out_shift=0)
    refused(N.RAVE_ERR_ARG, "precision", precision=N.PREC_SPLIT16)
    refused(N.RAVE_ERR_UNSUPPORTED, "stride", kernel=16, stride=8, out_shift=4, t_out=256)
    # the non-transposed entry points keep refusing these arguments
    assert N.lib.rave_conv1d_backward_workspace(C.byref(_args(c))) == N.RAVE_ERR_ARG
    assert "transposed" in N.lib.rave_last_error().decode()


# ================================================================== 5. the public surface
def _convt(*a, grad=True, cached=False, precision="f32", **kw):
    from rave_amd import cc
    cc.use_cached_conv(cached)
    cc.set_precision(precision)
    cc.use_transposed_grad(grad)
    try:
        return cc.ConvTranspose1d(*a, **kw).to(DEV)
    finally:
        cc.use_cached_conv(False)
        cc.set_precision("f32")
        cc.use_transposed_grad(False)


def test_new_symbols_and_ops_exist():
    N = _N()
    for name in ("rave_conv_transpose1d_backward_data", "rave_conv_transpose1d_backward_weight",
                 "rave_conv_transpose1d_backward_workspace"):
        assert hasattr(N.lib, name)
    from rave_amd import cc  # noqa: F401
    assert torch.ops.rave_amd.conv_transpose1d_w and torch.ops.rave_amd.conv_transpose1d_backward


def test_conv_transpose1d_is_differentiable():
    """weight.grad, bias.grad and x.grad bit for bit the C boundary's and within 4 e_ref; the output
    under grad bit for bit the no-grad output and a default-constructed module's."""
    torch.manual_seed(0)
    up = _convt(16, 8, 8, stride=4, padding=2, bias=True)
    assert up.differentiable
    x = torch.randn(2, 16, 100, device=DEV, requires_grad=True)
    y = up(x)
    assert y.grad_fn is not None and y.shape == (2, 8, 400)
    with torch.no_grad():
        y0 = up(x)
    assert y0.grad_fn is None and same_bits(y0, y)
    plain = _convt(16, 8, 8, stride=4, padding=2, bias=True, grad=False)
    assert not plain.differentiable
    with torch.no_grad():
        plain.weight.copy_(up.weight)
        plain.bias.copy_(up.bias)
    y1 = plain(x)
    assert y1.grad_fn is None and same_bits(y1, y)
    gy = torch.randn_like(y)
    y.backward(gy)
    c = dict(x=x.detach().cpu().numpy(), w=up.weight.detach().cpu().numpy(), gy=gy.cpu().numpy(),
             alpha=np.zeros(16, np.float32), r=4, act=G.ACT_NONE, slope=0.2, t_in=100, t_out=400, B=2, c_in=16, c_out=8)
    want, _ = _bwd(c)
    assert same_bits(x.grad, want["gx"]) and same_bits(up.weight.grad, want["gw"]) and same_bits(up.bias.grad, want["gb"])
    _held("cc.ConvTranspose1d(16, 8, 8, stride=4)", dict(gx=x.grad, gw=up.weight.grad, gb=up.bias.grad), c)


def test_weight_norm_gets_its_gradients():
    """weight_g.grad, weight_v.grad and bias.grad against fp32 torch autograd of the same
    composition on the same GPU (1e-3 of each gradient's max: the plumbing through the
    weight_norm edge; the kernels' bound is held above)."""
    import torch.nn.functional as F
    torch.manual_seed(2)
    up = torch.nn.utils.weight_norm(_convt(16, 8, 4, stride=2, padding=1, bias=True, activation=1))
    with torch.no_grad():
        up.weight_g.mul_(torch.rand_like(up.weight_g) + 0.5)              # g off its initial |v|
    x = torch.randn(2, 16, 64, device=DEV)
    y = up(x)
    assert y.grad_fn is not None
    gy = torch.randn_like(y)
    y.backward(gy)
    g, v, b = (t.detach().clone().requires_grad_(True) for t in (up.weight_g, up.weight_v, up.bias))
    w = torch._weight_norm(v, g, 0)
    ref = F.conv_transpose1d(F.leaky_relu(x, 0.2), w, b, stride=2, padding=1)
    assert float((ref - y).detach().abs().max()) < 1e-4
    ref.backward(gy)
    for got, want in ((up.weight_g, g), (up.weight_v, v), (up.bias, b)):
        assert got.grad is not None and got.grad.shape == want.grad.shape
        assert float((got.grad - want.grad).abs().max()) <= 1e-3 * float(want.grad.abs().max())


def test_frozen_weight_and_input_only_paths():
    """Only x asks for a gradient (frozen layer), and only the parameters do: the same bits as the full call."""
    up = _convt(16, 32, 4, stride=2, padding=1, bias=True)
    x = torch.randn(2, 16, 100, device=DEV)
    gy = torch.randn(2, 32, 200, device=DEV)
    xa = x.clone().requires_grad_(True)
    up(xa).backward(gy)
    full = (xa.grad.clone(), up.weight.grad.clone(), up.bias.grad.clone())
    up.zero_grad(set_to_none=True)
    up(x).backward(gy)                                     # x without grad: the weight is not saved
    assert same_bits(up.weight.grad, full[1]) and same_bits(up.bias.grad, full[2])
    for p in up.parameters():
        p.requires_grad_(False)
    xb = x.clone().requires_grad_(True)
    up(xb).backward(gy)                                    # frozen, no activation: x is not saved
    assert same_bits(xb.grad, full[0])


def test_other_modes_carry_no_grad_fn():
    x = torch.randn(1, 16, 64, device=DEV, requires_grad=True)
    assert _convt(16, 16, 4, stride=2, padding=1, grad=False)(x).grad_fn is None
    assert _convt(16, 16, 4, stride=2, padding=1, cached=True)(x).grad_fn is None
    assert _convt(16, 16, 4, stride=2, padding=1, precision="split16")(x).grad_fn is None


def test_double_backward_raises():
    up = _convt(16, 16, 4, stride=2, padding=1)
    x = torch.randn(1, 16, 64, device=DEV, requires_grad=True)
    with pytest.raises((NotImplementedError, RuntimeError), match="double backward"):
        torch.autograd.grad(up(x).sum(), x, create_graph=True)


# ================================================================== 6. the module tree
@pytest.mark.parametrize("activation", ["leaky", "snake"])
def test_loss_fills_every_parameter_of_a_v2_decoder(activation):
    """Every parameter of a small GeneratorV2 built under the switch gets a gradient, within 1e-3 of
    its max of fp32 torch autograd of the same tree in plain torch on the same GPU (a plumbing
    check, the kernels' bounds are held above and in tests/test_gpu_conv_grad.py)."""
    import torch.nn.functional as F
    from rave_amd import cc, modules as M
    torch.manual_seed(3)
    cc.use_transposed_grad(True)
    try:
        gen = M.GeneratorV2(data_size=16, capacity=16, ratios=(2, 4), latent_size=16, kernel_size=3, dilations=[1, 3],
                            activation=activation, adain=False, noise=None).to(DEV)
    finally:
        cc.use_transposed_grad(False)
    with torch.no_grad():
        for m in gen.modules():
            if isinstance(m, M.Snake):
                m.alpha.uniform_(0.5, 2.0)
    z = torch.randn(2, 16, 33, device=DEV, requires_grad=True)
    y = gen(z)
    assert y.grad_fn is not None and y.shape == (2, 16, 33 * 8)
    gy = torch.randn_like(y)
    y.backward(gy)

    leaves = {id(p): p.detach().clone().requires_grad_(True) for p in gen.parameters()}
    L = lambda p: None if p is None else leaves[id(p)]
    zr = z.detach().clone().requires_grad_(True)

    def act_of(m, h):
        if isinstance(m, M.Snake):
            al = L(m.alpha)
            return h + (al + 1e-9).reciprocal() * (al * h).sin().pow(2)        # modules.Snake.forward
        return F.leaky_relu(h, m.negative_slope)

    def conv(m, h):
        return F.conv1d(F.pad(h, (m.pad_l, m.pad_r)), L(m.weight), L(m.bias), stride=m.stride, dilation=m.dilation)

    h, ups = zr, 0
    for m in gen.net:
        if isinstance(m, (M.Snake, M.LeakyReLU)):
            h = act_of(m, h)
        elif isinstance(m, cc.ConvTranspose1d):
            assert m.differentiable
            h = F.conv_transpose1d(h, L(m.weight), L(m.bias), stride=m.stride, padding=m.stride // 2)
            ups += 1
        elif isinstance(m, M.Residual):
            net = m.aligned.branches[0].net
            h = h + conv(net[3], act_of(net[2], conv(net[1], act_of(net[0], h))))
        else:
            assert isinstance(m, cc.Conv1d)
            h = conv(m, h)
    assert ups == 2
    ref = torch.tanh(h[:, :16] * torch.sigmoid(h[:, 16:]))
    assert float((ref - y).detach().abs().max()) < 1e-4
    ref.backward(gy)
    params = dict(gen.named_parameters())
    assert len(params) == len(leaves) and any("alpha" in n for n in params) == (activation == "snake")
    for name, p in [("z", z)] + list(params.items()):
        want = zr.grad if name == "z" else leaves[id(p)].grad
        assert p.grad is not None and p.grad.shape == want.shape, name
        err, top = float((p.grad - want).abs().max()), float(want.abs().max())
        print(f"GeneratorV2 {activation} {name}: max {top:.3e} err {err:.3e}")
        assert err <= 1e-3 * top, (name, err, top)


# ================================================================== 7. end to end
# ConvTranspose1d(32, 64, 4, stride 2, LeakyReLU in front) on a (2, 32, 128) input -> Conv1d(64, rows, 7)
# -> CachedPQMF.inverse(., mode, noise) -> sum(MultiResolutionSTFTLoss): tests/test_gpu_conv_grad.py's
# chain with the upsampler in front.

@functools.lru_cache(maxsize=None)
def _e2e_inputs(rows, mode):
    """The upsampler's x, weight, bias and `delta`, and the conv test's own inputs.  The upsampler's
    output is pinned to that test's x: delta = x - up(xu) in float64, added to the upsampler's output
    (a plain add, which hands the cotangent through: the forward kernel takes no residual on a
    transposed conv), so the multiband tensor stays pinned through the conv's fused residual."""
    x, w, bias, res, noise, target = _conv_inputs(rows, mode)
    rng = np.random.default_rng(2007)
    xu = rng.standard_normal((2, 32, 128)).astype(np.float32)
    wu = (rng.standard_normal((32, 64, 4)) / np.sqrt(32 * 2)).astype(np.float32)
    bu = (0.1 * rng.standard_normal(64)).astype(np.float32)
    y0 = G.forward(xu, wu, bu, None, None, 2, G.ACT_LEAKY, 0.2)
    return xu, wu, bu, (x.astype(np.float64) - y0).astype(np.float32), (x, w, bias, res, noise, target)


@functools.lru_cache(maxsize=None)
def _e2e_ref(rows, mode):
    """CPU autograd of the oracle composition: the float64 gradients of the upsampler's weight and
    input, the fp32 ones, and the share of clamped bins."""
    import torch.nn.functional as F
    from tests import stft_loss_ref as S
    from tests.test_gpu_pqmf_grad import _filters
    from tests.test_pqmf_grad_ref_host import _head, _oracle_inverse
    _, hki = _filters()
    xu, wu, bu, delta, (x, w, bias, res, noise, target) = _e2e_inputs(rows, mode)
    resolutions = S.fork_resolutions(44100)
    out = {}
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(a).to(dtype)
        xt, wt = t(xu).requires_grad_(True), t(wu).requires_grad_(True)
        up = F.conv_transpose1d(F.leaky_relu(xt, 0.2), wt, t(bu), stride=2, padding=1) + t(delta)
        y = F.conv1d(F.pad(up, (3, 3)), t(w), t(bias)) + t(res)
        audio = _oracle_inverse(_head(y, mode, t(noise)), t(hki), False)
        sc, mag = S.mr_loss(audio, t(target), resolutions)
        out[dtype] = torch.autograd.grad(sc + mag, (wt, xt))
        if dtype == torch.float64:
            out["share"] = S.clamped_share(audio.detach(), resolutions)
    return out


@pytest.mark.parametrize("rows,mode", E2E_CASES)
def test_loss_gradient_reaches_the_upsampler(rows, mode):
    """weight.grad and x.grad of the upsampler within 4 e_ref of the float64 CPU gradient, in max-abs
    and in relative L2; e_ref the CPU fp32 autograd gradient's error against it.  The cotangent
    arrives from the conv's data gradient (section 19), the PQMF adjoint (18) and the loss (17).
    Measured on the MI355X, kernel / e_ref in max-abs and L2: weight.grad 0.17 and 0.16, x.grad
    0.12 and 0.14 (16 rows, mode 2); 0.31 and 0.31, 0.30 and 0.29 (32 rows, mode 1)."""
    from rave_amd import cc
    from rave_amd.distance import MultiResolutionSTFTLoss
    from tests.test_gpu_conv_grad import _conv
    from tests.test_gpu_pqmf_grad import _pqmf
    ref = _e2e_ref(rows, mode)
    assert ref["share"] < 1e-4, ref["share"]
    xu, wu, bu, delta, (x, w, bias, res, noise, target) = _e2e_inputs(rows, mode)
    up = _convt(32, 64, 4, stride=2, padding=1, bias=True, activation=cc.ACT_LEAKY)
    conv = _conv(64, rows, 7, padding=cc.get_padding(7))
    with torch.no_grad():
        up.weight.copy_(torch.from_numpy(wu))
        up.bias.copy_(torch.from_numpy(bu))
        conv.weight.copy_(torch.from_numpy(w))
        conv.bias.copy_(torch.from_numpy(bias))
    xt = torch.from_numpy(xu).to(DEV).requires_grad_(True)
    h = up(xt) + torch.from_numpy(delta).to(DEV)
    assert float((h.detach().cpu() - torch.from_numpy(x)).abs().max()) < 1e-5
    y = conv(h, torch.from_numpy(res).to(DEV))
    audio = _pqmf().inverse(y, mode, torch.from_numpy(noise).to(DEV))[:, 0]
    assert audio.shape == (2, 4096)
    loss = sum(MultiResolutionSTFTLoss.for_sample_rate(44100)(audio, torch.from_numpy(target).to(DEV)))
    loss.backward()
    fails = []
    for name, got, g64, g32 in zip(("weight", "x"), (up.weight.grad, xt.grad), ref[torch.float64], ref[torch.float32]):
        def errs(g):
            d = g.double().cpu() - g64
            return float(d.abs().max()), float(d.norm() / g64.norm())
        (e_abs, e_l2), (k_abs, k_l2) = errs(g32), errs(got)
        print(f"end to end rows {rows} mode {mode} upsampler {name}.grad: clamped share {ref['share']:.2e}; e_ref max-abs "
              f"{e_abs:.3e} L2 {e_l2:.3e}; kernel {k_abs:.3e} {k_l2:.3e}; ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
        assert bool(torch.isfinite(got).all())
        if not (k_abs <= 4 * e_abs and k_l2 <= 4 * e_l2):
            fails.append((name, k_abs, e_abs, k_l2, e_l2))
    assert not fails, fails
