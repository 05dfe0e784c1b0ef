"""The conv1d backward kernels (rave_conv1d_backward_data / _weight, conv_grad.hip)
and cc.Conv1d's autograd over them, against tests/conv_grad_ref.py.

Bar: per output (gx, gweight, gbias, galpha), kernel max-abs error <= 4 e_ref,
e_ref the reference's own float32 run against its float64 run.  Every call
goes through NaN-guarded strided views of x, gy and gx.

Measured on the MI355X, worst kernel / e_ref over the edge sweep: gx 1.64,
gweight 1.57, gbias 1.48, galpha 2.94.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import conv_grad_harness as H, conv_grad_ref as G
from tests.conv_grad_harness import native as _N
from tests.test_gpu_aux_kernels import DEV, same_bits

pytestmark = pytest.mark.gpu
T_OUTS = [1, 2, 31, 32, 33, 63, 64, 65, 129, 257]
# channel pairs from {16, 40, 64, 136}, on and off the kernels' 16 / 32 / 64 tiles; the two
# last (small) ones go with the long t_out so that the reference's Python loops stay short
PAIRS = [(16, 16), (40, 16), (16, 40), (64, 40), (40, 64), (136, 16), (16, 136), (64, 64), (40, 40), (16, 64)]
ACTS = [G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE]


def _geometry(fam, pad, t_out):
    k, s, d = fam
    span = (k - 1) * d + 1
    pl, pr = {"centred": ((span - 1) // 2, span // 2), "causal": (span - 1, 0), "none": (0, 0), "tail": (0, 0)}[pad]
    t_in = (t_out - 1) * s + span - pl - pr + (s - 1 if pad == "tail" else 0)
    return pl, pr, t_in


def _case(fam, pad, act, B, c_in, c_out, t_out, seed=0):
    k, s, d = fam
    pl, pr, t_in = _geometry(fam, pad, t_out)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c_in, t_in)).astype(np.float32)
    x[0, 0, : min(3, t_in)] = 0.0                           # exact zeros beside the negatives
    w = (rng.standard_normal((c_out, c_in, k)) / np.sqrt(c_in * k)).astype(np.float32)
    gy = rng.standard_normal((B, c_out, t_out)).astype(np.float32)
    alpha = rng.uniform(0.1, 3.0, c_in).astype(np.float32)
    alpha[-1] = 0.0
    return dict(x=x, w=w, gy=gy, alpha=alpha, k=k, s=s, d=d, pl=pl, pr=pr, act=act, slope=0.2, t_in=t_in, t_out=t_out,
                B=B, c_in=c_in, c_out=c_out)


def _args(c, **kw):
    N = _N()
    a = N.ConvBackwardArgs()
    a.c_in, a.c_out, a.kernel, a.stride, a.dilation = c["c_in"], c["c_out"], c["k"], c["s"], c["d"]
    a.pad_left, a.pad_right, a.act, a.leaky_slope = c["pl"], c["pr"], c["act"], c["slope"]
    a.batch, a.t_in, a.t_out, a.precision = c["B"], c["t_in"], c["t_out"], N.PREC_F32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd(c, **kw):
    """One data + one weight call on guarded views; returns (dict of outputs, workspace floats)."""
    return H.bwd("rave_conv1d_backward", (c["c_out"], c["c_in"], c["k"]), _args, c, **kw)


def _ref(c):
    return G.with_e_ref(c["gy"], c["x"], c["w"], c["alpha"], c["k"], c["s"], c["d"], c["pl"], c["pr"], c["act"], c["slope"])


def _held(what, out, c):
    """Print every figure, then assert 4 e_ref per output; returns the worst ratio."""
    return H.held(what, out, _ref(c))


# ================================================================== 1. the edge sweep
def _sweep():
    for f, fam in enumerate(G.FAMILIES):
        pads = ["centred", "causal", "none"] + (["tail"] if fam[1] > 1 else [])
        for i, t_out in enumerate(T_OUTS):
            c_in, c_out = PAIRS[(i + f) % 8] if i < 8 else PAIRS[8 + (i + f) % 2]
            yield pytest.param(fam, pads[(i + 2 * f) % len(pads)], ACTS[(i + f) % 3], 1 + 2 * ((i + f // 3) % 2), c_in,
                               c_out, t_out, id=f"k{fam[0]}s{fam[1]}d{fam[2]}-t{t_out}")


@pytest.mark.parametrize("fam,pad,act,B,c_in,c_out,t_out", list(_sweep()))
def test_backward_vs_float64(fam, pad, act, B, c_in, c_out, t_out):
    c = _case(fam, pad, act, B, c_in, c_out, t_out, seed=t_out)
    out, _ = _bwd(c)
    _held(f"{fam} {pad} act {act} B {B} {c_in}->{c_out} t_out {t_out}", out, c)
    if pad == "tail":
        assert bool((out["gx"][:, :, c["t_in"] - (fam[1] - 1):] == 0).all())


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_every_padding_and_activation(fam):
    """The paddings and activations the rotation of the sweep leaves out at one family, at one odd shape."""
    for pad in ["centred", "causal", "none"] + (["tail"] if fam[1] > 1 else []):
        for act in ACTS:
            c = _case(fam, pad, act, 2, 40, 16, 33, seed=5)
            _held(f"{fam} {pad} act {act}", _bwd(c)[0], c)


def test_forward_and_backward_refuse_the_same_shapes():
    N = _N()
    for k, s, d in G.FAMILIES + [(5, 1, 1), (3, 2, 1), (7, 1, 2), (3, 1, 17), (4, 4, 1)]:
        for c_in in (16, 40, 64, 136):
            for c_out in (16, 40, 64, 136):
                pl, pr, t_in = _geometry((k, s, d), "centred", 8)
                f = N.ConvArgs()
                f.c_in, f.c_out, f.kernel, f.stride, f.dilation, f.pad_left, f.pad_right = c_in, c_out, k, s, d, pl, pr
                f.batch, f.t_in, f.t_out, f.precision = 1, t_in, 8, N.PREC_F32
                dummy = torch.zeros(4, device=DEV)
                f.x = f.y = f.weight = dummy.data_ptr()     # the forward checks for NULL first; nothing is launched
                rf = min(N.lib.rave_conv1d_configs(C.byref(f), None, 0), 0)
                c = dict(c_in=c_in, c_out=c_out, k=k, s=s, d=d, pl=pl, pr=pr, act=0, slope=0.2, B=1, t_in=t_in, t_out=8)
                rb = min(N.lib.rave_conv1d_backward_workspace(C.byref(_args(c))), 0)
                assert rf == rb, ((k, s, d), c_in, c_out, rf, rb)


# ================================================================== 2. split and unsplit
@pytest.mark.parametrize("fam", [(1, 1, 1), (3, 1, 1), (7, 1, 1), (4, 2, 1), (8, 4, 1)])      # one per weight-kernel instance
def test_split_and_unsplit_paths(fam):
    split = _case(fam, "centred", G.ACT_LEAKY, 3, 16, 16, 700, seed=11)       # 33 chunks of 64 columns, one tile
    out, nws = _bwd(split)
    assert nws > 0
    _held(f"{fam} split-K", out, split)
    again, _ = _bwd(split)
    assert all(same_bits(out[k], again[k]) for k in out)
    one = _case(fam, "centred", G.ACT_LEAKY, 1, 16, 16, 129, seed=12)         # 3 chunks: below four per split
    out, nws = _bwd(one)
    assert nws == 0
    _held(f"{fam} unsplit", out, one)
    snake = _case(fam, "centred", G.ACT_SNAKE, 1, 16, 16, 129, seed=13)       # alpha partials only
    assert _bwd(snake)[1] > 0 and _bwd(snake, want=("gx", "gw", "gb"))[1] == 0


# ================================================================== 3. unit cotangents
@pytest.mark.parametrize("fam", G.FAMILIES)
def test_unit_cotangents(fam):
    k, s, d = fam
    c = _case(fam, "centred", G.ACT_LEAKY, 2, 40, 16, 65, seed=21)
    c["w"] = (1.0 + np.arange(16 * 40 * k, dtype=np.float32).reshape(16, 40, k))      # every tap distinct
    b0, m0 = 1, 5
    a_ref = np.where(c["x"] > 0, c["x"], c["x"] * np.float32(0.2)).astype(np.float32)
    for n0 in (0, 31, 64):
        c["gy"] = np.zeros((2, 16, 65), np.float32)
        c["gy"][b0, m0, n0] = 1.0
        hot = dict(c, act=G.ACT_NONE)
        ga = _bwd(hot, want=("gx",))[0]["gx"].cpu().numpy()
        gw = _bwd(c, want=("gw",))[0]["gw"].cpu().numpy()
        want_ga = np.zeros_like(ga)
        want_gw = np.zeros_like(gw)
        for j in range(k):
            t = n0 * s + j * d - c["pl"]
            if 0 <= t < c["t_in"]:
                want_ga[b0, :, t] = c["w"][m0, :, j]
                want_gw[m0, :, j] = a_ref[b0, :, t]
        assert np.array_equal(ga.view(np.uint32), want_ga.view(np.uint32))
        assert np.array_equal(gw.view(np.uint32), want_gw.view(np.uint32))


# ================================================================== 4. NULL outputs, zeros, reruns
@pytest.mark.parametrize("fam", [(3, 1, 9), (4, 2, 1)])
def test_null_outputs_zero_cotangent_and_reruns(fam):
    c = _case(fam, "causal", G.ACT_SNAKE, 3, 40, 64, 257, seed=31)
    full, nws = _bwd(c)
    assert nws > 0
    again, _ = _bwd(c)
    assert all(same_bits(full[k], again[k]) for k in full)
    for drop in ("gx", "gw", "gb", "ga"):
        rest = tuple(k for k in ("gx", "gw", "gb", "ga") if k != drop)
        part, _ = _bwd(c, want=rest)
        assert set(part) == set(rest) and all(same_bits(part[k], full[k]) for k in rest), drop
    bias_only, _ = _bwd(c, want=("gb",), null_x=False)
    assert same_bits(bias_only["gb"], full["gb"])
    z = dict(c, gy=np.zeros_like(c["gy"]))
    out, _ = _bwd(z)
    assert all(bool((v == 0).all()) for v in out.values())


def test_missing_x_is_refused_only_where_needed():
    N = _N()
    c = _case((3, 1, 1), "centred", G.ACT_NONE, 1, 16, 16, 32)
    out, _ = _bwd(c, want=("gx", "gb"), null_x=True)                       # neither needs x
    full, _ = _bwd(c)
    assert same_bits(out["gx"], full["gx"]) and same_bits(out["gb"], full["gb"])
    assert _bwd(c, want=("gw",), null_x=True, check=False)[0] == N.RAVE_ERR_ARG
    assert "needs the input x" in N.lib.rave_last_error().decode()
    assert _bwd(dict(c, act=G.ACT_LEAKY), want=("gx",), null_x=True, check=False)[0] == N.RAVE_ERR_ARG
    assert _bwd(c, check=False, transposed=1)[0] == N.RAVE_ERR_ARG
    assert "transposed" in N.lib.rave_last_error().decode()
    assert _bwd(c, check=False, precision=N.PREC_SPLIT16)[0] == N.RAVE_ERR_ARG
    assert "precision" in N.lib.rave_last_error().decode()


# ================================================================== 5. the public surface
def _conv(*a, cached=False, precision="f32", cls="Conv1d", **kw):
    from rave_amd import cc
    cc.use_cached_conv(cached)
    cc.set_precision(precision)
    try:
        return getattr(cc, cls)(*a, **kw).to(DEV)
    finally:
        cc.use_cached_conv(False)
        cc.set_precision("f32")


def test_new_symbols_and_ops_exist():
    N = _N()
    for name in ("rave_conv1d_backward_data", "rave_conv1d_backward_weight", "rave_conv1d_backward_workspace"):
        assert hasattr(N.lib, name)
    from rave_amd import cc  # noqa: F401
    assert torch.ops.rave_amd.conv1d_w and torch.ops.rave_amd.conv1d_backward


def test_conv1d_is_differentiable():
    """weight.grad, bias.grad and x.grad bit for bit the C boundary's and within 4 e_ref;
    the output under grad bit for bit the no-grad output."""
    from rave_amd import cc
    torch.manual_seed(0)
    conv = _conv(16, 32, 3, padding=cc.get_padding(3, dilation=3), dilation=3)
    x = torch.randn(2, 16, 200, device=DEV, requires_grad=True)
    y = conv(x)
    assert y.grad_fn is not None and y.shape == (2, 32, 200)
    with torch.no_grad():
        y0 = conv(x)
    assert y0.grad_fn is None and same_bits(y0, y)
    y.sum().backward()
    pl, pr = cc.get_padding(3, dilation=3)
    c = dict(x=x.detach().cpu().numpy(), w=conv.weight.detach().cpu().numpy(), gy=np.ones((2, 32, 200), np.float32),
             alpha=np.zeros(16, np.float32), k=3, s=1, d=3, pl=pl, pr=pr, act=G.ACT_NONE, slope=0.2, t_in=200, t_out=200,
             B=2, c_in=16, c_out=32)
    want, _ = _bwd(c)
    assert same_bits(x.grad, want["gx"]) and same_bits(conv.weight.grad, want["gw"]) and same_bits(conv.bias.grad, want["gb"])
    _held("cc.Conv1d(16, 32, 3, dilation=3)", dict(gx=x.grad, gw=conv.weight.grad, gb=conv.bias.grad), c)


def test_weight_norm_gets_its_gradients():
    """weight_g.grad, weight_v.grad and bias.grad against fp32 torch autograd of the same
    composition on the same GPU (1e-3 of each gradient's max: the plumbing through the
    weight_norm edge; the kernels' bound is held above)."""
    import torch.nn.functional as F
    torch.manual_seed(2)
    conv = torch.nn.utils.weight_norm(_conv(16, 16, 3, padding=(1, 1)))
    with torch.no_grad():
        conv.weight_g.mul_(torch.rand_like(conv.weight_g) + 0.5)          # g off its initial |v|
    x = torch.randn(2, 16, 64, device=DEV)
    y = conv(x)
    assert y.grad_fn is not None
    gy = torch.randn_like(y)
    y.backward(gy)
    g, v, b = (t.detach().clone().requires_grad_(True) for t in (conv.weight_g, conv.weight_v, conv.bias))
    w = torch._weight_norm(v, g, 0)
    ref = F.conv1d(F.pad(x, (1, 1)), w, b)
    assert float((ref - y).detach().abs().max()) < 1e-4
    ref.backward(gy)
    for got, want in ((conv.weight_g, g), (conv.weight_v, v), (conv.bias, b)):
        assert got.grad is not None and got.grad.shape == want.grad.shape
        assert float((got.grad - want.grad).abs().max()) <= 1e-3 * float(want.grad.abs().max())


def test_frozen_weight_and_input_only_paths():
    """Only x asks for a gradient (frozen layer), and only the parameters do: the same bits as the full call."""
    conv = _conv(16, 32, 3, padding=(1, 1))
    x = torch.randn(2, 16, 100, device=DEV)
    gy = torch.randn(2, 32, 100, device=DEV)
    xa = x.clone().requires_grad_(True)
    conv(xa).backward(gy)
    full = (xa.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    conv.zero_grad(set_to_none=True)
    conv(x).backward(gy)                                   # x without grad: the weight is not saved
    assert same_bits(conv.weight.grad, full[1]) and same_bits(conv.bias.grad, full[2])
    for p in conv.parameters():
        p.requires_grad_(False)
    xb = x.clone().requires_grad_(True)
    conv(xb).backward(gy)                                  # frozen, no activation: x is not saved
    assert same_bits(xb.grad, full[0])


# an input column that no valid output reads may hold anything: the right tail a stride
# leaves, and the gaps of a dilated tap set around a short output
@pytest.mark.parametrize("fam,pad,t_out", [((4, 2, 1), "tail", 65), ((8, 4, 1), "tail", 33), ((3, 1, 16), "none", 1),
                                           ((3, 1, 9), "none", 2)])
def test_unread_input_columns_may_hold_nan(fam, pad, t_out):
    k, s, d = fam
    c = _case(fam, pad, G.ACT_LEAKY, 2, 40, 16, t_out, seed=41)
    read = np.zeros(c["t_in"], bool)
    for j in range(k):
        t = np.arange(t_out) * s + j * d - c["pl"]
        read[t[(t >= 0) & (t < c["t_in"])]] = True
    assert not read.all()
    clean, _ = _bwd(c, want=("gw", "gb"))
    dirty = dict(c, x=c["x"].copy())
    dirty["x"][:, :, ~read] = np.nan
    out, _ = _bwd(dirty, want=("gw", "gb"))
    assert same_bits(out["gw"], clean["gw"]) and same_bits(out["gb"], clean["gb"])
    gx = _bwd(dict(dirty, act=G.ACT_NONE), want=("gx",))[0]["gx"]
    assert bool((gx[:, :, torch.from_numpy(~read).to(DEV)] == 0).all()) and bool(torch.isfinite(gx).all())


def test_dilated_unit_with_snake_through_the_module_tree():
    """x.grad, the residual's grad, both convs' parameter grads and both Snake alphas'
    grads, against fp32 torch autograd of the modules' own expressions on the same GPU
    (1e-3 of each gradient's max: a plumbing check, the kernels' bound is held above)."""
    import torch.nn.functional as F
    from rave_amd import modules as M
    torch.manual_seed(1)
    unit = M.DilatedUnit(16, 3, 3, activation="snake").to(DEV)
    snakes, convs = [unit.net[0], unit.net[2]], [unit.net[1], unit.net[3]]
    assert all(isinstance(m, M.Snake) for m in snakes)
    with torch.no_grad():
        for sn in snakes:
            sn.alpha.uniform_(0.5, 2.0)
    x = torch.randn(2, 16, 130, device=DEV, requires_grad=True)
    res = torch.randn(2, 16, 130, device=DEV, requires_grad=True)
    y = unit(x, res)
    assert y.grad_fn is not None
    gy = torch.randn_like(y)
    y.backward(gy)
    # the same tree in torch
    leaves = [t.detach().clone().requires_grad_(True) for t in
              (x, res, snakes[0].alpha, snakes[1].alpha, convs[0].weight, convs[0].bias, convs[1].weight, convs[1].bias)]
    xr, rr, a0, a1, w0, b0, w1, b1 = leaves
    h = xr
    for al, w, b, cv in ((a0, w0, b0, convs[0]), (a1, w1, b1, convs[1])):
        a = h + (al + 1e-9).reciprocal() * (al * h).sin().pow(2)            # modules.Snake.forward
        h = F.conv1d(F.pad(a, (cv.pad_l, cv.pad_r)), w, b, dilation=cv.dilation)
    (h + rr).backward(gy)
    assert same_bits(res.grad, gy)
    got = (x, res, snakes[0].alpha, snakes[1].alpha, convs[0].weight, convs[0].bias, convs[1].weight, convs[1].bias)
    for g, r in zip(got, leaves):
        assert g.grad is not None and g.grad.shape == r.grad.shape
        assert float((g.grad - r.grad).abs().max()) <= 1e-3 * float(r.grad.abs().max())


def test_other_modes_carry_no_grad_fn():
    x = torch.randn(1, 16, 64, device=DEV, requires_grad=True)
    assert _conv(16, 16, 3, padding=(1, 1), precision="split16")(x).grad_fn is None
    assert _conv(16, 16, 3, padding=(1, 1), cached=True)(x).grad_fn is None
    assert _conv(16, 16, 4, stride=2, padding=1, cls="ConvTranspose1d")(x).grad_fn is None


def test_double_backward_raises():
    conv = _conv(16, 16, 3, padding=(1, 1))
    x = torch.randn(1, 16, 64, device=DEV, requires_grad=True)
    with pytest.raises((NotImplementedError, RuntimeError), match="double backward"):
        torch.autograd.grad(conv(x).sum(), x, create_graph=True)


# ================================================================== 6. end to end
# Conv1d(64, rows, 7) -> CachedPQMF.inverse(., mode, noise) -> sum(MultiResolutionSTFTLoss) on a
# (2, 64, 256) input: GeneratorV2's last conv in front of its head, with amplitude modulation
# (32 rows, mode 1) and without (16 rows, mode 2; inverse's mode 1 takes 2 x 16 rows).
E2E_CASES = [(16, 2), (32, 1)]


@functools.lru_cache(maxsize=None)
def _e2e_inputs(rows, mode):
    """x, weight, bias, residual, noise, target.  The conv's output is pinned to
    tests/test_gpu_pqmf_grad.py's multiband tensor (whose synthesis is close to
    tests/stft_loss_ref.py's case a prediction, so that nearly no bin of the
    reference sits under the loss's power clamp) through the fused residual:
    res = that tensor - conv(x) in float64, so conv(x) + res is it up to one rounding."""
    from tests.test_gpu_pqmf_grad import _e2e_inputs as pqmf_inputs
    y_mb, noise, target = pqmf_inputs()
    y64 = y_mb.astype(np.float64)
    if mode == 2:                                          # the same pre-tanh value without the gate
        y64 = y64[:, :16] / (1.0 + np.exp(-y64[:, 16:]))
    assert y64.shape == (2, rows, 256)
    rng = np.random.default_rng(1907)
    x = rng.standard_normal((2, 64, 256)).astype(np.float32)
    w = (rng.standard_normal((rows, 64, 7)) / np.sqrt(64 * 7)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(rows)).astype(np.float32)
    y0 = G.forward(x, w, bias, None, None, 7, 1, 1, 3, 3, G.ACT_NONE, 0.2)
    return x, w, bias, (y64 - y0).astype(np.float32), noise, target


@functools.lru_cache(maxsize=None)
def _e2e_ref(rows, mode):
    """CPU autograd of the oracle composition (F.pad + F.conv1d + residual, oracle/torch_cpu.py's
    inverse behind the head in torch, tests/stft_loss_ref.py's loss): the float64 gradients of
    the conv's weight and input, the fp32 ones, and the share of clamped bins."""
    import torch.nn.functional as F
    from tests import stft_loss_ref as S
    from tests.test_gpu_pqmf_grad import _filters
    from tests.test_pqmf_grad_ref_host import _head, _oracle_inverse
    _, hki = _filters()
    x, w, bias, res, noise, target = _e2e_inputs(rows, mode)
    resolutions = S.fork_resolutions(44100)
    out = {}
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(a).to(dtype)
        xt, wt = t(x).requires_grad_(True), t(w).requires_grad_(True)
        y = F.conv1d(F.pad(xt, (3, 3)), wt, t(bias)) + t(res)
        audio = _oracle_inverse(_head(y, mode, t(noise)), t(hki), False)
        sc, mag = S.mr_loss(audio, t(target), resolutions)
        out[dtype] = torch.autograd.grad(sc + mag, (wt, xt))
        if dtype == torch.float64:
            out["share"] = S.clamped_share(audio.detach(), resolutions)
    return out


@pytest.mark.parametrize("rows,mode", E2E_CASES)
def test_loss_gradient_reaches_the_conv(rows, mode):
    """weight.grad and x.grad of the conv within 4 e_ref of the float64 CPU gradient, in max-abs
    and in relative L2; e_ref the CPU fp32 autograd gradient's error against it.  The cotangent
    arrives from the PQMF adjoint (section 18), whose own comes from the loss kernels (section 17).
    Measured on the MI355X, kernel / e_ref in max-abs and L2: weight.grad 0.10 and 0.14, x.grad
    0.13 and 0.14 (16 rows, mode 2); 0.25 and 0.28, 0.28 and 0.29 (32 rows, mode 1); e_ref itself
    is 4 to 7 % in L2, one fp32 rounding of the conv's output under the log term."""
    from rave_amd import cc
    from rave_amd.distance import MultiResolutionSTFTLoss
    from tests.test_gpu_pqmf_grad import _pqmf
    ref = _e2e_ref(rows, mode)
    assert ref["share"] < 1e-4, ref["share"]
    x, w, bias, res, noise, target = _e2e_inputs(rows, mode)
    conv = _conv(64, rows, 7, padding=cc.get_padding(7))
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
        conv.bias.copy_(torch.from_numpy(bias))
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = conv(xt, torch.from_numpy(res).to(DEV))
    audio = _pqmf().inverse(y, mode, torch.from_numpy(noise).to(DEV))[:, 0]
    assert audio.shape == (2, 4096)
    loss = sum(MultiResolutionSTFTLoss.for_sample_rate(44100)(audio, torch.from_numpy(target).to(DEV)))
    loss.backward()
    fails = []
    for name, got, g64, g32 in zip(("weight", "x"), (conv.weight.grad, xt.grad), ref[torch.float64], ref[torch.float32]):
        def errs(g):
            d = g.double().cpu() - g64
            return float(d.abs().max()), float(d.norm() / g64.norm())
        (e_abs, e_l2), (k_abs, k_l2) = errs(g32), errs(got)
        print(f"end to end rows {rows} mode {mode} {name}.grad: clamped share {ref['share']:.2e}; e_ref max-abs {e_abs:.3e} "
              f"L2 {e_l2:.3e}; kernel {k_abs:.3e} {k_l2:.3e}; ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
        assert bool(torch.isfinite(got).all())
        if not (k_abs <= 4 * e_abs and k_l2 <= 4 * e_l2):
            fails.append((name, k_abs, e_abs, k_l2, e_l2))
    assert not fails, fails
