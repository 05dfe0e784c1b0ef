"""The differentiable spectral losses on the GPU (rave_stft_loss_forward /
rave_stft_loss_backward, rave_amd/csrc/stft_loss.hip) against float64 torch.stft
and torch autograd on the CPU (tests/stft_loss_ref.py, which
tests/golden/make_stft_loss_check.py checks against the reference's own
functions to 1e-12).

Multi-resolution shapes, with the fork's three resolutions (2048, 220, 1102),
(4096, 441, 2205), (512, 88, 441): a (2, 4096); b (3, 5000), T no multiple of
any hop; c (1, 2049), the smallest T that n_fft = 4096's reflect pad accepts.
An odd geometry (64, 5, 37) at (2, 300) runs the general framing off the fork's
numbers (16 frames per transform, 61 frames: a partial tile).  AudioDistanceV1:
the cases a / b / c of tests/distance_ref.py at both epsilons.

Forward bar: 1e-4 relative, the project's parity bar for these sums.  Gradient
bar: 4 e_ref in max-abs and in relative L2 over the whole gradient, e_ref being
the same error of CPU fp32 torch autograd against float64 on the same input,
computed here (the log terms amplify any fp32 rounding by 1 / magnitude and
flip sign on it, so no constant bound holds)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import distance_ref as D
from tests import stft_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY = 1e-4
FORK = R.fork_resolutions()
KINDS = ("sc", "mag", "sum")


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def errs(got: torch.Tensor, want: torch.Tensor):
    """(max-abs, relative L2) of got against the float64 want."""
    d = got.double() - want
    return float(d.abs().max()), float(d.norm() / want.norm())


def _mr_data(case):
    return (R.odd_inputs(), R.ODD) if case == "odd" else (R.mr_inputs(case), FORK)


@functools.lru_cache(maxsize=None)
def _mr_ref(case):
    """CPU reference of one case, computed once: float64 values, per-resolution
    terms and the gradients of sc, mag and sc + mag; the same gradients in fp32."""
    (pred, target), res = _mr_data(case)

    def fn(dtype):
        t = torch.from_numpy(target).to(dtype)

        def f(v):
            sc, mag = R.mr_loss(v, t, res)
            return sc, mag, sc + mag
        return f
    vals, g64 = R.grad_of(fn(torch.float64), pred, torch.float64)
    _, g32 = R.grad_of(fn(torch.float32), pred, torch.float32)
    terms = [(float(s), float(m)) for s, m in R.mr_terms(torch.from_numpy(pred).double(),
                                                         torch.from_numpy(target).double(), res)]
    share = R.clamped_share(torch.from_numpy(pred).double(), res)
    return dict(vals=vals, terms=terms, g64=dict(zip(KINDS, g64)), g32=dict(zip(KINDS, g32)), share=share)


@functools.lru_cache(maxsize=None)
def _mr_gpu(case):
    """The kernels' values, terms and the three gradients, computed once."""
    from rave_amd.distance import MultiResolutionSTFTLoss
    (pred, target), res = _mr_data(case)
    loss = MultiResolutionSTFTLoss(res)
    p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    t = torch.from_numpy(target).to(DEV)
    sc, mag = loss(p, t)
    assert sc.grad_fn is not None and mag.grad_fn is not None
    g = {"sc": torch.autograd.grad(sc, p, retain_graph=True)[0],
         "mag": torch.autograd.grad(mag, p, retain_graph=True)[0],
         "sum": torch.autograd.grad(sc + mag, p)[0]}
    terms = [(float(a), float(b)) for a, b in loss.terms(p, t)]
    return dict(vals=(float(sc.detach()), float(mag.detach())), terms=terms, g={k: v.cpu() for k, v in g.items()})


@functools.lru_cache(maxsize=None)
def _v1_ref(case, e):
    x, y = D.inputs(case)

    def fn(dtype):
        xt = torch.from_numpy(x).to(dtype)
        return lambda v: (R.v1_distance(xt, v, D.DEFAULT_SCALES, D.EPS[e]),)
    vals, g64 = R.grad_of(fn(torch.float64), y, torch.float64)
    _, g32 = R.grad_of(fn(torch.float32), y, torch.float32)
    return vals[0], g64[0], g32[0]


def _v1_gpu(case, e):
    from rave_amd.distance import AudioDistance
    x, y = (torch.from_numpy(v).to(DEV) for v in D.inputs(case))
    y.requires_grad_(True)
    d = AudioDistance(D.DEFAULT_SCALES, D.EPS[e])(x, y)["spectral_distance"]
    assert d.grad_fn is not None and d.dim() == 0
    (g,) = torch.autograd.grad(d, y)
    return float(d.detach()), g.cpu()


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", ["a", "b", "c", "odd"])
def test_multires_forward(case):
    ref, got = _mr_ref(case), _mr_gpu(case)
    print(f"multires {case}: sc {rel(got['vals'][0], ref['vals'][0]):.2e} mag {rel(got['vals'][1], ref['vals'][1]):.2e}")
    assert rel(got["vals"][0], ref["vals"][0]) <= PARITY
    assert rel(got["vals"][1], ref["vals"][1]) <= PARITY
    assert len(got["terms"]) == len(ref["terms"])
    for (gs, gm), (ws, wm) in zip(got["terms"], ref["terms"]):
        print(f"  sc {rel(gs, ws):.2e} mag {rel(gm, wm):.2e}")
        assert rel(gs, ws) <= PARITY and rel(gm, wm) <= PARITY


@pytest.mark.parametrize("e", ["e7", "e0"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_v1_forward(case, e):
    want = _v1_ref(case, e)[0]
    got = _v1_gpu(case, e)[0]
    print(f"v1 {case} {e}: rel {rel(got, want):.2e}")
    assert rel(got, want) <= PARITY
    x, y = (torch.from_numpy(v).double() for v in D.inputs(case))
    assert rel(want, D.distance(x, y, D.DEFAULT_SCALES, D.EPS[e])) <= 1e-12      # the restatement is distance_ref's


# ------------------------------------------------------------------ gradients
def test_odd_geometry_gradient():
    """The general framing of the backward -- window offset 13, hop 5, win 37,
    the gather's frame ranges and fold-back -- through the spectral-convergence
    term.  The path from the per-bin G to the gradient is the same for both
    terms; the log term's per-bin weight is checked on the three shapes above.
    It is not compared here: 5 of this input's 20130 bins sit under the clamp
    (2.5e-4, above the 1e-4 the parity test allows) and those just above it
    carry a 1 / magnitude^2 weight about a thousand times the typical one, so
    both metrics are the rounding error of a handful of bins (measured on the
    MI355X: 6.0 and 5.6 e_ref)."""
    ref, got = _mr_ref("odd"), _mr_gpu("odd")
    want = ref["g64"]["sc"]
    e_abs, e_l2 = errs(ref["g32"]["sc"], want)
    k_abs, k_l2 = errs(got["g"]["sc"], want)
    print(f"odd geometry grad sc: ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
    assert k_abs <= 4 * e_abs and k_l2 <= 4 * e_l2
    m = 33                                                # n_fft/2 + 1: the fold-back region
    for sl in (slice(0, m), slice(-m, None)):
        e_abs, _ = errs(ref["g32"]["sc"][:, sl], want[:, sl])
        k_abs, _ = errs(got["g"]["sc"][:, sl], want[:, sl])
        assert k_abs <= 4 * e_abs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_multires_gradient(case, kind):
    ref, got = _mr_ref(case), _mr_gpu(case)
    assert ref["share"] <= 1e-4, "the clamp branch must not mask an error"
    want = ref["g64"][kind]
    e_abs, e_l2 = errs(ref["g32"][kind], want)
    k_abs, k_l2 = errs(got["g"][kind], want)
    assert got["g"][kind].shape == want.shape and got["g"][kind].dtype == torch.float32
    print(f"multires grad {case} {kind}: e_ref max-abs {e_abs:.3e} L2 {e_l2:.3e}; kernel {k_abs:.3e} {k_l2:.3e}; "
          f"ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
    assert k_abs <= 4 * e_abs
    assert k_l2 <= 4 * e_l2


@pytest.mark.parametrize("e", ["e7", "e0"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_v1_gradient(case, e):
    _, want, g32 = _v1_ref(case, e)
    got = _v1_gpu(case, e)[1]
    assert got.shape == want.shape == D.CASES[case]
    e_abs, e_l2 = errs(g32, want)
    k_abs, k_l2 = errs(got, want)
    print(f"v1 grad {case} {e}: e_ref max-abs {e_abs:.3e} L2 {e_l2:.3e}; kernel {k_abs:.3e} {k_l2:.3e}; "
          f"ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
    assert k_abs <= 4 * e_abs
    assert k_l2 <= 4 * e_l2


@pytest.mark.parametrize("kind", KINDS)
def test_reflect_fold_back(kind):
    """Case c: the first and the last n_fft/2 + 1 samples of the gradient, where
    the reflect pads fold back onto the signal, per resolution."""
    ref, got = _mr_ref("c"), _mr_gpu("c")
    for n_fft, _, _ in FORK:
        m = n_fft // 2 + 1
        for name, sl in (("first", slice(0, m)), ("last", slice(-m, None))):
            want = ref["g64"][kind][:, sl]
            e_abs, e_l2 = errs(ref["g32"][kind][:, sl], want)
            k_abs, k_l2 = errs(got["g"][kind][:, sl], want)
            print(f"fold-back {kind} {name} {m}: ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
            assert k_abs <= 4 * e_abs and k_l2 <= 4 * e_l2, (n_fft, name)


# ------------------------------------------------------------------ edges
def test_zero_pred_has_zero_gradient():
    """Every bin of pred = 0 sits under the clamp, whose derivative is 0."""
    from rave_amd.distance import MultiResolutionSTFTLoss
    target = R.mr_inputs("b")[1]
    p = torch.zeros(target.shape, device=DEV, requires_grad=True)
    sc, mag = MultiResolutionSTFTLoss(FORK)(p, torch.from_numpy(target).to(DEV))
    (g,) = torch.autograd.grad(sc + mag, p)
    assert bool((g == 0).all())
    sc, mag = sc.detach(), mag.detach()
    wsc, wmag = R.mr_loss(torch.zeros(target.shape, dtype=torch.float64), torch.from_numpy(target).double(), FORK)
    assert np.isfinite(float(sc)) and np.isfinite(float(mag))
    assert rel(sc, wsc) <= PARITY and rel(mag, wmag) <= PARITY


@pytest.mark.parametrize("e", ["e7", "e0"])
def test_v1_zero_value_is_finite(e):
    """y = 0: no NaN in the distance or its gradient.  The value shares its FFT
    with the target, whose rounding noise (about 1e-7 of its spectrum) is what
    the kernel sees in place of an exact zero: at eps = 1 that is invisible and
    the distance equals the reference's; at eps = 1e-7 it is not compared."""
    from rave_amd.distance import AudioDistance
    x = torch.from_numpy(D.inputs("b")[0]).to(DEV)
    y = torch.zeros_like(x, requires_grad=True)
    d = AudioDistance(D.DEFAULT_SCALES, D.EPS[e])(x, y)["spectral_distance"]
    (g,) = torch.autograd.grad(d, y)
    d = d.detach()
    assert bool(torch.isfinite(d)) and bool(torch.isfinite(g).all())
    if e == "e0":
        want = D.distance(x.cpu().double(), torch.zeros(x.shape, dtype=torch.float64), D.DEFAULT_SCALES, 1.0)
        assert rel(d, want) <= PARITY


# ------------------------------------------------------------------ upstream gradient, determinism, graphs
def _loss_and_inputs(case="b"):
    from rave_amd.distance import MultiResolutionSTFTLoss
    pred, target = R.mr_inputs(case)
    return (MultiResolutionSTFTLoss(FORK), torch.from_numpy(pred).to(DEV).requires_grad_(True),
            torch.from_numpy(target).to(DEV))


def test_upstream_weight():
    """The fork's weighting (rave/model.py:386-391): 2.5 (sc + mag)."""
    ref = _mr_ref("b")
    loss, p, t = _loss_and_inputs()
    sc, mag = loss(p, t)
    (2.5 * (sc + mag)).backward()
    want = 2.5 * ref["g64"]["sum"]
    e_abs, e_l2 = errs(2.5 * ref["g32"]["sum"], want)
    k_abs, k_l2 = errs(p.grad.cpu(), want)
    print(f"upstream 2.5: ratios {k_abs / e_abs:.2f} {k_l2 / e_l2:.2f}")
    assert k_abs <= 4 * e_abs and k_l2 <= 4 * e_l2


def test_unused_output_contributes_zero():
    """grad_out = (1, 0) is the gradient of sc alone, bit for bit."""
    loss, p, t = _loss_and_inputs()
    sc, mag = loss(p, t)
    (alone,) = torch.autograd.grad(sc, p, retain_graph=True)
    (both,) = torch.autograd.grad(sc + 0.0 * mag, p)
    assert torch.equal(alone, both)


def test_backward_is_bitwise_reproducible():
    from rave_amd.distance import MultiResolutionSTFTLoss
    loss, p, t = _loss_and_inputs()
    sc, mag = loss(p, t)
    (first,) = torch.autograd.grad(sc + mag, p, retain_graph=True)
    first = first.clone()
    (second,) = torch.autograd.grad(sc + mag, p)
    assert torch.equal(first, second)
    sc, mag = MultiResolutionSTFTLoss(FORK)(p, t)              # fresh tables and workspace
    assert torch.equal(first, torch.autograd.grad(sc + mag, p)[0])


def test_graph_replay_follows_a_device_grad_out():
    """Forward + backward captured once; the upstream weights live on the device
    and change between replays, and each replay equals the eager result bit for
    bit (no host sync, no allocation in the library)."""
    loss, p, t = _loss_and_inputs()
    w = torch.tensor([1.0, 1.0], device=DEV)

    def step():
        sc, mag = loss(p, t)
        return torch.autograd.grad(w[0] * sc + w[1] * mag, p)[0]
    eager = {}
    for a, b in ((1.0, 1.0), (2.5, 0.5)):
        w.copy_(torch.tensor([a, b]))
        eager[(a, b)] = step().clone()
    torch.cuda.synchronize()
    assert not torch.equal(eager[(1.0, 1.0)], eager[(2.5, 0.5)])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for a, b in ((1.0, 1.0), (2.5, 0.5)):
        w.copy_(torch.tensor([a, b]))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[(a, b)]), (a, b)


# ------------------------------------------------------------------ existing behaviour, plumbing
def test_audio_distance_without_grad_has_not_moved():
    """No requires_grad: the bits of rave_audio_distance called directly."""
    from rave_amd import _native as N
    from rave_amd.distance import AudioDistance
    x, y = (torch.from_numpy(v).to(DEV) for v in D.inputs("b"))
    dist = AudioDistance()
    got = dist(x, y)["spectral_distance"]
    assert got.grad_fn is None and dist._loss is None
    rows, T = x.shape[0] * x.shape[1], x.shape[2]
    a = N.DistanceArgs(rows=rows, t_len=T, n_scales=len(D.DEFAULT_SCALES), log_epsilon=1e-7)
    tables = [torch.from_numpy(N.pack_stft_table(n)).to(DEV) for n in D.DEFAULT_SCALES]
    for i, n in enumerate(D.DEFAULT_SCALES):
        a.scales[i], a.tables[i] = n, tables[i].data_ptr()
    work = torch.empty(int(N.lib.rave_audio_distance_workspace(C.byref(a))) // 4, device=DEV)
    out = torch.empty(1 + 2 * len(D.DEFAULT_SCALES), device=DEV)
    a.x, a.y, a.workspace, a.out = x.data_ptr(), y.data_ptr(), work.data_ptr(), out.data_ptr()
    N.check(N.lib.rave_audio_distance(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "distance")
    torch.cuda.synchronize()
    assert torch.equal(got, out[0])
    with torch.no_grad():                                       # requires_grad without a graph: the old path too
        d = dist(x, y.clone().requires_grad_(True))["spectral_distance"]
    assert torch.equal(d, out[0]) and dist._loss is None


def test_autograd_plumbing():
    from rave_amd.distance import AudioDistance
    loss, p, t = _loss_and_inputs("a")
    sc, mag = loss(p, t)
    (g,) = torch.autograd.grad(sc + mag, p, retain_graph=True)
    assert g.shape == p.shape and g.dtype == torch.float32 and g.device == p.device
    # through earlier autograd ops, and a non-contiguous value
    base = torch.cat([p.detach(), p.detach()], 0).repeat_interleave(2, 1).requires_grad_(True)    # (4, 2T)
    view = base[:2, ::2]
    assert not view.is_contiguous() and torch.equal(view, p.detach())
    sc2, mag2 = loss(view, t)
    (gb,) = torch.autograd.grad(sc2 + mag2, base)
    assert gb.shape == base.shape
    assert torch.equal(gb[:2, ::2], g) and not gb[2:].any() and not gb[:, 1::2].any()
    # V1 through (B, C, T)
    x, y = (torch.from_numpy(v).to(DEV) for v in D.inputs("b"))
    y.requires_grad_(True)
    d = AudioDistance()(x, y)["spectral_distance"]
    (gy,) = torch.autograd.grad(d, y)
    assert gy.shape == y.shape
    with pytest.raises(ValueError, match="target is constant"):
        loss(p, t.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="target is constant"):
        AudioDistance()(x.clone().requires_grad_(True), y)


def test_double_backward_raises():
    loss, p, t = _loss_and_inputs("a")
    sc, mag = loss(p, t)
    (g,) = torch.autograd.grad(sc + mag, p, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), p)
