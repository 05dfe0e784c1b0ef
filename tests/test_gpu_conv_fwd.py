"""The forward kernels of the inference path (rave_conv1d, rave_residual_unit,
rave_residual_stack) through the C boundary, against tests/conv_fwd_ref.py (which
tests/test_conv_fwd_ref_host.py pins to torch and the oracle on the CPU).

Every call goes through interior views of larger NaN-filled buffers: x, y and
the residual start at an offset, x's rows are 16-byte aligned with a channel
stride of a multiple of 4 floats and a padded batch stride, y's rows are aligned
in one case and not in the next.  After each call the output is finite, every
guard word of the y buffer has its bits from before, the arrival counters of the
workspace are zero, and a second call gives the first call's bits.

Bounds, per output tensor, e_ref the restatement's float32 run against its
float64 run and S the condition sum of an output:
  f32, f32_ring and the skinny-N (gemv) tiles, exact fp32 chains: err <= 4 e_ref.
  bf16x3 and split16: err <= K e_ref with one K per mode and kernel (BOUND), never
  above the older 2e-5 max(1, max |ref|); K is the next power of two at or above
  twice the worst err / e_ref measured over this module on the MI355X (the factor
  2 for the spread between seeds and split orders), and for bf16x3 K <= 8 (its
  error is documented as within 1.5x of exact fp32).  split16 is also held, per
  output, to the header's model 4 e_ref + 2^-21 S (twice the 2^-23 per operand).

Measured on the MI355X, worst err / e_ref over this module (8546 judged calls: the
sweep, every launch configuration at T in {1, 33, 129}, the options, units, cooperative
forms and stacks), and the K that follows:
             f32    f32_ring  gemv tiles  bf16x3       split16
    conv     1.79   1.96      2.08        1.71 -> 4    2.73 -> 8
    unit     1.38   1.44      -           1.35 -> 4    1.24 -> 4
    stack    -      -         -           1.02 -> 4    1.16 -> 4
Worst err / S: conv 3.4e-7 (f32), 2.8e-7 (bf16x3, split16); unit 1.1e-7 (f32, f32_ring),
4.5e-8 (bf16x3), 5.7e-8 (split16); stack 2.8e-8 (both).  No split16 output left the
header's model, and no bound met the 2e-5 ceiling.

The sweep's T is the GEMM's column count: t_out of a conv, and for the transposed
conv the columns per phase, t_in - pad_left (t_out = T r).

The f32_ring and bf16x3 convs take 16-byte window pieces and refuse t_in % 4 != 0
whatever the strides are ("needs 16-byte aligned input rows and t_in % 4 == 0").
Where a case has such a t_in the refusal is asserted, and the two modes then run
the same t_out on the input without its last t_in % 4 columns, the right padding
that much larger (none exists for the transposed conv, whose t_out follows t_in).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import conv_fwd_ref as R, conv_grad_ref as G
from tests.conv_grad_harness import native as _N, stream as _st
from tests.test_gpu_aux_kernels import DEV, guarded, put, ratio_of, same_bits, untouched
from tests.test_gpu_conv_grad import _geometry

pytestmark = pytest.mark.gpu
T_OUTS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
MODES = ["f32", "f32_ring", "bf16x3", "split16"]
EXACT = ("f32", "f32_ring")
# K of err <= K e_ref for the two modes that are not exact fp32 chains
BOUND = {"conv": {"bf16x3": 4.0, "split16": 8.0}, "unit": {"bf16x3": 4.0, "split16": 4.0},
         "stack": {"bf16x3": 4.0, "split16": 4.0}}
# (mode, width) pairs without a fused kernel (unit_supported / rave_stack_supported false): the only skips
UNSUPPORTED_UNITS = []
UNSUPPORTED_STACKS = []
ACTS = [G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE]
CONV_FAMILIES = [("c",) + f for f in G.FAMILIES] + [("c", 3, 1, 2)]
CONVT_FAMILIES = [("t", 2, False), ("t", 2, True), ("t", 4, False), ("t", 4, True)]
FAMILIES = CONV_FAMILIES + CONVT_FAMILIES
# channel pairs from {8, 16, 40, 64, 136}, on and off the 16 / 32 / 64 tiles; the four last
# (small) ones go with the long T so that the reference's loops stay short
PAIRS = [(16, 16), (40, 8), (8, 40), (64, 40), (40, 64), (136, 16), (16, 136), (64, 64), (40, 40), (16, 64), (8, 16),
         (64, 8)]


def _fid(fam):
    return f"k{fam[1]}s{fam[2]}d{fam[3]}" if fam[0] == "c" else f"t{fam[1]}{'cached' if fam[2] else 'offline'}"


def _taps(fam):
    return fam[1] if fam[0] == "c" else 2


# ================================================================== cases and references
@functools.lru_cache(maxsize=None)
def _case(fam, pad, act, B, c_in, c_out, T, seed=0, opts=()):
    """One conv case: the operands (fp32), the struct's fields, and (lazily) its reference.
    opts: "res" a residual, "nobias", "slope0" / "slope1", "alpha0" every Snake alpha 0."""
    rng = np.random.default_rng(seed)
    c = dict(fam=fam, act=act, B=B, c_in=c_in, c_out=c_out, opts=opts,
             slope={"slope0": 0.0, "slope1": 1.0}.get(next((o for o in opts if o.startswith("slope")), ""), 0.2))
    if fam[0] == "c":
        _, k, s, d = fam
        pl, pr, t_in = _geometry((k, s, d), pad, T)
        c.update(k=k, s=s, d=d, pl=pl, pr=pr, tr=0, P=0, t_in=t_in, t_out=T)
        wshape = (c_out, c_in, k)
    else:
        _, r, cached = fam
        pl, P, _ = R.convt_geometry(T + 1, r, cached)
        c.update(k=2 * r, s=r, d=1, pl=pl, pr=0, tr=1, P=P, t_in=T + pl, t_out=T * r)
        wshape = (c_in, c_out, 2 * r)
    x = rng.standard_normal((B, c_in, c["t_in"])).astype(np.float32)
    x[0, 0, : min(3, c["t_in"])] = 0.0                       # exact zeros beside the negatives
    x[0, c_in - 1, 0] = -0.0
    c["x"] = x
    c["w"] = (rng.standard_normal(wshape) / np.sqrt(c_in * _taps(fam))).astype(np.float32)
    c["bias"] = None if "nobias" in opts else (0.1 * rng.standard_normal(c_out)).astype(np.float32)
    c["alpha"] = rng.uniform(0.1, 3.0, c_in).astype(np.float32)
    c["alpha"][-1] = 0.0
    if "alpha0" in opts:
        c["alpha"][:] = 0.0
    c["res"] = rng.standard_normal((B, c_out, c["t_out"])).astype(np.float32) if "res" in opts else None
    return c


def _trimmed(c):
    """The case without its last t_in % 4 input columns and that much more right padding (same
    t_out), for the kernels that take whole 16-byte pieces; None where no such case exists."""
    cut = c["t_in"] % 4
    if c["tr"] or cut == 0 or c["t_in"] - cut < 1:
        return None
    if "_trim" not in c:
        c["_trim"] = dict({k: v for k, v in c.items() if not k.startswith("_")}, x=np.ascontiguousarray(c["x"][:, :, :-cut]),
                          t_in=c["t_in"] - cut, pr=c["pr"] + cut)
    return c["_trim"]


def _ref(c):
    if "_ref" not in c:
        if c["tr"]:
            c["_ref"] = R.with_e_ref(R.convt, c["x"], c["w"], c["bias"], c["alpha"], c["s"], c["pl"], c["P"], c["act"],
                                     c["slope"])
        else:
            c["_ref"] = R.with_e_ref(R.conv, c["x"], c["w"], c["bias"], c["alpha"], c["res"], c["k"], c["s"], c["d"],
                                     c["pl"], c["t_out"], c["act"], c["slope"])
    return c["_ref"]


def _judge(kind, mode, what, got, ref):
    """Print every figure, then assert the mode's bound; returns err / e_ref."""
    r64, e_ref, S = ref
    diff = np.abs(got.double().cpu().numpy() - r64)
    err, scale = float(diff.max()), float(np.abs(r64).max())
    ratio = ratio_of(err, e_ref)
    over_s = float((diff / np.maximum(S, np.finfo(np.float64).tiny)).max())
    print(f"[fwd] {kind} {mode} {what}: e_ref {e_ref:.3e} err {err:.3e} err/e_ref {ratio:.2f} err/S {over_s:.3e}")
    assert bool(torch.isfinite(got).all()), (kind, mode, what)
    if mode in EXACT:
        assert err <= 4 * e_ref, (kind, mode, what, err, e_ref)
        return ratio
    if mode == "split16":
        model = 4 * e_ref + 2.0 ** -21 * S
        assert bool((diff <= model).all()), (kind, mode, what, "beyond 4 e_ref + 2^-21 S", float((diff / model).max()))
    assert err <= min(BOUND[kind][mode] * e_ref, 2e-5 * max(1.0, scale)), (kind, mode, what, err, e_ref, scale)
    return ratio


def _pads(t, lo=4):
    """Time padding of a view of t columns: `lo` before; with lo = 4 the row length is a multiple of 4."""
    return (lo, 4 + (-t) % 4 if lo == 4 else 5)


def _dev(c, name, make):
    c.setdefault("_dev", {})
    if name not in c["_dev"]:
        c["_dev"][name] = make()
    return c["_dev"][name]


# ================================================================== the conv harness
def _conv_call(c, mode, ws=True, config=0, check=True, x_shift=0, list_configs=False, **kw):
    """One rave_conv1d call (and, when it is checked, a second one) on guarded views.  Returns
    the output, or with check = False (status, whether the y buffer is untouched), or with
    list_configs rave_conv1d_configs() of these very args, nothing launched."""
    N = _N()
    B, ci, co, prec = c["B"], c["c_in"], c["c_out"], N.PRECISION[mode]
    xb, xv, xm = _dev(c, "x", lambda: put(c["x"], [(1, 1), (1, 2), _pads(c["t_in"])]))
    packed = _dev(c, "w" + mode, lambda: torch.from_numpy(N.pack_conv_weight(
        c["w"], ci, co, c["k"], c["s"], c["d"], c["tr"], out_shift=c["P"], precision=prec)).to(DEV))
    ylo = 4 if c["t_out"] % 2 == 0 else 3                                # aligned rows and not
    yb, yv, ym = guarded((B, co, c["t_out"]), [(1, 1), (2, 1), _pads(c["t_out"], ylo)])
    a = N.ConvArgs(c_in=ci, c_out=co, kernel=c["k"], stride=c["s"], dilation=c["d"], pad_left=c["pl"], pad_right=c["pr"],
                   transposed=c["tr"], out_shift=c["P"], act=c["act"], leaky_slope=c["slope"], batch=B, t_in=c["t_in"],
                   t_out=c["t_out"], precision=prec, x=xv.data_ptr() + 4 * x_shift, x_sb=xv.stride(0), x_sc=xv.stride(1),
                   y=yv.data_ptr(), y_sb=yv.stride(0), y_sc=yv.stride(1), weight=packed.data_ptr(), config=config)
    if c["bias"] is not None:
        a.bias = _dev(c, "bias", lambda: torch.from_numpy(c["bias"]).to(DEV)).data_ptr()
    if c["act"] == G.ACT_SNAKE:
        a.alpha = _dev(c, "alpha", lambda: torch.from_numpy(c["alpha"]).to(DEV)).data_ptr()
    if c["res"] is not None:                                             # the residual at its own strides
        rb, rv, rm = _dev(c, "res", lambda: put(c["res"], [(0, 1), (1, 0), _pads(c["t_out"], 4 if ylo == 3 else 3)]))
        a.residual, a.r_sb, a.r_sc = rv.data_ptr(), rv.stride(0), rv.stride(1)
    for name, v in kw.items():
        setattr(a, name, v)
    if list_configs:
        return N.conv_configs(a)
    wsbuf = None
    if ws:
        nws = N.lib.rave_conv1d_workspace(C.byref(a))
        if check:
            assert nws >= 0, N.lib.rave_last_error().decode()
        if nws > 0:
            wsbuf = torch.full((nws + 16,), float("nan"), device=DEV)    # the slabs need no initialisation
            wsbuf[:N.SPLITK_TICKETS] = 0
            a.partial = wsbuf.data_ptr()
    before = yb.clone()
    rc = N.lib.rave_conv1d(C.byref(a), _st())
    if not check:
        torch.cuda.synchronize()
        return rc, same_bits(yb, before)
    N.check(rc, f"conv1d {mode} config {config}")
    torch.cuda.synchronize()
    first = yb.clone()
    assert bool(torch.isfinite(yv).all()), (mode, config)
    assert same_bits(first[ym], before[ym]), (mode, config, "guard words of y changed")
    assert untouched(xb, xm)
    if wsbuf is not None:
        assert int(torch.count_nonzero(wsbuf[:N.SPLITK_TICKETS].view(torch.int32))) == 0, (mode, config)
        assert bool(torch.isnan(wsbuf[nws:]).all())
    yb.copy_(before)
    N.check(N.lib.rave_conv1d(C.byref(a), _st()), "conv1d, second call")
    torch.cuda.synchronize()
    assert same_bits(yb, first), (mode, config, "the second call differs")
    if wsbuf is not None:
        assert int(torch.count_nonzero(wsbuf[:N.SPLITK_TICKETS].view(torch.int32))) == 0, (mode, config)
    return yv.clone()


RING_TEXT = "needs 16-byte aligned input rows and t_in % 4 == 0"


def _mode_case(c, mode):
    """The case a mode runs: its own, or for the 16-byte kernels at t_in % 4 != 0 (refused, asserted
    here) the trimmed one; None where there is none."""
    N = _N()
    if mode in ("f32", "split16") or c["t_in"] % 4 == 0:
        return c
    rc, clean = _conv_call(c, mode, check=False)
    assert rc == N.RAVE_ERR_UNSUPPORTED and RING_TEXT in N.lib.rave_last_error().decode() and clean, (mode, rc)
    return _trimmed(c)


def _run_modes(what, c, configs=False):
    worst = {}
    for mode in MODES:
        cm = _mode_case(c, mode)
        if cm is None:
            continue
        ref = _ref(cm)
        for ws in (True, False):
            r = _judge("conv", mode, f"{what} ws {int(ws)}", _conv_call(cm, mode, ws=ws), ref)
            worst[mode] = max(worst.get(mode, 0.0), r)
        if configs:
            cfgs = _conv_call(cm, mode, list_configs=True)
            assert cfgs, (what, mode, "no configurations listed")
            for cfg in cfgs:
                tile = (cfg - 1) & 15
                kind = "gemv" if mode == "f32" and tile >= 8 else mode
                r = _judge("conv", mode, f"{what} config {cfg} ({kind} tile {tile})", _conv_call(cm, mode, config=cfg), ref)
                worst[mode] = max(worst.get(mode, 0.0), r)
    return worst


# ================================================================== 1. the edge sweep
def _sweep():
    for f, fam in enumerate(FAMILIES):
        if fam[0] == "c":
            pads = ["centred", "causal", "none"] + (["tail"] if fam[2] > 1 else [])
        else:
            pads = ["cached" if fam[2] else "offline"]
        for i, T in enumerate(T_OUTS):
            c_in, c_out = PAIRS[(i + f) % 8] if i < 8 else PAIRS[8 + (i + f) % 4]
            opts = ("res",) if fam[0] == "c" and (i + f) % 4 == 1 else ()
            yield pytest.param(fam, pads[(i + 2 * f) % len(pads)], ACTS[(i + f) % 3], 1 + 2 * ((i + f // 3) % 2), c_in, c_out,
                               T, opts, id=f"{_fid(fam)}-T{T}")
        chunk = R.CHUNK[_taps(fam)]                       # c_in one below and one above the K-chunk
        for j, c_in in enumerate((chunk - 1, chunk + 1)):
            yield pytest.param(fam, pads[(j + f) % len(pads)], ACTS[(j + f) % 3], 1 + 2 * ((j + f) % 2), c_in, 16, 33, (),
                               id=f"{_fid(fam)}-cin{c_in}")


@pytest.mark.parametrize("fam,pad,act,B,c_in,c_out,T,opts", list(_sweep()))
def test_conv_vs_float64(fam, pad, act, B, c_in, c_out, T, opts):
    N = _N()
    assert N.conv_chunk(c_in, 2 * fam[1] if fam[0] == "t" else fam[1], fam[1] if fam[0] == "t" else fam[2],
                        1 if fam[0] == "t" else fam[3], fam[0] == "t") == R.CHUNK[_taps(fam)]
    c = _case(fam, pad, act, B, c_in, c_out, T, seed=T + c_in, opts=opts)
    _run_modes(f"{_fid(fam)} {pad} act {act} B {B} {c_in}->{c_out} T {T} {opts}", c, configs=T in (1, 33, 129))


@pytest.mark.parametrize("fam", FAMILIES, ids=_fid)
def test_every_padding_and_activation(fam):
    """The paddings and activations the rotation of the sweep leaves out at one family, at one odd shape."""
    if fam[0] == "c":
        pads = ["centred", "causal", "none"] + (["tail"] if fam[2] > 1 else [])
    else:
        pads = ["cached" if fam[2] else "offline"]
    for pad in pads:
        for act in ACTS:
            for B in (1, 3):
                _run_modes(f"{_fid(fam)} {pad} act {act} B {B}", _case(fam, pad, act, B, 40, 16, 33, seed=5))


# ================================================================== 2. the options of the struct
OPTIONS = [("nobias",), ("slope0",), ("slope1",), ("alpha0",), ("res", "nobias"), ("res", "slope1")]


@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "+".join(o))
@pytest.mark.parametrize("fam", [("c", 1, 1, 1), ("c", 3, 1, 9), ("c", 7, 1, 1), ("c", 4, 2, 1), ("c", 8, 4, 1), ("t", 2, False),
                                 ("t", 4, True)], ids=_fid)
def test_conv_options(fam, opts):
    """bias = NULL, leaky_slope 0 and 1, every Snake alpha exactly 0, the residual at its own strides
    (exact zeros and -0.0 are among the inputs of every case)."""
    if fam[0] == "t" and "res" in opts:
        opts = tuple(o for o in opts if o != "res")                      # (no residual on the transposed conv)
    act = G.ACT_SNAKE if "alpha0" in opts else G.ACT_LEAKY
    pad = ("cached" if fam[2] else "offline") if fam[0] == "t" else "centred"
    c = _case(fam, pad, act, 2, 40, 16, 33, seed=17, opts=opts)
    assert (c["x"] == 0).sum() >= 2 and np.signbit(c["x"][0, -1, 0])
    _run_modes(f"{_fid(fam)} {opts}", c)
    if "alpha0" in opts:                                                 # Snake at alpha 0 is the identity
        none = _case(fam, pad, G.ACT_NONE, 2, 40, 16, 33, seed=17, opts=())
        assert np.array_equal(_ref(c)[0], _ref(none)[0])


# ================================================================== 3. unit impulses
@pytest.mark.parametrize("fam", FAMILIES, ids=_fid)
def test_unit_impulses(fam):
    """act none, zero bias, one 1.0 per batch item at (first | last | chunk-seam channel) x (column 0 |
    last | a tile seam): the output is the fp32 weight taps, bit for bit in the three modes whose
    operands are exact (1 w is exact, and so is w's three-way bf16 split), within 2^-22 |w| (the
    documented operand representation) in split16, and zero everywhere else."""
    c_in, c_out = 40, 16
    T = 65 if fam[0] == "c" else 64 - int(fam[2])           # transposed: t_in = 64, so every mode runs it
    base = _case(fam, ("cached" if fam[2] else "offline") if fam[0] == "t" else "centred", G.ACT_NONE, 9, c_in, c_out, T,
                 seed=23)
    c = dict({k: v for k, v in base.items() if not k.startswith("_")}, bias=np.zeros(c_out, np.float32))
    x = np.zeros_like(base["x"])
    t_in = c["t_in"]
    seam = 32 * (c["s"] if not c["tr"] else 1)
    spots = [(ci, col) for ci in (0, c_in - 1, R.CHUNK[_taps(fam)]) for col in (0, t_in - 1, min(seam, t_in - 1))]
    for b, (ci, col) in enumerate(spots):
        x[b, ci, col] = 1.0
    c["x"] = x
    if c["tr"]:
        want = R.convt(x, c["w"], c["bias"], None, c["s"], c["pl"], c["P"], G.ACT_NONE, 0.2, dtype=np.float32)
    else:
        want = R.conv(x, c["w"], c["bias"], None, None, c["k"], c["s"], c["d"], c["pl"], c["t_out"], G.ACT_NONE, 0.2,
                      dtype=np.float32)
    assert want.dtype == np.float32 and np.count_nonzero(want) > 0
    assert set(np.abs(want[want != 0]).tolist()) <= set(np.abs(c["w"]).ravel().tolist())        # taps, nothing summed
    for mode in MODES:
        cm = c
        if mode in ("f32_ring", "bf16x3") and t_in % 4:
            if c["tr"]:
                continue
            cm = _trimmed(c)                       # the impulses of the last column leave with it
            want_m = R.conv(cm["x"], cm["w"], cm["bias"], None, None, cm["k"], cm["s"], cm["d"], cm["pl"], cm["t_out"],
                            G.ACT_NONE, 0.2, dtype=np.float32)
        else:
            want_m = want
        for ws in (True, False):
            got = _conv_call(cm, mode, ws=ws).cpu().numpy()
            if mode == "split16":
                assert bool((np.abs(got.astype(np.float64) - want_m) <= 2.0 ** -22 * np.abs(want_m)).all()), (mode, ws)
            else:
                assert np.array_equal(got, want_m), (mode, ws)


# ================================================================== 4. fused residual units
UNIT_WIDTHS = [64, 128, 256, 512]
# the largest dilation each launcher accepts: kUnitMaxDil (unit.hip), kUSMaxDil and kUSBf512Dil (unit_split.hip)
UNIT_MAX_DIL = {"f32": 24, "f32_ring": 16, "split16": 16, "bf16x3": 16}
COOP_RB = {64: [], 128: [], 256: [0, 2, 4], 512: [0, 4]}        # rave_unit_args.coop_rb, with a workspace


def _unit_max_dil(mode, width):
    return 4 if (mode, width) == ("bf16x3", 512) else UNIT_MAX_DIL[mode]


@functools.lru_cache(maxsize=None)
def _unit_case(width, B, T, d, pl, act, cached=0, seed=0, slope=0.2):
    """cached: 0 the one-shot form; else res_shift (x = [2 d history | block], pad_left 0)."""
    rng = np.random.default_rng(seed)
    xl = 2 * d + T if cached else T
    x = rng.standard_normal((B, width, xl)).astype(np.float32)
    x[0, 0, : min(3, xl)] = 0.0
    x[0, width - 1, 0] = -0.0
    u = _unit_operands(rng, width)
    return dict(C=width, B=B, T=T, d=d, pl=0 if cached else pl, act=act, slope=slope, x=x, xl=xl, x_len=xl if cached else 0,
                rs=cached, **u)


def _unit_operands(rng, width):
    alphas = [rng.uniform(0.1, 3.0, width).astype(np.float32) for _ in range(2)]
    alphas[0][-1] = alphas[1][0] = 0.0
    return dict(w1=(rng.standard_normal((width, width, 3)) / np.sqrt(3 * width)).astype(np.float32),
                w2=(rng.standard_normal((width, width, 1)) / np.sqrt(width)).astype(np.float32),
                b1=(0.1 * rng.standard_normal(width)).astype(np.float32), b2=(0.1 * rng.standard_normal(width)).astype(np.float32),
                a0=alphas[0], a2=alphas[1])


def _unit_ref(c):
    if "_ref" not in c:
        c["_ref"] = R.with_e_ref(R.unit, c["x"], c["w1"], c["w2"], c["b1"], c["b2"], c["a0"], c["a2"], c["d"], c["pl"], c["T"],
                                 c["act"], c["slope"], x_len=c["x_len"], res_shift=c["rs"])
    return c["_ref"]


def _unit_call(c, mode, coop=None, check=True, **kw):
    """One rave_residual_unit call (and a second) on guarded views; coop: None = no workspace, else
    coop_rb with the cooperative workspace.  The columns of x past x_len are NaN."""
    N = _N()
    W, B, T, prec = c["C"], c["B"], c["T"], N.PRECISION[mode]
    xb, xv, xm = _dev(c, "x", lambda: put(c["x"], [(1, 1), (1, 2), _pads(c["xl"])]))
    packed = _dev(c, "w" + mode, lambda: torch.from_numpy(N.pack_unit_weight(c["w1"], c["w2"], W, precision=prec)).to(DEV))
    small = _dev(c, "small", lambda: {k: torch.from_numpy(c[k]).to(DEV) for k in ("b1", "b2", "a0", "a2")})
    yb, yv, ym = guarded((B, W, T), [(1, 1), (2, 1), _pads(T, 4 if T % 2 == 0 else 3)])
    snake = c["act"] == G.ACT_SNAKE
    a = N.UnitArgs(channels=W, batch=B, t_len=T, dilation=c["d"], pad_left=c["pl"], act=c["act"], leaky_slope=c["slope"],
                   precision=prec, x=xv.data_ptr(), x_sb=xv.stride(0), x_sc=xv.stride(1), y=yv.data_ptr(), y_sb=yv.stride(0),
                   y_sc=yv.stride(1), weight=packed.data_ptr(), bias1=small["b1"].data_ptr(), bias2=small["b2"].data_ptr(),
                   alpha0=small["a0"].data_ptr() if snake else None, alpha2=small["a2"].data_ptr() if snake else None,
                   x_len=c["x_len"], res_shift=c["rs"], coop_rb=coop or 0)
    for name, v in kw.items():
        setattr(a, name, v)
    wsbuf = None
    if coop is not None and check:
        nws = N.lib.rave_unit_workspace(C.byref(a))
        assert nws > N.SPLITK_TICKETS, (mode, W, coop, nws)
        wsbuf = torch.zeros(nws + 16, device=DEV)
        wsbuf[nws:] = float("nan")
        a.workspace = wsbuf.data_ptr()
    before = yb.clone()
    rc = N.lib.rave_residual_unit(C.byref(a), _st())
    if not check:
        torch.cuda.synchronize()
        return rc, same_bits(yb, before)
    N.check(rc, f"residual_unit {mode} coop {coop}")
    torch.cuda.synchronize()
    first = yb.clone()
    assert bool(torch.isfinite(yv).all()), (mode, coop)
    assert same_bits(first[ym], before[ym]), (mode, coop, "guard words of y changed")
    assert untouched(xb, xm)
    if wsbuf is not None:
        assert int(torch.count_nonzero(wsbuf[:N.SPLITK_TICKETS].view(torch.int32))) == 0, (mode, coop)
        assert bool(torch.isnan(wsbuf[nws:]).all())
    yb.copy_(before)
    N.check(N.lib.rave_residual_unit(C.byref(a), _st()), "residual_unit, second call")
    torch.cuda.synchronize()
    assert same_bits(yb, first), (mode, coop, "the second call differs")
    if wsbuf is not None:
        assert int(torch.count_nonzero(wsbuf[:N.SPLITK_TICKETS].view(torch.int32))) == 0, (mode, coop)
    return yv.clone()


def _run_unit_modes(what, c):
    N = _N()
    for mode in MODES:
        if (mode, c["C"]) in UNSUPPORTED_UNITS:
            continue
        assert N.unit_supported(c["C"], N.PRECISION[mode]), (mode, c["C"])
        if c["d"] > _unit_max_dil(mode, c["C"]):                         # refused, not skipped
            rc, clean = _unit_call(c, mode, check=False)
            assert rc == N.RAVE_ERR_UNSUPPORTED and clean, (mode, rc)
            assert ("C = 512 supports dilations <= 4" if mode == "bf16x3" and c["C"] == 512 else "dilation too large") in \
                N.lib.rave_last_error().decode()
            continue
        for coop in [None] + (COOP_RB[c["C"]] if mode != "f32" else []):
            _judge("unit", mode, f"{what} coop {coop}", _unit_call(c, mode, coop=coop), _unit_ref(c))


def _unit_sweep():
    dils = [1, 2, 3, 9]
    for w, width in enumerate(UNIT_WIDTHS):
        for i, T in enumerate(t for t in T_OUTS if width < 256 or t <= 129):
            d = dils[(i + w) % 4]
            pl = [0, 1, d, d + 1, 2 * d][(i + 2 * w) % 5]
            B = (1 + 2 * ((i + w) % 2)) if width < 256 else 1 + (i + w) % 2
            yield pytest.param(width, B, T, d, pl, [G.ACT_LEAKY, G.ACT_SNAKE][(i + w // 2) % 2], id=f"C{width}-T{T}")


@pytest.mark.parametrize("width,B,T,d,pl,act", list(_unit_sweep()))
def test_unit_vs_float64(width, B, T, d, pl, act):
    _run_unit_modes(f"C {width} B {B} T {T} d {d} pl {pl} act {act}", _unit_case(width, B, T, d, pl, act, seed=T + width))


@pytest.mark.parametrize("width", UNIT_WIDTHS)
def test_unit_every_pad_left_and_dilation(width):
    """pad_left in {0, 1, d, d + 1, 2 d} at each of the dilations 1, 2, 3, 9, at one odd length."""
    for i, d in enumerate((1, 2, 3, 9)):
        for pl in sorted({0, 1, d, d + 1, 2 * d}):
            act = [G.ACT_LEAKY, G.ACT_SNAKE][(i + pl) % 2]
            _run_unit_modes(f"C {width} d {d} pl {pl} act {act}", _unit_case(width, 2 if width < 256 else 1, 33, d, pl, act, seed=d))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", UNIT_WIDTHS)
def test_unit_largest_dilation(width, mode):
    """The largest dilation the mode's launcher accepts, centred and causal; one more is refused
    (test_refusals)."""
    d = _unit_max_dil(mode, width)
    for pl, act in ((d, G.ACT_LEAKY), (2 * d, G.ACT_SNAKE)):
        c = _unit_case(width, 1, 65, d, pl, act, seed=d)
        for coop in [None] + (COOP_RB[width] if mode != "f32" else []):
            _judge("unit", mode, f"C {width} d {d} pl {pl} coop {coop}", _unit_call(c, mode, coop=coop), _unit_ref(c))


@pytest.mark.parametrize("width", UNIT_WIDTHS)
def test_unit_cached_form(width):
    """pad_left 0, x_len = 2 d + t_len, the residual at res_shift 2 d (and d, the centred delay);
    every column of x past x_len is NaN."""
    for T, d, rs, act in ((1, 1, 2, G.ACT_LEAKY), (33, 3, 6, G.ACT_SNAKE), (64, 9, 9, G.ACT_LEAKY), (126, 1, 2, G.ACT_SNAKE)):
        _run_unit_modes(f"cached C {width} T {T} d {d} res_shift {rs}", _unit_case(width, 2, T, d, 0, act, cached=rs, seed=T))


def test_unit_leaky_slopes():
    for slope in (0.0, 1.0):
        _run_unit_modes(f"C 64 slope {slope}", _unit_case(64, 2, 33, 3, 3, G.ACT_LEAKY, seed=3, slope=slope))


# ================================================================== 5. residual stacks
STACK_T = [1, 31, 32, 33, 64, 65, 129]
STACK_MODES = ["split16", "bf16x3"]
# the largest dilations the bf16x3 form's 24-column halo and the 32-column margin allow:
# centred pad = d <= 16 with d2 + d3 <= 32; causal pad = 2 d <= 24 with 2 (d2 + d3) <= 32
STACK_DILS = {"centred": [(1, 3, 9), (16, 16, 16)], "causal": [(1, 3, 9), (12, 8, 8)]}


@functools.lru_cache(maxsize=None)
def _stack_case(width, B, T, dils, causal, act, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, width, T)).astype(np.float32)
    x[0, 0, : min(3, T)] = 0.0
    units = [dict(_unit_operands(rng, width), d=d, pl=2 * d if causal else d) for d in dils]
    return dict(C=width, B=B, T=T, act=act, x=x, units=units)


def _stack_ref(c):
    if "_ref" not in c:
        units = [(u["w1"], u["w2"], u["b1"], u["b2"], u["a0"], u["a2"], u["d"], u["pl"]) for u in c["units"]]
        c["_ref"] = R.with_e_ref(R.stack, c["x"], units, c["act"], 0.2)
    return c["_ref"]


def _stack_call(c, mode, check=True, **kw):
    N = _N()
    W, B, T, prec = c["C"], c["B"], c["T"], N.PRECISION[mode]
    xb, xv, xm = _dev(c, "x", lambda: put(c["x"], [(1, 1), (1, 2), _pads(T)]))
    yb, yv, ym = guarded((B, W, T), [(1, 1), (2, 1), _pads(T, 4 if T % 2 == 0 else 3)])
    a = N.StackArgs(channels=W, batch=B, t_len=T, act=c["act"], leaky_slope=0.2, precision=prec, x=xv.data_ptr(),
                    x_sb=xv.stride(0), x_sc=xv.stride(1), y=yv.data_ptr(), y_sb=yv.stride(0), y_sc=yv.stride(1))
    for i, u in enumerate(c["units"]):
        dev = _dev(c, f"u{i}{mode}", lambda: [torch.from_numpy(N.pack_unit_weight(u["w1"], u["w2"], W, precision=prec)).to(DEV)]
                   + [torch.from_numpy(u[k]).to(DEV) for k in ("b1", "b2", "a0", "a2")])
        setattr(a, f"dilation{i}", u["d"])
        setattr(a, f"pad_left{i}", u["pl"])
        for f, t in zip(("weight", "bias1", "bias2", "alpha0", "alpha2"), dev):
            setattr(a, f"{f}{i}", t.data_ptr())
    for name, v in kw.items():
        setattr(a, name, v)
    before = yb.clone()
    rc = N.lib.rave_residual_stack(C.byref(a), _st())
    if not check:
        torch.cuda.synchronize()
        return rc, same_bits(yb, before)
    N.check(rc, f"residual_stack {mode}")
    torch.cuda.synchronize()
    first = yb.clone()
    assert bool(torch.isfinite(yv).all()), mode
    assert same_bits(first[ym], before[ym]), (mode, "guard words of y changed")
    assert untouched(xb, xm)
    yb.copy_(before)
    N.check(N.lib.rave_residual_stack(C.byref(a), _st()), "residual_stack, second call")
    torch.cuda.synchronize()
    assert same_bits(yb, first), (mode, "the second call differs")
    return yv.clone()


def _stack_sweep():
    for w, width in enumerate((64, 128)):
        for i, T in enumerate(STACK_T):
            pad = ["centred", "causal"][(i + w) % 2]
            yield pytest.param(width, 1 + 2 * ((i + w + 1) % 2), T, pad, [G.ACT_LEAKY, G.ACT_SNAKE][(i // 2 + w) % 2],
                               id=f"C{width}-T{T}")


@pytest.mark.parametrize("width,B,T,pad,act", list(_stack_sweep()))
def test_stack_vs_float64(width, B, T, pad, act):
    N = _N()
    assert N.stack_supported(width)
    for dils in STACK_DILS[pad]:
        c = _stack_case(width, B, T, dils, pad == "causal", act, seed=T + width)
        for mode in STACK_MODES:
            if (mode, width) in UNSUPPORTED_STACKS:
                continue
            _judge("stack", mode, f"C {width} B {B} T {T} {pad} {dils} act {act}", _stack_call(c, mode), _stack_ref(c))


@pytest.mark.parametrize("width", [64, 128])
def test_stack_both_paddings_at_one_length(width):
    for pad in ("centred", "causal"):
        for act in (G.ACT_LEAKY, G.ACT_SNAKE):
            c = _stack_case(width, 2, 33, (1, 3, 9), pad == "causal", act, seed=29)
            for mode in STACK_MODES:
                _judge("stack", mode, f"C {width} {pad} act {act}", _stack_call(c, mode), _stack_ref(c))


# ================================================================== 6. refusals
def _refuse_conv(mode, fam=("c", 3, 1, 1), T=32, **kw):
    return lambda: _conv_call(_case(fam, "centred", G.ACT_LEAKY, 1, 16, 16, T, seed=1), mode, check=False, **kw)


def _refuse_unit(mode, width, d, **kw):
    if width not in UNIT_WIDTHS:                               # no packer for it: any image will do
        def call():
            c = _unit_case(64, 1, 32, d, d, G.ACT_LEAKY, seed=1)
            return _unit_call(c, mode, check=False, channels=width)
        return call
    return lambda: _unit_call(_unit_case(width, 1, 32, d, d, G.ACT_LEAKY, seed=1), mode, check=False, **kw)


def _refuse_stack(mode, width, dils, causal, **kw):
    return lambda: _stack_call(_stack_case(width if width in (64, 128) else 64, 1, 32, dils, causal, G.ACT_LEAKY, seed=1), mode,
                               check=False, **kw)


ERR_ARG, ERR_UNSUPPORTED = -1, -3
REFUSALS = [
    # one dilation past the staged window
    ("conv f32 d17", _refuse_conv("f32", dilation=17, pad_left=17, pad_right=17), ERR_ARG, "conv1d: dilation out of range"),
    ("conv split16 d17", _refuse_conv("split16", dilation=17, pad_left=17, pad_right=17), ERR_ARG,
     "conv1d: dilation out of range"),
    ("unit f32 d25", _refuse_unit("f32", 64, 25), ERR_ARG, "residual_unit: dilation out of range"),
    ("unit split16 d17", _refuse_unit("split16", 128, 17), ERR_UNSUPPORTED, "residual_unit(split16): dilation too large"),
    ("unit f32_ring d17", _refuse_unit("f32_ring", 64, 17), ERR_UNSUPPORTED, "residual_unit(split16): dilation too large"),
    ("unit bf16x3 d17", _refuse_unit("bf16x3", 256, 17), ERR_UNSUPPORTED, "residual_unit(split16): dilation too large"),
    ("unit bf16x3 C512 d5", _refuse_unit("bf16x3", 512, 5), ERR_UNSUPPORTED,
     "residual_unit(bf16x3): C = 512 supports dilations <= 4"),
    # a stack reaching past its margin or halo
    ("stack split16 margin", _refuse_stack("split16", 64, (1, 9, 9), True), ERR_UNSUPPORTED,
     "residual_stack: units 2..3 reach past the 32-column margin"),
    ("stack bf16x3 margin", _refuse_stack("bf16x3", 128, (1, 16, 16), False, pad_left1=17), ERR_UNSUPPORTED,
     "residual_stack: units 2..3 reach past the 32-column margin"),
    ("stack bf16x3 halo", _refuse_stack("bf16x3", 64, (1, 3, 13), True), ERR_UNSUPPORTED,
     "residual_stack(bf16x3): a unit's taps reach past the 24-row plane halo"),
    # an unsupported width
    ("unit f32 C96", _refuse_unit("f32", 96, 1), ERR_UNSUPPORTED,
     "residual_unit: fused residual unit supports C in {64, 128, 256, 512}"),
    ("unit split16 C32", _refuse_unit("split16", 32, 1), ERR_UNSUPPORTED,
     "residual_unit: fused residual unit supports C in {64, 128, 256, 512}"),
    ("stack C256", _refuse_stack("split16", 256, (1, 3, 9), False, channels=256), ERR_UNSUPPORTED, "residual_stack: C in {64, 128}"),
    # coop_rb out of range
    ("unit C256 coop_rb 3", _refuse_unit("split16", 256, 1, coop_rb=3), ERR_ARG, "residual_unit: coop_rb must be 0"),
    ("unit C512 coop_rb 2", _refuse_unit("bf16x3", 512, 1, coop_rb=2), ERR_ARG, "residual_unit: coop_rb must be 0"),
    ("unit C64 coop_rb 2", _refuse_unit("f32_ring", 64, 1, coop_rb=2), ERR_ARG, "residual_unit: coop_rb must be 0"),
    # an unaligned ring row: the start one float off, t_in % 4 != 0, a channel stride off
    ("conv f32_ring start", _refuse_conv("f32_ring", x_shift=1), ERR_UNSUPPORTED, "conv1d(f32_ring): " + RING_TEXT),
    ("conv bf16x3 start", _refuse_conv("bf16x3", x_shift=1), ERR_UNSUPPORTED, "conv1d(bf16x3): " + RING_TEXT),
    ("conv f32_ring t_in", _refuse_conv("f32_ring", T=33), ERR_UNSUPPORTED, "conv1d(f32_ring): " + RING_TEXT),
    ("conv bf16x3 t_in", _refuse_conv("bf16x3", fam=("c", 4, 2, 1), T=33), ERR_UNSUPPORTED, "conv1d(bf16x3): " + RING_TEXT),
    ("conv bf16x3 stride", _refuse_conv("bf16x3", x_sc=41), ERR_UNSUPPORTED, "conv1d(bf16x3): " + RING_TEXT),
]


@pytest.mark.parametrize("name,call,status,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, call, status, text):
    """The launcher refuses the shape with its status code and its text, and leaves y as it was."""
    N = _N()
    assert (ERR_ARG, ERR_UNSUPPORTED) == (N.RAVE_ERR_ARG, N.RAVE_ERR_UNSUPPORTED)
    rc, clean = call()
    last = N.lib.rave_last_error().decode()
    assert rc == status and text in last and clean, (name, rc, last, clean)


def test_static_skip_lists_are_the_library_s():
    N = _N()
    assert [(m, w) for m in MODES for w in UNIT_WIDTHS if not N.unit_supported(w, N.PRECISION[m])] == UNSUPPORTED_UNITS
    assert [(m, w) for m in STACK_MODES for w in (64, 128) if not N.stack_supported(w)] == UNSUPPORTED_STACKS
