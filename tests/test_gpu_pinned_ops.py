"""The single ops that the pinned C3 plans run, in the form the streaming
engine runs them, and the agreement of rave_conv1d_workspace with rave_conv1d.

tests/test_gpu_configs_pinned.py says "the pinned plan is wrong"; these say
which op.  Every ``conv|...`` and ``unit|...`` entry of
``profiles/tuning/c3_{f32_bf3,auto}.json`` is decoded (rave_amd/csrc/engine.cpp:
key_of, Model::conv_launch: value = precision * 65536 + config, key
``conv|node|stream form|B|t_in[|noring]``; Model::unit_pick: value = precision |
coop << 8, key ``unit|k3 node|B|T``), its node looked up in the causal graph,
and that one op run through rave_conv1d / rave_residual_unit with the pinned
precision and config on the operand view the streaming engine gives it
(conv_stream / stream_convs in engine.cpp): x starts ``need`` columns before the
block inside a [history | block] row -- an odd width and offset for ``noring``
keys, 16-byte rows otherwise, since those are the rows the choice was made for
-- the cached ConvTranspose with its one history column, the cached unit with
x_len = 2d + T and res_shift.  A conv entry whose t_in is the bare block length
of a dilated unit's k3 conv is the one-shot form that Model::fuse_unit times.

Reference: the float64 oracle on the same window (oracle.rave_oracle conv1d,
conv_transpose1d, leaky_relu).  Tolerance: the layer tolerance, 2e-5 x
max(1, max|ref|).  bf16x3 entries also pass the fp32-class check of
test_conv_bf16x3_is_fp32_class / test_residual_unit_bf16x3_is_fp32_class
against the fp32 ring kernel on the same operands."""
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_parity import (GEMV_CASES, _stream_conv_cases, conv_case, maxabs,  # noqa: E402
                                   run_cached_unit)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ["f32_bf3", "auto"]
Y_PAD = 5                       # output columns past t_out: NaN before, NaN after


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def N():
    from rave_amd import _native
    return _native


def _entries(precision, kind):
    with open(os.path.join(REPO, "profiles", "tuning", f"c3_{precision}.json")) as fh:
        return [(k, int(v)) for k, v, _ in json.load(fh) if k.startswith(kind + "|")]


def _c3_nodes():
    from rave_amd import config as rcfg
    cases = _stream_conv_cases(rcfg.causal())
    return {n.name: (n, ts) for n, ts in cases}, [n for n, _ in cases]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _conv_entry(N, dev, key, n, ts, t_in, noring, prec, config, rng):
    """One conv entry on its streaming view; returns (output, float64 reference)."""
    from oracle.rave_oracle import conv1d, conv_transpose1d, leaky_relu
    B = int(key.split("|")[3])
    need = 1 if n.transposed else n.pad[0]           # causal: r = 0, no stride delay
    oneshot = not n.transposed and need > 0 and t_in == ts
    assert oneshot or t_in == need + ts, f"{key}: t_in is neither the block's {ts} nor need + block = {need + ts}"
    t_out = ts * n.stride if n.transposed else ts // n.stride
    if oneshot:                                      # dense rows, zero padding (Model::fuse_unit's timing form)
        off, width = 0, t_in
    elif noring:                                     # odd history offset, odd row width
        off = 3
        width = off + t_in + 3
        width += 1 if width % 4 == 0 else 0
    else:                                            # rows the 16-byte kernels take
        off = 4
        width = (off + t_in + 3) // 4 * 4 + 4
    xw = np.full((B, n.c_in, width), np.nan, np.float32)     # past x_len: NaN, must not reach the output
    xw[:, :, :off + t_in] = rng.standard_normal((B, n.c_in, off + t_in))
    wshape = (n.c_in, n.c_out, n.kernel) if n.transposed else (n.c_out, n.c_in, n.kernel)
    w = (rng.uniform(-1, 1, wshape) / np.sqrt(n.c_in * n.kernel)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, n.c_out).astype(np.float32) if n.bias else None
    has_res = n.residual is not None
    r_sc = t_out + 3
    res = rng.standard_normal((B, n.c_out, r_sc)).astype(np.float32) if has_res else None
    assert n.act in ("none", "leaky"), key
    xa = xw[:, :, off:off + t_in].astype(np.float64)
    xa = leaky_relu(xa, 0.2) if n.act == "leaky" else xa
    if n.transposed:      # cached form: y[u s + q] = W[q + s] x[u - 1] + W[q] x[u], x[-1] the history column
        ref = conv_transpose1d(xa, w, n.stride, n.stride, bias)
    else:
        ref = conv1d(xa, w, bias, n.stride, n.dilation, n.pad if oneshot else (0, 0))
    if has_res:
        ref = ref + res[:, :, :t_out]
    assert ref.shape[-1] == t_out, (key, ref.shape, t_out)

    xd = torch.from_numpy(xw).to(dev)
    bd = torch.from_numpy(bias).to(dev) if bias is not None else None
    rd = torch.from_numpy(res).to(dev) if has_res else None
    y_sc = t_out + Y_PAD
    outs = {}
    # a bf16x3 entry is also run on the fp32 ring kernel, same operands (the fp32-class check)
    for p in [prec] + ([N.PREC_F32_RING] if prec == N.PREC_BF16X3 else []):
        packed = torch.from_numpy(N.pack_conv_weight(w, n.c_in, n.c_out, n.kernel, n.stride, n.dilation,
                                                     n.transposed, out_shift=0, precision=p)).to(dev)
        y = torch.full((B, n.c_out, y_sc), float("nan"), device=dev)
        a = N.ConvArgs(c_in=n.c_in, c_out=n.c_out, kernel=n.kernel, stride=n.stride, dilation=n.dilation,
                       pad_left=1 if n.transposed else n.pad[0] if oneshot else 0,
                       pad_right=n.pad[1] if oneshot else 0, transposed=int(n.transposed), out_shift=0,
                       act=N.ACT[n.act], leaky_slope=0.2, batch=B, t_in=t_in, t_out=t_out, precision=p,
                       x=xd.data_ptr() + 4 * off, x_sb=n.c_in * width, x_sc=width,
                       y=y.data_ptr(), y_sb=n.c_out * y_sc, y_sc=y_sc,
                       residual=rd.data_ptr() if has_res else None, r_sb=n.c_out * r_sc if has_res else 0,
                       r_sc=r_sc if has_res else 0, weight=packed.data_ptr(),
                       bias=bd.data_ptr() if bd is not None else None, config=config if p == prec else 0)
        nws = int(N.lib.rave_conv1d_workspace(C.byref(a)))
        assert nws >= 0, f"{key}: workspace query refuses precision {p} config {a.config}: " \
                         f"{N.lib.rave_last_error().decode()}"
        ws = None
        if nws > 0:
            ws = torch.full((nws,), float("nan"), device=dev)
            ws[:N.SPLITK_TICKETS] = 0
            a.partial = ws.data_ptr()
        first = None
        for _ in range(2):
            y.fill_(float("nan"))
            rc = N.lib.rave_conv1d(C.byref(a), _stream())
            assert rc == 0, f"{key}: launch refuses precision {p} config {a.config} (status {rc}): " \
                            f"{N.lib.rave_last_error().decode()}"
            torch.cuda.synchronize()
            out = y.cpu().numpy()
            assert np.isnan(out[..., t_out:]).all(), f"{key}: wrote past t_out"
            assert np.isfinite(out[..., :t_out]).all(), f"{key}: NaN or inf in the output"
            if ws is not None:
                assert int((ws[:N.SPLITK_TICKETS].view(torch.int32) != 0).sum()) == 0, f"{key}: counters not zero"
            assert first is None or np.array_equal(out, first, equal_nan=True), f"{key}: second call differs"
            first = out
        outs[p] = first[..., :t_out]
    return outs, ref


@pytest.mark.parametrize("precision", PRECISIONS)
def test_c3_pinned_conv_entries_vs_oracle(N, dev, precision):
    """Every conv entry of the pinned C3 file, on the streaming operand view."""
    nodes, _ = _c3_nodes()
    rng = np.random.default_rng(3)
    worst, n_bf3, tiles = 0.0, 0, set()
    for key, val in _entries(precision, "conv"):
        p = key.split("|")
        assert p[1] in nodes, f"{key}: no such node in the causal graph"
        n, ts = nodes[p[1]]
        prec, config = val // 65536, val % 65536
        assert int(p[2]) == int(n.transposed), f"{key}: stream form {p[2]} on a {'' if n.transposed else 'non-'}transposed conv"
        outs, ref = _conv_entry(N, dev, key, n, ts, int(p[4]), len(p) == 6, prec, config, rng)
        scale = max(1.0, float(np.abs(ref).max()))
        err = maxabs(outs[prec], ref)
        worst = max(worst, err / scale)
        assert err <= 2e-5 * scale, f"{key} (precision {prec}, config {config}): max-abs {err:.3e}, scale {scale:.3e}"
        if prec == N.PREC_F32 and config:
            tiles.add((config - 1) & 15)
        if prec == N.PREC_BF16X3:
            n_bf3 += 1
            s = float(np.abs(ref).max())
            e_ring, e_bf3 = maxabs(outs[N.PREC_F32_RING], ref) / s, err / s
            d_rb = maxabs(outs[prec], outs[N.PREC_F32_RING]) / s
            assert e_bf3 <= 1.5 * e_ring + 1e-7, f"{key}: bf16x3 rel err {e_bf3:.2e}, fp32 ring {e_ring:.2e}"
            assert d_rb <= 1e-6, f"{key}: bf16x3 vs fp32 ring {d_rb:.2e} of the output scale"
    print(f"\n[parity] C3 pinned conv entries ({precision}): worst err / (2e-5 x scale) = {worst / 2e-5:.3f}; "
          f"{n_bf3} bf16x3 entries; exact-fp32 tiles pinned {sorted(tiles)}")
    # the forms this file exists for are among the entries: the row-sliced skinny-N tiles
    assert {14, 15} <= tiles, tiles
    assert (precision != "f32_bf3") or n_bf3 >= 20, n_bf3


@pytest.mark.parametrize("precision", PRECISIONS)
def test_c3_pinned_unit_entries_vs_oracle(N, dev, precision):
    """Every fused-unit entry of the pinned C3 file in its cached form (B = 1,
    x_len = 2d + T, res_shift = 2d, the pinned arithmetic and cooperative form)."""
    nodes, _ = _c3_nodes()
    worst, n_bf3 = 0.0, 0
    for key, val in _entries(precision, "unit"):
        p = key.split("|")
        assert p[1] in nodes, f"{key}: no such node in the causal graph"
        n, ts = nodes[p[1]]
        prec, coop = val & 255, val >> 8
        B, T = int(p[2]), int(p[3])
        assert T == ts and n.kernel == 3 and n.pad == (2 * n.dilation, 0), key
        assert N.unit_supported(n.c_in, prec), f"{key}: no fused unit of precision {prec} at C = {n.c_in}"
        case = (n.c_in, n.dilation, n.act, True, B, T, {0: False, 1: True, 2: 4}[coop])
        try:
            got, ref, ws = run_cached_unit(N, dev, case, prec, y_pad=Y_PAD, calls=2)
        except (N.NativeError, NotImplementedError, ValueError) as e:
            raise AssertionError(f"{key}: precision {prec} coop {coop} refused at launch: {e}")
        assert (ws is not None) == bool(coop), f"{key}: cooperative form {coop} but workspace {ws is not None}"
        assert np.isnan(got[..., T:]).all(), f"{key}: wrote past t_len"
        assert np.isfinite(got[..., :T]).all(), f"{key}: NaN or inf in the output"
        if ws is not None:
            assert int(torch.count_nonzero(ws[:N.SPLITK_TICKETS])) == 0, f"{key}: counters not zero"
        scale = max(1.0, float(np.abs(ref).max()))
        err = maxabs(got[..., :T], ref)
        worst = max(worst, err / scale)
        assert err <= 2e-5 * scale, f"{key} (precision {prec}, coop {coop}): max-abs {err:.3e}, scale {scale:.3e}"
        if prec == N.PREC_BF16X3:
            n_bf3 += 1
            ring, _, _ = run_cached_unit(N, dev, case[:6] + (False,), N.PREC_F32_RING)
            s = float(np.abs(ref).max())
            e_ring, e_bf3 = maxabs(ring, ref) / s, err / s
            d_rb = maxabs(got[..., :T], ring) / s
            assert e_bf3 <= 1.5 * e_ring + 1e-7, f"{key}: bf16x3 rel err {e_bf3:.2e}, fp32 ring {e_ring:.2e}"
            assert d_rb <= 1e-6, f"{key}: bf16x3 vs fp32 ring {d_rb:.2e} of the output scale"
    print(f"\n[parity] C3 pinned unit entries ({precision}): worst err / (2e-5 x scale) = {worst / 2e-5:.3f}; "
          f"{n_bf3} bf16x3 entries")
    assert (precision != "f32_bf3") or n_bf3 == 22, n_bf3


# ------------------------------------------------------------------ workspace query == launcher
# ConvT shapes of GEMV_CASES in the torch form (out_shift = stride / 2: two phase
# groups, group 1 starting at a 64-row boundary), one of them in the cached form
# too (out_shift 0: one group), and a plain conv as the control
REFUSAL_CASES = [(GEMV_CASES[4], None), (GEMV_CASES[5], None), (GEMV_CASES[13], None), (GEMV_CASES[5], 0),
                 (GEMV_CASES[0], None)]


@pytest.mark.parametrize("case,out_shift", REFUSAL_CASES, ids=[f"{c[:8]}-shift{s}" for c, s in REFUSAL_CASES])
def test_conv_rows_workspace_and_launcher_refuse_alike(N, dev, case, out_shift):
    """For every config word of the row-sliced tiles 14 and 15 -- each K-split
    count the word can carry, with and without bit 9, and words past the 10 bits,
    most of which rave_conv1d_configs never lists -- rave_conv1d_workspace answers
    >= 0 exactly when rave_conv1d succeeds; a refusal is an error return before
    anything is launched (the NaN-prefilled output stays NaN); and every
    configuration rave_conv1d_configs lists is accepted by both."""
    c_in, c_out, k, s, d, transposed, act, has_res, B, T = case
    assert c_in and not has_res
    x, w, b, alpha, res, pad, ref = conv_case(case)
    if out_shift is None:
        out_shift = s // 2 if transposed else 0
    else:       # the cached ConvTranspose form: one history column, no crop (length only; not compared)
        assert transposed and out_shift == 0
        T = T - 1
    t_out = T * s if transposed else ref.shape[-1]
    packed = torch.from_numpy(N.pack_conv_weight(w, c_in, c_out, k, s, d, transposed, out_shift=out_shift,
                                                 precision=N.PREC_F32)).to(dev)
    xd = torch.from_numpy(x).to(dev)
    bd = torch.from_numpy(b).to(dev)
    ad = torch.from_numpy(alpha).to(dev) if alpha is not None else None
    y = torch.full((B, c_out, t_out), float("nan"), device=dev)
    ws = torch.zeros(N.SPLITK_TICKETS + 64, device=dev)        # grown to what a configuration asks for
    t_in = x.shape[-1]

    def args(config):
        return N.ConvArgs(c_in=c_in, c_out=c_out, kernel=k, stride=s, dilation=d,
                          pad_left=(1 if out_shift == 0 else 0) if transposed else pad[0],
                          pad_right=0 if transposed else pad[1], transposed=transposed, out_shift=out_shift,
                          act=N.ACT[act], leaky_slope=0.2, batch=B, t_in=t_in, t_out=t_out, precision=N.PREC_F32,
                          x=xd.data_ptr(), x_sb=c_in * t_in, x_sc=t_in, y=y.data_ptr(), y_sb=c_out * t_out,
                          y_sc=t_out, weight=packed.data_ptr(), bias=bd.data_ptr(),
                          alpha=ad.data_ptr() if ad is not None else None, partial=ws.data_ptr(), config=config)
    listed = set(N.conv_configs(args(0)))
    words = [1 + tile + 16 * (S - 1) + 512 * sep + 1024 * hi
             for tile in (14, 15) for sep in (0, 1) for S in range(1, 33) for hi in (0, 1) if hi == 0 or S <= 2]
    assert {w_ for w_ in listed if (w_ - 1) & 15 >= 14} <= set(words)
    accepted, unlisted = [], 0
    for cfg in sorted(set(words) | listed):
        a = args(cfg)
        nws = int(N.lib.rave_conv1d_workspace(C.byref(a)))
        if nws > ws.numel():                         # a listed K-split configuration with larger slabs
            assert int(torch.count_nonzero(ws[:N.SPLITK_TICKETS])) == 0
            ws = torch.zeros(nws, device=dev)
            a.partial = ws.data_ptr()
        y.fill_(float("nan"))
        rc = N.lib.rave_conv1d(C.byref(a), _stream())
        torch.cuda.synchronize()
        assert (nws >= 0) == (rc == 0), f"config {cfg}: workspace query says {nws}, launch returns {rc} " \
                                        f"({N.lib.rave_last_error().decode()})"
        if rc != 0:
            assert rc in (N.RAVE_ERR_ARG, N.RAVE_ERR_UNSUPPORTED), (cfg, rc)
            assert torch.isnan(y).all(), f"config {cfg}: refused, yet the output was written"
            assert cfg not in listed, f"config {cfg}: listed by rave_conv1d_configs, refused at launch"
        else:
            assert torch.isfinite(y).all(), f"config {cfg}: accepted, output not finite"
            if cfg in words:
                accepted.append(cfg)
                unlisted += cfg not in listed
            if out_shift == (s // 2 if transposed else 0):       # the form conv_case's reference is for
                err = maxabs(y.cpu().numpy(), ref)
                assert err <= 2e-5 * max(1.0, np.abs(ref).max()), (cfg, err)
    assert int(torch.count_nonzero(ws[:N.SPLITK_TICKETS])) == 0
    print(f"\n[refusal] {case[:8]} out_shift {out_shift}: {len(words)} row-sliced config words tried, "
          f"{len(accepted)} accepted by both entry points ({sorted(accepted)}), {unlisted} of them unlisted")
    # the row-sliced form exists at these shapes (U <= 32): 8, 16 and 32 rows per workgroup
    assert {15, 16, 527} <= set(accepted), accepted
