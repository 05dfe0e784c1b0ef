"""tests/conv_fwd_ref.py against float64 torch and the oracle's conv1d /
conv_transpose1d / leaky_relu / snake (no GPU): every layer family, every padding
kind, both transposed forms, the unit at every pad_left and in its cached form, the
stack; and that the float32 run is a float32 chain, not a rounded float64 result."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rave_oracle as O
from tests import conv_fwd_ref as R, conv_grad_ref as G
from tests.test_conv_grad_ref_host import _geometry, _torch_act

FAMILIES = G.FAMILIES + [(3, 1, 2)]
ACTS = (G.ACT_NONE, G.ACT_LEAKY, G.ACT_SNAKE)
CONV_CASES = [(fam, pad, act) for fam in FAMILIES for pad in ("centred", "causal", "none", "tail") for act in ACTS
              if not (pad == "tail" and fam[1] == 1)]
TOL = 1e-11


def _oracle_act(x, act, slope, alpha):
    return O.leaky_relu(x, slope) if act == G.ACT_LEAKY else O.snake(x, alpha) if act == G.ACT_SNAKE else x


def _alpha(rng, c):
    alpha = rng.uniform(0.1, 3.0, c)
    alpha[-1] = 0.0
    return alpha


@pytest.mark.parametrize("fam,pad,act", CONV_CASES)
def test_conv_matches_torch_and_oracle(fam, pad, act):
    k, s, d = fam
    t_out, c_in, c_out = 9, 2 * R.CHUNK[k] + 1, 6                   # three K-chunks, the last of one channel
    pl, pr, t_in = _geometry(fam, pad, t_out)
    rng = np.random.default_rng(k + 10 * d)
    x, w = rng.standard_normal((2, c_in, t_in)), rng.standard_normal((c_out, c_in, k))
    x[0, 0, : min(3, t_in)] = 0.0
    bias, res, alpha = rng.standard_normal(c_out), rng.standard_normal((2, c_out, t_out)), _alpha(rng, c_in)
    got = R.conv(x, w, bias, alpha, res, k, s, d, pl, t_out, act, 0.2)
    assert got.shape == (2, c_out, t_out) and G.t_out_of(t_in, k, s, d, pl, pr) == t_out
    xt = _torch_act(torch.tensor(x), act, 0.2, torch.tensor(alpha))
    want = F.conv1d(F.pad(xt, (pl, pr)), torch.tensor(w), torch.tensor(bias), stride=s, dilation=d) + torch.tensor(res)
    assert np.abs(got - want.numpy()).max() < TOL
    ora = O.conv1d(_oracle_act(x, act, 0.2, alpha), w, bias, s, d, (pl, pr)) + res
    assert np.abs(got - ora).max() < TOL
    bare = R.conv(x, w, None, alpha, None, k, s, d, pl, t_out, act, 0.2)
    assert np.abs(bare - (want.numpy() - res - bias[None, :, None])).max() < TOL
    assert np.abs(got - G.forward(x, w, bias, alpha, res, k, s, d, pl, pr, act, 0.2)).max() < TOL


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("act", ACTS)
def test_convt_matches_torch_and_oracle(r, cached, act):
    c_in, c_out, t_in = 2 * R.CHUNK[2] + 1, 5, 7
    rng = np.random.default_rng(r)
    x, w = rng.standard_normal((2, c_in, t_in)), rng.standard_normal((c_in, c_out, 2 * r))
    bias, alpha = rng.standard_normal(c_out), _alpha(rng, c_in)
    pl, P, t_out = R.convt_geometry(t_in, r, cached)
    got = R.convt(x, w, bias, alpha, r, pl, P, act, 0.2)
    assert got.shape == (2, c_out, t_out)
    xt = _torch_act(torch.tensor(x), act, 0.2, torch.tensor(alpha))
    if cached:      # the overlap-add of the view, without the first and the last r columns (one history column)
        want = F.conv_transpose1d(xt, torch.tensor(w), torch.tensor(bias), stride=r)[..., r:t_in * r]
    else:
        want = F.conv_transpose1d(xt, torch.tensor(w), torch.tensor(bias), stride=r, padding=r // 2)
    assert np.abs(got - want.numpy()).max() < TOL
    ora = O.conv_transpose1d(_oracle_act(x, act, 0.2, alpha), w, r, r if cached else r // 2, bias)
    assert np.abs(got - ora).max() < TOL


def _unit_operands(rng, C):
    w1, w2 = rng.standard_normal((C, C, 3)) / np.sqrt(3 * C), rng.standard_normal((C, C, 1)) / np.sqrt(C)
    b1, b2 = 0.1 * rng.standard_normal(C), 0.1 * rng.standard_normal(C)
    return w1, w2, b1, b2, _alpha(rng, C), _alpha(rng, C)


def _torch_unit(x, ops, d, pl, act, res):
    w1, w2, b1, b2, a0, a2 = (torch.tensor(v) for v in ops)
    h = F.conv1d(F.pad(_torch_act(x, act, 0.2, a0), (pl, 2 * d - pl)), w1, b1, dilation=d)
    return res + F.conv1d(_torch_act(h, act, 0.2, a2), w2, b2)


@pytest.mark.parametrize("d", [1, 2, 3, 9])
@pytest.mark.parametrize("act", ACTS)
def test_unit_matches_torch_and_oracle_at_every_pad_left(d, act):
    C, T = 6, 11
    rng = np.random.default_rng(d)
    x, ops = rng.standard_normal((2, C, T)), _unit_operands(rng, C)
    for pl in sorted({0, 1, d, d + 1, 2 * d}):
        got = R.unit(x, *ops, d, pl, T, act, 0.2)
        want = _torch_unit(torch.tensor(x), ops, d, pl, act, torch.tensor(x))
        assert np.abs(got - want.numpy()).max() < TOL, pl
        w1, w2, b1, b2, a0, a2 = ops
        h = _oracle_act(O.conv1d(_oracle_act(x, act, 0.2, a0), w1, b1, 1, d, (pl, 2 * d - pl)), act, 0.2, a2)
        assert np.abs(got - (x + O.conv1d(h, w2, b2, 1, 1, (0, 0)))).max() < TOL, pl
    assert np.abs(R.unit(x, ops[0], ops[1], None, None, ops[4], ops[5], d, d, T, act, 0.2)
                  - _torch_unit(torch.tensor(x), (ops[0], ops[1], 0 * ops[2], 0 * ops[3], ops[4], ops[5]), d, d, act,
                                torch.tensor(x)).numpy()).max() < TOL


@pytest.mark.parametrize("causal", [False, True])
def test_unit_cached_form(causal):
    """x = [2 d history columns | block], pad_left 0, x_len = 2 d + t_len, the residual x shifted by
    2 d - delay; whatever lies past x_len is never read."""
    C, T, d = 5, 9, 3
    rng = np.random.default_rng(7)
    ops = _unit_operands(rng, C)
    xl, rs = 2 * d + T, 2 * d - (0 if causal else d)
    x = np.full((2, C, xl + 3), np.nan)
    x[:, :, :xl] = rng.standard_normal((2, C, xl))
    got = R.unit(x, *ops, d, 0, T, G.ACT_SNAKE, 0.2, x_len=xl, res_shift=rs)
    xt = torch.tensor(x[:, :, :xl])
    w1, w2, b1, b2, a0, a2 = (torch.tensor(v) for v in ops)
    h = F.conv1d(_torch_act(xt, G.ACT_SNAKE, 0.2, a0), w1, b1, dilation=d)
    want = xt[:, :, rs:rs + T] + F.conv1d(_torch_act(h, G.ACT_SNAKE, 0.2, a2), w2, b2)
    assert np.isfinite(got).all() and np.abs(got - want.numpy()).max() < TOL


def test_stack_is_three_units():
    C, T = 4, 13
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, C, T))
    units = [_unit_operands(rng, C) + (d, pl) for d, pl in ((1, 1), (3, 6), (9, 9))]
    got, S = R.stack(x, units, G.ACT_LEAKY, 0.2, cond=True)
    y = torch.tensor(x)
    for u in units:
        y = _torch_unit(y, u[:6], u[6], u[7], G.ACT_LEAKY, y)
    assert np.abs(got - y.numpy()).max() < TOL and S.shape == got.shape and bool((S >= np.abs(got) - 1e-9).all())


def test_float32_run_is_a_float32_chain():
    """The fp32 run keeps float32 after every step: on a long sum it differs from the rounded
    float64 result, by about sqrt(K) half-ulps, and stays within K ulps of it."""
    k, s, d = 3, 1, 1
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 512, 16)).astype(np.float32)
    w = rng.standard_normal((8, 512, 3)).astype(np.float32)
    r64, e_ref, S = R.with_e_ref(R.conv, x, w, None, None, None, k, s, d, 1, 16, G.ACT_NONE, 0.2)
    r32 = R.conv(x, w, None, None, None, k, s, d, 1, 16, G.ACT_NONE, 0.2, dtype=np.float32)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and S.dtype == np.float64
    assert not np.array_equal(r32, r64.astype(np.float32))
    eps = 2.0 ** -24
    assert 0 < e_ref <= 3 * 512 * eps * S.max()
    assert e_ref > eps * np.abs(r64).max()                 # more than one rounding of the result
    brute = np.einsum("ock,bckt->bot", np.abs(w.astype(np.float64)),
                      np.lib.stride_tricks.sliding_window_view(np.pad(np.abs(x.astype(np.float64)), ((0, 0), (0, 0), (1, 1))),
                                                               3, axis=2).transpose(0, 1, 3, 2))
    assert np.allclose(S, brute, rtol=1e-12)
    for fn, args in ((R.unit, (x[:, :8], w[:, :8], w[:, :8, :1], None, None, None, None, 1, 1, 16, G.ACT_LEAKY, 0.2)),
                     (R.convt, (x, w.transpose(1, 0, 2)[:, :, :2].repeat(2, axis=2), None, None, 2, 0, 1, G.ACT_NONE, 0.2))):
        y64, e, _ = R.with_e_ref(fn, *args)
        assert e > 0 and fn(*args, dtype=np.float32).dtype == np.float32
