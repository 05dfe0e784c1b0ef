"""tests/edge_ref.py against the float64 oracle (no GPU): head and tail in the composition
tests/test_gpu_edges.py uses (conv1d, reverse_half, get_padding, snake, leaky_relu), both padding
modes, both tail modes, both activations, noise on and off, F in {1, 5, 33, 257}; and that the
judge of tests/test_gpu_edge_sweep.py (err <= 4 e_ref) sees the faults it is there for: with the
float32 run as the stand-in for a correct kernel, six mutants of the restatement each leave the
bound on a named case."""
import functools

import numpy as np
import pytest

from oracle import rave_oracle as O
from tests import edge_ref as E, filterbank_ref as FB

FRAMES = (1, 5, 33, 257)
TOL = 1e-12


_FILTERS = {}


@pytest.fixture(scope="module", autouse=True)
def _load_filters(golden):
    """The PQMF prototype of the golden("pqmf") fixture, through the oracle's pqmf_filters."""
    _FILTERS["hkf"], _FILTERS["hki"] = O.pqmf_filters(golden("pqmf")["hk"])


def _filters():
    return _FILTERS["hkf"], _FILTERS["hki"]


def _pads(causal):
    return (O.get_padding(E.K7, causal=causal), O.get_padding(E.ANA_TAPS, causal=causal),
            O.get_padding(E.SYN_TAPS, causal=causal))


@functools.lru_cache(maxsize=None)
def _head_case(F, causal, nb=6, co=24, B=2, bias=True):
    rng = np.random.default_rng(F + 7 * causal + nb)
    T = 16 * F
    x = (0.3 * np.sin(np.arange(T) * 0.05)[None] + 0.1 * rng.standard_normal((B, T))).astype(np.float32)
    w = (rng.uniform(-1, 1, (co, nb, E.K7)) / np.sqrt(nb * E.K7)).astype(np.float32)
    b = (0.1 * rng.standard_normal(co)).astype(np.float32) if bias else None
    return x, w, b


@functools.lru_cache(maxsize=None)
def _tail_case(F, causal, mode, act, noise, B=2):
    rng = np.random.default_rng(F + 3 * mode + 5 * causal + 11 * act)
    co = 32 if mode == 1 else 16
    x = rng.standard_normal((B, 64, F)).astype(np.float32)
    x[0, 0, : min(3, F)] = 0.0
    w = (rng.uniform(-1, 1, (co, 64, E.K7)) / np.sqrt(64 * E.K7)).astype(np.float32)
    b = (0.1 * rng.standard_normal(co)).astype(np.float32)
    alpha = rng.uniform(0.1, 3.0, 64).astype(np.float32)
    alpha[-1] = 0.0
    nz = (0.05 * rng.standard_normal((B, 16, F))).astype(np.float32) if noise else None
    return x, w, b, alpha, nz


def _oracle_head(x, hkf, w, b, causal):
    cpad, ppad, _ = _pads(causal)
    nb = w.shape[1]
    bands = O.reverse_half(O.conv1d(x[:, None].astype(np.float64), hkf.astype(np.float64), None, stride=16, pad=ppad))[:, :nb]
    return O.conv1d(bands, w.astype(np.float64), None if b is None else b.astype(np.float64), pad=cpad)


def _oracle_tail(x, hki, w, b, alpha, nz, act, mode, causal):
    cpad, _, spad = _pads(causal)
    xa = O.leaky_relu(x.astype(np.float64)) if act == E.ACT_LEAKY else O.snake(x.astype(np.float64), alpha.reshape(-1, 1))
    wv = O.conv1d(xa, w.astype(np.float64), b.astype(np.float64), pad=cpad)
    if mode == 1:
        v, amp = np.split(wv, 2, axis=1)
        wv = v * (1.0 / (1.0 + np.exp(-amp)))
    wv = np.tanh(wv + (nz if nz is not None else 0.0))
    ys = O.conv1d(O.reverse_half(wv), hki.astype(np.float64), None, pad=spad) * 16
    return ys[:, ::-1, :].transpose(0, 2, 1).reshape(x.shape[0], -1)


# ================================================================== 1. float64 pins
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("F", FRAMES)
def test_head_matches_oracle(F, causal):
    hkf, _ = _filters()
    cpad, ppad, _ = _pads(causal)
    for nb, co, bias in ((6, 24, True), (5, 1, False), (8, 64, True)):
        x, w, b = _head_case(F, causal, nb, co, bias=bias)
        got, S = E.head(x, hkf, w, b, cpad[0], ppad[0], F, cond=True)
        want = _oracle_head(x, hkf, w, b, causal)
        assert got.shape == want.shape == (2, co, F) and got.dtype == np.float64
        assert np.abs(got - want).max() <= TOL * max(np.abs(want).max(), 1e-300), (nb, co)
        assert S.shape == got.shape and bool((S >= np.abs(got) - 1e-12).all())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("act", [E.ACT_LEAKY, E.ACT_SNAKE])
@pytest.mark.parametrize("noise", [False, True])
def test_tail_matches_oracle(noise, act, mode, causal):
    _, hki = _filters()
    cpad, _, spad = _pads(causal)
    for F in FRAMES:
        x, w, b, alpha, nz = _tail_case(F, causal, mode, act, noise)
        got, S = E.tail(x, hki, w, b, alpha, nz, act, 0.2, mode, cpad[0], spad[0], F, cond=True)
        want = _oracle_tail(x, hki, w, b, alpha, nz, act, mode, causal)
        assert got.shape == want.shape == (2, 16 * F) and got.dtype == np.float64
        assert np.abs(got - want).max() <= TOL * np.abs(want).max(), F
        # |y| <= 16 sum |hki| |s| <= S
        assert S.shape == got.shape and bool((S >= np.abs(got) - 1e-12).all())


def test_float32_runs_are_float32_chains():
    """The float32 runs differ from the rounded float64 results (they are chains held in float32, with
    a float32 intermediate), and e_ref stays far below the coarse bound 3 K eps S."""
    hkf, hki = _filters()
    cpad, ppad, spad = _pads(False)
    x, w, b = _head_case(33, False)
    r64, e_ref, S = E.with_e_ref(E.head, x, hkf, w, b, cpad[0], ppad[0], 33)
    r32 = E.head(x, hkf, w, b, cpad[0], ppad[0], 33, dtype=np.float32)
    assert r32.dtype == np.float32 and not np.array_equal(r32, r64.astype(np.float32))
    assert 0 < e_ref <= 3 * (513 + 42) * 2.0 ** -24 * S.max()
    x, w, b, alpha, nz = _tail_case(33, False, 1, E.ACT_SNAKE, True)
    args = (x, hki, w, b, alpha, nz, E.ACT_SNAKE, 0.2, 1, cpad[0], spad[0], 33)
    r64, e_ref, S = E.with_e_ref(E.tail, *args)
    r32 = E.tail(*args, dtype=np.float32)
    assert r32.dtype == np.float32 and not np.array_equal(r32, r64.astype(np.float32))
    assert 0 < e_ref <= 3 * (448 + 528) * 2.0 ** -24 * S.max()


def test_bands_take_the_global_parity():
    """bands() from an odd first frame equals the same frames cut from a run that starts at 0."""
    hkf, _ = _filters()
    x, _, _ = _head_case(33, False)
    whole = E.bands(x, hkf, 6, 256, 0, 33)
    for first in (-3, -6, 5, 8):
        part = E.bands(x, hkf, 6, 256, first, 12)
        lo = max(first, 0)
        assert np.abs(part[:, :, lo - first:] - whole[:, :, lo:first + 12]).max() <= 1e-15


# ================================================================== 2. the judge sees the faults
def _head_sweep():
    for causal in (False, True):
        for F in FRAMES:
            yield f"head F {F} {'causal' if causal else 'centred'}", F, causal


def _tail_sweep():
    for causal in (False, True):
        for F in FRAMES:
            for mode, act, noise in ((1, E.ACT_SNAKE, True), (2, E.ACT_LEAKY, False)):
                yield f"tail F {F} {'causal' if causal else 'centred'} mode {mode} act {act} noise {int(noise)}", F, causal, mode, act, noise


@functools.lru_cache(maxsize=None)
def _head_ref(F, causal):
    hkf, _ = _filters()
    cpad, ppad, _ = _pads(causal)
    x, w, b = _head_case(F, causal)
    return E.with_e_ref(E.head, x, hkf, w, b, cpad[0], ppad[0], F)


@functools.lru_cache(maxsize=None)
def _tail_ref(F, causal, mode, act, noise):
    _, hki = _filters()
    cpad, _, spad = _pads(causal)
    x, w, b, alpha, nz = _tail_case(F, causal, mode, act, noise)
    return E.with_e_ref(E.tail, x, hki, w, b, alpha, nz, act, 0.2, mode, cpad[0], spad[0], F)


def _passes(got32, ref):
    r64, e_ref, _ = ref
    assert got32.dtype == np.float32
    return float(np.abs(got32.astype(np.float64) - r64).max()) <= 4 * e_ref


def test_the_float32_run_passes_everywhere():
    hkf, hki = _filters()
    for name, F, causal in _head_sweep():
        cpad, ppad, _ = _pads(causal)
        x, w, b = _head_case(F, causal)
        assert _passes(E.head(x, hkf, w, b, cpad[0], ppad[0], F, dtype=np.float32), _head_ref(F, causal)), name
    for name, F, causal, mode, act, noise in _tail_sweep():
        cpad, _, spad = _pads(causal)
        x, w, b, alpha, nz = _tail_case(F, causal, mode, act, noise)
        got = E.tail(x, hki, w, b, alpha, nz, act, 0.2, mode, cpad[0], spad[0], F, dtype=np.float32)
        assert _passes(got, _tail_ref(F, causal, mode, act, noise)), name


# ---- the mutants: each the float32 restatement with one fault of the kind the kernels could have
f32 = np.float32


def _head_a(x, hkf, w, b, cpl, ppl, F):
    """(a) the bands outside [0, F) are the analysis of the zero-extended audio."""
    ext = E.bands(x, hkf, w.shape[1], ppl, -cpl, F + E.K7 - 1, f32)
    return E.head_conv(ext, w, b, 0, F, f32)


def _head_c(x, hkf, w, b, cpl, ppl, F):
    """(c) reverse_half's parity from the tile-local frame, the tile starting at g0 = n0 - conv_pad_left."""
    nb = w.shape[1]
    bd = E.bands(x, hkf, nb, ppl, 0, F, f32)
    k, f = np.arange(nb)[:, None], np.arange(F)[None, :]
    bd = bd * (FB.rh(k, f) * FB.rh(k, f + cpl)).astype(f32)[None]            # global sign off, local sign on
    return E.head_conv(bd, w, b, cpl, F, f32)


def _head_d(x, hkf, w, b, cpl, ppl, F):
    """(d) conv_pad_left off by one."""
    return E.head(x, hkf, w, b, cpl + 1, ppl, F, dtype=f32)


HEAD_MUTANTS = [("a", _head_a, "head F 5 centred"), ("a", _head_a, "head F 257 centred"), ("c", _head_c, "head F 33 centred"),
                ("d", _head_d, "head F 1 centred"), ("d", _head_d, "head F 257 causal")]


@pytest.mark.parametrize("letter,mutant,where", HEAD_MUTANTS, ids=[f"{m[0]}-{m[2].replace(' ', '_')}" for m in HEAD_MUTANTS])
def test_head_mutant_is_rejected(letter, mutant, where):
    hkf, _ = _filters()
    caught = []
    for name, F, causal in _head_sweep():
        cpad, ppad, _ = _pads(causal)
        x, w, b = _head_case(F, causal)
        if not _passes(mutant(x, hkf, w, b, cpad[0], ppad[0], F), _head_ref(F, causal)):
            caught.append(name)
    assert where in caught, f"mutant ({letter}) passes 4 e_ref at '{where}'; rejected only at {caught}"


def _tail_parts(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F):
    return E.tail_conv(x, w, b, alpha, act, 0.2, cpl, F, f32)


def _tail_b(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F):
    """(b) the conv's outputs outside [0, F) go through the epilogue (tanh(bias)) instead of being 0."""
    n = F + E.SYN_TAPS - 1
    c = E.conv(x, w, b, alpha, None, E.K7, 1, 1, cpl + spl, n, act, 0.2, dtype=f32, chunk=E.EDGE_CHUNK)   # frames -spl ...
    nze = None if nz is None else FB._window(nz, -spl, n, f32)
    return FB.synthesis(c, hki, 0, mode, -spl, n, nze, F, f32)


def _tail_d(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F):
    """(d) conv_pad_left off by one."""
    return E.tail(x, hki, w, b, alpha, nz, act, 0.2, mode, cpl - 1 if cpl else 1, spl, F, dtype=f32)


def _tail_e(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F, tap=16, col=32):
    """(e) one tap of the 33rd synthesis column dropped: the staged window's column 32 (the first one
    past a 32-column block) is not read by tap 16, so output frame 32 - 16 misses that term."""
    c = _tail_parts(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F)
    y = FB.synthesis(c, hki, spl, mode, 0, 0, nz, F, f32).astype(np.float64)
    t = col - tap
    if t < F:
        win = FB.staged(c, spl, mode, 0, 0, nz, F, f32).astype(np.float64)
        h = np.asarray(hki, np.float64)
        term = np.zeros((x.shape[0], 16))
        for ch in range(16):
            term = term + h[None, :, ch, tap] * win[:, None, ch, col]
        y[:, 16 * t:16 * t + 16] -= 16 * term[:, ::-1]
    return y.astype(f32)


def _tail_f(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F):
    """(f) the amplitude half read from channels 0..15."""
    c = _tail_parts(x, hki, w, b, alpha, nz, act, mode, cpl, spl, F)
    c = np.concatenate([c[:, :16], c[:, :16]], axis=1)
    return FB.synthesis(c, hki, spl, mode, 0, 0, nz, F, f32)


TAIL_MUTANTS = [("b", _tail_b, "tail F 1 centred mode 1 act 2 noise 1"), ("b", _tail_b, "tail F 257 causal mode 2 act 1 noise 0"),
                ("d", _tail_d, "tail F 33 causal mode 2 act 1 noise 0"), ("e", _tail_e, "tail F 33 centred mode 2 act 1 noise 0"),
                ("e", _tail_e, "tail F 257 causal mode 1 act 2 noise 1"), ("f", _tail_f, "tail F 5 centred mode 1 act 2 noise 1")]


@pytest.mark.parametrize("letter,mutant,where", TAIL_MUTANTS, ids=[f"{m[0]}-{m[2].replace(' ', '_')}" for m in TAIL_MUTANTS])
def test_tail_mutant_is_rejected(letter, mutant, where):
    _, hki = _filters()
    caught = []
    for name, F, causal, mode, act, noise in _tail_sweep():
        cpad, _, spad = _pads(causal)
        x, w, b, alpha, nz = _tail_case(F, causal, mode, act, noise)
        got = mutant(x, hki, w, b, alpha, nz, act, mode, cpad[0], spad[0], F)
        if not _passes(got, _tail_ref(F, causal, mode, act, noise)):
            caught.append(name)
    assert where in caught, f"mutant ({letter}) passes 4 e_ref at '{where}'; rejected only at {caught}"
    if letter == "f":                                  # mode 2 has no amplitude half: the mutant is the kernel there
        assert not [n for n in caught if "mode 2" in n]
