"""tests/aux_ref.py against what the repository already trusts, on the CPU: the
splitmix known answers, the oracle (RVQ, AdaIN, the noise filter stage, the
pooling formulas of oracle/speaker_oracle.py), torch's own ops, and the proof
that the excused-frame caps of tests/test_gpu_aux_kernels.py hold for the
float64 reference alone on the inputs those tests use."""
import numpy as np
import pytest
import torch

from tests import aux_ref as R


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ------------------------------------------------------------------ uniform draw
def test_splitmix_known_answers():
    # splitmix64 seeded with 0: its published first outputs
    s, out = 0, []
    for _ in range(3):
        s = (s + R.G) & R.M64
        out.append(R.mix_int(s))
    assert out == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # the draw before the seed was hashed: seed 0, element 0
    assert int(R.uniform_state(0, 1, hashed_seed=False)[0]) == 0xE220A8397B1DCDAF
    assert float(R.uniform(0, 1, hashed_seed=False)[0]) == 0.8833107948303223
    # the draw as it stands (Python-int arithmetic, computed apart from numpy's)
    assert R.stream_key(0) == 0xE220A8397B1DCDAF
    assert [int(v) for v in R.uniform_state(0, 3)] == [0xA706DD2F4D197E6F, 0xB382A305F4414F5E, 0x631A9154FBABF717]
    assert R.uniform(0, 3).tolist() == [0.6524484753608704, 0.7012121081352234, 0.38712412118911743]
    assert R.stream_key(0x5EED) == 0x09F1FD9D03F0A9B4
    assert R.uniform(0x5EED, 3).tolist() == [0.07230788469314575, 0.7454074621200562, 0.6282155513763428]
    first = R.engine_seed(R.ENGINE_BASES[0], 1)
    assert first == 0xC276E44204ED84E8 and R.stream_key(first) == 0x9417034723148989
    assert R.uniform(first, 3).tolist() == [0.13752198219299316, 0.33699971437454224, 0.7911560535430908]


def test_numpy_mix_equals_the_integer_one():
    rng = np.random.default_rng(0)
    z = rng.integers(0, 1 << 64, 4096, dtype=np.uint64)
    z[:4] = [0, 1, R.M64, R.G]
    assert [int(v) for v in R.mix(z)] == [R.mix_int(int(v)) for v in z]
    seed = 0xFFFFFFFFFFFFFFF0                               # the counter wraps mod 2^64
    want = [R.mix_int(R.stream_key(seed) + R.G * (i + 1)) for i in range(8)]
    assert [int(v) for v in R.uniform_state(seed, 8)] == want


def test_ranges_and_moments_of_the_restatement():
    u = R.uniform(7, 1 << 20)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert abs(float(u.mean(dtype=np.float64)) - 0.5) < 5 * 0.28868 / 1024
    assert abs(float(u.var(dtype=np.float64)) - 1 / 12) < 5 * np.sqrt(1 / 180) / 1024
    assert np.unique(u, return_counts=True)[1].max() <= R.repeat_cap(1 << 20) == 8
    for lo, hi in [(-1.0, 1.0), (0.25, 0.75)]:
        v = R.uniform(7, 1000, lo, hi)
        assert v.min() >= lo and v.max() < hi


def lag1_equal(a, b):
    """Positions at which b[i] == a[i + 1]."""
    return int((b[:-1] == a[1:]).sum())


def lag1_cap(n):
    p = n * 2.0 ** -24
    return p + 6 * np.sqrt(p) + 1


@pytest.mark.parametrize("base", R.ENGINE_BASES)
def test_engine_schedule_shift_and_its_cure(base):
    """Unhashed, the engine's seeds base + G c make call c + 1 the bitwise copy
    of call c moved by one element; hashed, consecutive calls are unrelated."""
    n = 65536
    for c in range(1, 5):
        s0, s1 = R.engine_seed(base, c), R.engine_seed(base, c + 1)
        a, b = R.uniform(s0, n, hashed_seed=False), R.uniform(s1, n, hashed_seed=False)
        assert np.array_equal(b[:-1], a[1:])
        assert R.xcorr(a, b, 8)[8 - 1] > 0.99                     # lag -1: b[t - 1] == a[t]
        a, b = R.uniform(s0, n), R.uniform(s1, n)
        assert np.abs(R.xcorr(a, b, 8)).max() < 6 / np.sqrt(n)
        assert lag1_equal(a, b) <= lag1_cap(n)


# ------------------------------------------------------------------ RVQ
def test_rvq_restatement_vs_oracle_and_gap_rule():
    from oracle.rave_oracle import Oracle
    from rave_amd import config as rcfg
    from tests.test_gpu_parity import _rvq_encode_np
    z, cbs = R.rvq_case("k65")
    idx, gap = R.rvq_encode(z, cbs)
    idx2, gap2 = _rvq_encode_np(z, cbs)
    assert np.array_equal(idx, idx2) and maxabs(gap, gap2) < 1e-9
    o = Oracle(rcfg.discrete(), {}, np.zeros(1))
    o.codebooks = lambda: list(cbs.astype(np.float64))
    assert np.array_equal(o.rvq_encode(z), idx)
    assert maxabs(o.rvq_decode(idx), R.rvq_decode(idx, cbs)) < 1e-5
    bad = idx.copy()
    bad[0, 0, :2], bad[1, 1, :2] = -5, cbs.shape[1] + 3
    clamped = np.clip(bad, 0, cbs.shape[1] - 1)
    assert np.array_equal(R.rvq_decode(bad, cbs), R.rvq_decode(clamped, cbs))


@pytest.mark.parametrize("name", list(R.RVQ_CASES))
def test_rvq_excused_cap_holds_for_the_reference_alone(name):
    z, cbs = R.rvq_case(name)
    _, gap = R.rvq_encode(z, cbs)
    low = int((gap < R.GAP_RULE).sum())
    print(f"rvq case {name}: {low} of {gap.size} float64 gaps below {R.GAP_RULE}, smallest {gap.min():.3e}")
    assert low <= R.EXCUSED_CAP * gap.size


@pytest.mark.parametrize("D", [128, 64])
def test_rvq_tie_cases_are_ties_with_a_wide_margin(D):
    z, cbs, pair_of, want = R.rvq_tie_case(D)
    for a, b in R.TIE_PAIRS:
        assert np.array_equal(cbs[:, a].view(np.uint32), cbs[:, b].view(np.uint32))
    win, margin = R.rvq_pair_margin(z, cbs, pair_of)
    print(f"tie case D={D}: smallest float64 margin over the other codes {margin.min():.1f}")
    assert np.array_equal(win, want) and margin.min() > 1.0
    idx, gap = R.rvq_encode(z, cbs)                     # the plain argmin takes the first of a tie
    assert np.array_equal(idx, want) and float(np.abs(gap).max()) < 1e-3
    used = {int(k) for k in want.ravel()}
    assert used == {a for a, _ in R.TIE_PAIRS}           # every pair is exercised, in both layers
    assert {int(k) for k in want[:, 0].ravel()} == {int(k) for k in want[:, 1].ravel()} == used


# ------------------------------------------------------------------ AdaIN
def test_adain_restatement_vs_oracle():
    from oracle.rave_oracle import Oracle
    from rave_amd import config as rcfg
    rng = np.random.default_rng(3)
    B, Cc, T, MB = 3, 5, 63, 8
    o = Oracle(rcfg.v3(capacity=8), {}, np.zeros(1),
               adain_stats=Oracle.fresh_adain_state([("m", Cc)], MB))
    st = o.adain_stats["m"]
    stats = torch.zeros(4, MB, Cc, dtype=torch.float64)
    stats[1] = stats[3] = 1.0
    counters = [0.0, 0.0]
    for mode in (0, 2, 1, 2, 1, 0, 1):
        x = rng.standard_normal((B, Cc, T)) * 1.7 + 0.3
        o.learn_x, o.learn_y = mode == 1, mode == 2
        want = o._adain(x.copy(), "m")
        y, stats, counters = R.adain(torch.from_numpy(x), stats, counters, mode, 0)
        assert maxabs(y.numpy(), want) < 1e-12
        for i, k in enumerate(("mean_x", "std_x", "mean_y", "std_y")):
            assert maxabs(stats[i].numpy(), st[k][..., 0]) < 1e-12
        assert counters == [st["num_update_x"], st["num_update_y"]]
    # rows outside [row0, row0 + B) stay
    y, s2, _ = R.adain(torch.from_numpy(x), stats, counters, 1, 4)
    assert torch.equal(s2[:, :4], stats[:, :4]) and torch.equal(s2[:, 7:], stats[:, 7:])
    assert not torch.equal(s2[:2, 4:7], stats[:2, 4:7]) and torch.equal(s2[2:], stats[2:])


# ------------------------------------------------------------------ noise filter stage
def test_noise_restatement_vs_oracle():
    from oracle.rave_oracle import Oracle
    from rave_amd import config as rcfg
    cfg = rcfg.v3_noise()
    rng = np.random.default_rng(5)
    B, Fn, nb, tgt = 2, 33, 5, 8
    amp = (rng.standard_normal((B, 16 * nb, Fn)) * 4 + 3).astype(np.float32)
    u = rng.uniform(0, 1, (B, Fn, 16, tgt)).astype(np.float32)
    o = Oracle(cfg, {}, np.zeros(256))
    o._conv = lambda x, *a, **k: x
    o._act = lambda x, *a, **k: x
    want = o.noise_generator(amp.astype(np.float64), u)
    got = R.noise_synth(amp, u, 16, nb, tgt)
    assert got.shape == want.shape and maxabs(got, want) < 1e-13
    got32 = R.noise_synth(amp, u, 16, nb, tgt, np.float32)
    assert got32.dtype == np.float32 and 0 < maxabs(got32, want) < 1e-5


@pytest.mark.parametrize("nb,tgt", [(5, 8), (5, 16), (9, 16)])
def test_noise_restatement_vs_direct_convolution(nb, tgt):
    """The kept half of the circular product is the causal convolution of
    2 u - 1 with the padded impulse response (include/rave_amd.h)."""
    rng = np.random.default_rng(nb * tgt)
    amp = (rng.standard_normal((1, 3 * nb, 4)) * 4 + 3)
    u = rng.uniform(0, 1, (1, 4, 3, tgt))
    got = R.noise_synth(amp, u, 3, nb, tgt).reshape(3, 4, tgt)
    fs = 2 * (nb - 1)
    A = 2 / (1 + np.exp(-(amp[0] - 5))) ** 2.3 + 1e-7
    for j in range(3):
        for f in range(4):
            a = A[j * nb:(j + 1) * nb, f]
            n = np.arange(fs)
            ir = (a[0] + (-1.0) ** n * a[-1] + 2 * (a[1:-1, None] * np.cos(2 * np.pi * np.arange(1, nb - 1)[:, None] * n / fs)).sum(0)) / fs
            win = 0.5 - 0.5 * np.cos(2 * np.pi * n / fs)
            h = np.zeros(tgt)
            h[:fs // 2] = ir[:fs // 2] * win[fs // 2:]
            h[tgt - fs // 2:] = ir[fs // 2:] * win[:fs // 2]
            s = 2 * u[0, f, j] - 1
            want = np.array([sum(s[m] * h[i - m] for m in range(i + 1)) for i in range(tgt)])
            assert maxabs(got[j, f], want) < 1e-13


# ------------------------------------------------------------------ pooling head
def test_pooling_restatements_vs_the_oracle_formulas():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 7, 333))
    lg = 3 * rng.standard_normal((2, 7, 333))
    a = np.where(x > 0, x, 0.2 * x)                           # speaker_oracle.py: leaky_relu, then the lines below
    want = np.concatenate([a.mean(-1), np.sqrt(np.clip(a.var(-1, ddof=1), 1e-4, 1e4))], 1)
    assert maxabs(R.row_stats(torch.from_numpy(x), "leaky", 0.2, 1e-4, 1e4), want) < 1e-12
    w = np.exp(lg - lg.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    mu = (a * w).sum(-1)
    want = np.concatenate([mu, np.sqrt(np.clip((a ** 2 * w).sum(-1) - mu ** 2, 1e-4, 1e4))], 1)
    assert maxabs(R.attn_pool(torch.from_numpy(x), torch.from_numpy(lg), "leaky", 0.2, 1e-4, 1e4), want) < 1e-12
    assert torch.equal(R.row_stats(torch.from_numpy(x), "none", 0.2, 1e-4, 1e4)[:, :7], torch.from_numpy(x).mean(-1))


def test_linear_maxpool_shift_vs_torch():
    from tests.test_gpu_parity import _shift_ref
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.standard_normal((2, 65)))
    w = torch.from_numpy(rng.standard_normal((5, 65)))
    b = torch.from_numpy(rng.standard_normal(5))
    assert torch.allclose(R.linear(x, w, b), torch.nn.functional.linear(x, w, b), rtol=0, atol=1e-13)
    assert torch.allclose(R.linear(x, w), torch.nn.functional.linear(x, w), rtol=0, atol=1e-13)
    v = rng.standard_normal((2, 7, 101)).astype(np.float32)
    for k in (2, 3):
        assert np.array_equal(R.maxpool(v, k), torch.nn.functional.max_pool1d(torch.from_numpy(v), k).numpy())
    assert np.array_equal(R.shift_history(v, 64, 7), _shift_ref(v, 64, 7))
    assert np.array_equal(R.shift_history(v, 30, 71), _shift_ref(v, 30, 71))
