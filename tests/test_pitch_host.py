"""The pitch tests' CPU reference (tests/pitch_ref.py) checked on the host: its
FFT-route d(tau) against a direct float64 evaluation of the three sums of the
definition, its search against a plain loop, the class-256 catch-alls of the
one-hot, the frame counts, and that the fp32 run of the restatement itself
stays inside the caps the GPU tests grant (2 % of frames excused, 1 % of the
one-hot table's periods); and the edge sweep's exact sums, derived bound and
constructed rows (tests/pitch_ref.py SWEEP) that tests/test_gpu_pitch_edges.py
judges the kernels by.  No GPU."""
import numpy as np
import pytest
import torch

from tests import pitch_ref as R


@pytest.mark.parametrize("case", ["est", "short", "wave"])
def test_fft_route_matches_the_direct_sums(case):
    c = R.CASES[case]
    tau_min, tau_max, L, stride, _ = R.geometry(case)
    x = torch.tensor(R.inputs(case), dtype=torch.float64)
    frames = R.frame(x, L, stride).reshape(-1, L)
    got = R.diff_fft(frames, tau_max).numpy()
    f = frames.numpy()
    sq = np.concatenate([np.zeros((len(f), 1)), np.cumsum(f * f, -1)], -1)          # sq[i] = sum_{j<i} x_j^2
    want = np.empty_like(got)
    for tau in range(tau_max):
        r = (f[:, :L - tau] * f[:, tau:]).sum(-1)
        want[:, tau] = sq[:, L] + (sq[:, L - tau] - sq[:, tau]) - 2 * r
    scale = np.abs(sq[:, L]).max()
    assert np.abs(got - want).max() <= 1e-12 * scale
    # cmdf as the issue states it
    d = want[:, 1:]
    cm = d * np.arange(1, tau_max) / np.maximum(np.cumsum(d, -1), 1e-5)
    ref = R.reference(case)[0].reshape(-1, tau_max - 1 - tau_min).numpy()
    assert ref.shape == (len(f), tau_max - 1 - tau_min)
    assert np.abs(cm[:, tau_min:] - ref).max() <= 1e-10


def _loop_search(c, tau_max, threshold):
    below = [j for j in range(len(c)) if c[j] < threshold]
    first = below[0] if below and below[0] > 0 else tau_max
    for j in range(len(c)):
        if j >= first and (j == len(c) - 1 or c[j + 1] - c[j] >= 0.0):
            return j
    return 0


def test_search_matches_a_plain_loop():
    rng = np.random.Generator(np.random.PCG64(5))
    rows = [rng.uniform(0.0, 1.0, 40) for _ in range(200)]
    rows += [np.full(40, 0.5), np.full(40, 0.05), np.linspace(1, 0, 40), np.linspace(0, 1, 40),
             np.r_[np.full(39, 0.5), 0.01], np.r_[0.01, np.full(39, 0.5)], np.r_[0.5, 0.05, np.full(38, 0.05)]]
    c = np.stack(rows)
    got = R.search(torch.from_numpy(c), 60, 0.1).numpy()
    want = np.array([_loop_search(r, 60, 0.1) for r in c])
    assert np.array_equal(got, want)
    assert np.array_equal(R.margins(c, 0.1)[0], want)
    assert want[200] == 0 and want[201] == 0          # none below; index 0 below: both unvoiced
    assert want[202] == 39 and want[204] == 39        # falling to the end: the last index counts as rising
    assert (want > 0).any()


@pytest.mark.parametrize("case", list(R.CASES))
def test_reference_decisions_match_the_loop_and_f0(case):
    c = R.CASES[case]
    tau_min, tau_max = R.geometry(case)[:2]
    cmdf, idx, f0 = R.reference(case)
    loop, _ = R.margins(cmdf.reshape(-1, cmdf.shape[-1]).numpy())
    assert np.array_equal(loop, idx.reshape(-1).numpy())
    want = np.where(loop > 0, c["sr"] / (loop + tau_min + 1.0), 0.0)
    np.testing.assert_allclose(f0.reshape(-1).numpy(), want, rtol=1e-15, atol=0)
    assert np.array_equal(f0.reshape(-1).numpy() == 0, loop == 0)


@pytest.mark.parametrize("case", list(R.CASES))
def test_frame_counts(case):
    c = R.CASES[case]
    tau_min, tau_max, L, stride, frames = R.geometry(case)
    cmdf, idx, _ = R.reference(case)
    assert tuple(idx.shape) == c["shape"][:-1] + (frames,)
    assert cmdf.shape[-1] == tau_max - 1 - tau_min
    if "block" in c:
        assert frames == c["shape"][-1] // c["block"] == 16
        x = torch.tensor(R.inputs(case), dtype=torch.float64)
        assert torch.equal(R.get_pitch(x, c["block"]), R.reference(case)[2])
    for T, block in [(16384, 1024), (65536, 1024)]:   # the shapes the bench and the conditioner run
        L = 2 * int(44100 / 70.0)
        stride = int((T - L) / (T / block - 1) / 44100 * 44100)
        assert (T - L) // stride + 1 == T // block


@pytest.mark.parametrize("case", list(R.CASES))
def test_fp32_restatement_stays_within_the_excused_cap(case):
    c64, i64, _ = R.reference(case)
    c32, i32, _ = R.reference(case, "float32")
    e_ref = float((c32.double() - c64).abs().max())
    assert e_ref > 0
    _, margin = R.margins(c64.reshape(-1, c64.shape[-1]).numpy())
    excused = margin < 4 * e_ref
    differ = (i32 != i64).reshape(-1).numpy()
    print(f"case {case}: e_ref {e_ref:.3e}, {int(excused.sum())} excused, {int(differ.sum())} differ of {len(differ)}")
    assert excused.sum() <= R.EXCUSED_CAP * len(excused)
    assert not (differ & ~excused).any()
    if case != "short":
        assert (i64 > 0).any() and (i64 == 0).any()


def test_class_256_catches_zero_and_both_ends():
    f0 = torch.tensor([[0.0, 1.5, 2.02, 40.0, 100.0, 795.0, 797.0, 900.0, float("inf")]], dtype=torch.float64)
    v = R.f0_norm(f0)[0]
    assert torch.isnan(v[0]) and v[1] < 0 and 0 <= v[2] and v[5] < 1 <= v[6]
    k = R.f0_classes(f0)[0].tolist()
    assert k[0] == k[1] == k[6] == k[7] == k[8] == 256
    assert k[2] == 0 and k[5] == 255 and k[3] == 128 and 0 < k[4] < 256
    hot = R.f0_one_hot(f0)
    assert hot.shape == (1, 9, 257) and torch.equal(hot.argmax(-1)[0], torch.tensor(k))
    assert torch.equal(hot.sum(-1), torch.ones(1, 9))
    # floor(256 v) on the exact edges i / 256 is the bucketize class
    inside = (v >= 0) & (v < 1)
    assert torch.equal(torch.floor(v[inside] * 256).long(), torch.tensor(k)[inside])


def test_fp32_one_hot_table_stays_within_its_cap():
    f0 = torch.from_numpy(R.table_f0())
    assert len(f0) == 630 - 110 + 3
    v = R.f0_norm(f0.double())
    near = ((v * 256 - (v * 256).round()).abs() / 256 < R.ONEHOT_EDGE)[:-3]
    differ = (R.f0_classes(f0) != R.f0_classes(f0.double()))[:-3]
    assert near.sum() <= R.ONEHOT_CAP * (len(f0) - 3)
    assert not (differ & ~near).any()
    assert R.f0_classes(f0.double())[-3:].tolist() == [256, 256, 256]


# ------------------------------------------------------------------ the edge sweep
def _group(kind, tau_max):
    return [n for n, c in R.SWEEP.items() if c["kind"] == kind and c["tau_max"] == tau_max]


GROUPS = [("sweep", t) for t in R.SWEEP_TAU_MAX] + [("frame", t) for t in R.FRAME_TAU_MAX] + [("thr", 64), ("thr", 257)]


def _three_sums(f, tau_max):
    """The unsliced cmdf by the kernel's formula, c0 + (sq[L - tau] - sq[tau]) - 2 r, in float64 numpy."""
    L = f.shape[-1]
    sq = np.concatenate([np.zeros((len(f), 1)), np.cumsum(f * f, -1)], -1)
    d = np.empty((len(f), tau_max))
    for tau in range(tau_max):
        d[:, tau] = sq[:, L] + (sq[:, L - tau] - sq[:, tau]) - 2 * (f[:, :L - tau] * f[:, tau:]).sum(-1)
    return d[:, 1:] * np.arange(1, tau_max) / np.maximum(np.cumsum(d[:, 1:], -1), 1e-5)


def test_sweep_covers_what_it_claims():
    sweep = [c for c in R.SWEEP.values() if c["kind"] == "sweep"]
    assert {c["tau_max"] for c in sweep} == set(R.SWEEP_TAU_MAX)
    assert {c["tau_max"] % 4 for c in sweep if c["tau_max"] <= 256} == {0, 1, 2, 3}
    assert {c["tau_max"] % 4 for c in sweep if c["tau_max"] > 256} == {0, 1, 2, 3}
    assert {0, 1} <= {c["tau_min"] for c in sweep} and all(c["tau_min"] < c["tau_max"] - 1 for c in sweep)
    for c in sweep:
        total = len(c["rows"]) * c["frames"]
        assert (total == 2) if c["tau_max"] == 2205 else (total in (50, 55) and c["frames"] == 5)
    frame = [c for c in R.SWEEP.values() if c["kind"] == "frame"]
    for tau_max in R.FRAME_TAU_MAX:
        mine = [c for c in frame if c["tau_max"] == tau_max]
        L = 2 * tau_max
        assert {len(c["rows"]) * c["frames"] for c in mine} >= {1, 2, 3, 5, 7}
        assert {c["stride"] for c in mine} == {1, 3, L, L + 5}
        for s in (1, 3, L, L + 5):
            assert {c["T"] for c in mine if c["stride"] == s} >= {1, L - 1, L, L + 1, L + s - 1, L + s}
    for name, c in R.SWEEP.items():
        x = R.sweep_input(name)
        assert x.shape == (len(c["rows"]), c["T"]) and x.dtype == np.float32


@pytest.mark.parametrize("kind,tau_max", GROUPS)
def test_three_sum_route_stays_within_the_bound_of_the_exact_sums(kind, tau_max):
    """The bound on the formula it bounds, per row; a silent frame gives exactly
    0.  The float64 FFT restatement's distance to the truth is printed, not
    asserted: on the DC rows it is 1e-10 and more, no ground truth there."""
    for name in _group(kind, tau_max):
        c, t = R.SWEEP[name], R.sweep_truth(name)
        x = torch.tensor(R.sweep_input(name), dtype=torch.float64)
        fr = R.frame(x, c["L"], c["stride"]).numpy()
        for r, row in enumerate(c["rows"]):
            ok = ~t["poisoned"][r]
            if not ok.any():
                continue
            got = _three_sums(fr[r][ok], tau_max)[:, c["tau_min"]:]
            err = np.abs(got - t["cmdf"][r][ok])
            assert (err <= t["bound"][r][ok]).all(), (name, row, float((err - t["bound"][r][ok]).max()))
            worst = float((err / np.maximum(t["bound"][r][ok], 1e-300)).max())
            fft = float(np.abs(t["fft64"][r][ok] - t["cmdf"][r][ok]).max())
            print(f"{name} row {r} {row}: three sums err/bound {worst:.3f}, bound max {float(t['bound'][r][ok].max()):.2e}, "
                  f"fft64 off the truth by {fft:.2e}")
            if row == "silence":
                assert (t["bound"][r] == 0).all() and (t["cmdf"][r] == 0).all() and (got == 0).all()
            if row == "glide":
                assert fft <= 1e-10


@pytest.mark.parametrize("kind,tau_max", GROUPS)
def test_sweep_margins_and_the_fp32_restatement(kind, tau_max):
    """Frames whose margin lies below the bound stay within EXCUSED_CAP per
    case.  The fp32 restatement decides like the truth outside the frames that
    4 e_ref excuses: the existing rule, kept for the glide rows only -- on the DC
    and special rows e_ref measures the FFT's cancellation (7.7e-2 on a cmdf of
    order 1), not a tolerance anyone could grant."""
    for name in _group(kind, tau_max):
        c, t = R.SWEEP[name], R.sweep_truth(name)
        excused = t["margin"] < t["limit"]
        print(f"{name}: {int(excused.sum())} of {excused.size} frames below the bound")
        assert excused.sum() <= R.EXCUSED_CAP * excused.size, name
        g = [r for r, row in enumerate(c["rows"]) if row == "glide"]
        e_ref = float(np.abs(t["fft32"][g] - t["fft64"][g]).max())
        assert e_ref > 0 or kind != "sweep"
        assert np.array_equal(t["idx_fft64"][g], t["idx"][g]), name
        ex32 = t["margin"][g] < 4 * e_ref
        differ = t["idx_fft32"][g] != t["idx"][g]
        print(f"{name}: e_ref {e_ref:.3e}, {int(ex32.sum())} excused by 4 e_ref, {int(differ.sum())} differ")
        assert not (differ & ~ex32).any(), name


@pytest.mark.parametrize("tau_max", [t for t in R.SWEEP_TAU_MAX if t != 2205])
def test_special_rows_produce_what_they_were_built_for(tau_max):
    seen = set()
    for name in _group("sweep", tau_max):
        c, t = R.SWEEP[name], R.sweep_truth(name)
        want = R.intended(name)
        for r, row in enumerate(c["rows"]):
            idx, cm = t["idx"][r], t["cmdf"][r]
            if row in want:
                assert not (t["margin"][r] < t["limit"][r]).any(), (name, row)
                seen.add(want[row])
            if want.get(row) == "last":
                assert (idx == c["m"] - 1).all() and c["m"] > 1, (name, row, idx)
                assert (cm[:, 0] >= c["threshold"]).all()
            elif want.get(row) == "first0":
                assert (idx == 0).all() and (cm[:, 0] < c["threshold"]).all(), (name, row)
            elif want.get(row) == "unvoiced":
                hit = cm.any(-1)                # the frames that hold the impulse; the others are silent
                assert (idx == 0).all() and hit.any() and (cm[hit] >= c["threshold"]).all(), (name, row)
            if row in ("nan", "inf"):
                p = t["poisoned"][r]
                assert 0 < p.sum() < len(p)
                assert np.isnan(t["fft64"][r][p]).all() and (t["idx_fft64"][r][p] == 0).all()
                assert np.isfinite(t["fft64"][r][~p]).all()
                assert np.array_equal(t["idx_fft64"][r][~p], idx[~p])
            else:
                assert not t["poisoned"][r].any()
        g = [r for r, row in enumerate(c["rows"]) if row == "glide"]
        if tau_max >= 63 and c["tau_min"] <= tau_max // 5:
            seen.add("voiced" if (t["idx"][g] > 0).any() else "")
    assert seen >= ({"first0", "unvoiced", "last"} | ({"voiced"} if tau_max >= 63 else set()))


@pytest.mark.parametrize("tau_max", [64, 257])
def test_threshold_cases(tau_max):
    for name in _group("thr", tau_max):
        c, t = R.SWEEP[name], R.sweep_truth(name)
        if c["threshold"] in (2.0, float("inf")):
            assert (t["cmdf"][..., 0] < c["threshold"]).all() and (t["idx"] == 0).all()      # index 0 passes
        elif c["threshold"] <= 0.0:
            assert (t["cmdf"] >= c["threshold"]).all() and (t["idx"] == 0).all()              # none below
        else:
            assert (t["idx"] > 0).any() and (t["idx"] == 0).any()


@pytest.mark.parametrize("bins", [1, 2, 256, 4096])
def test_onehot_edge_neighbours_in_float64(bins):
    """What the GPU test may excuse among the constructed values: float64 itself
    puts the rounded edge and its fp32 neighbours out to +-2 ulp within
    ONEHOT_EDGE of the edge (one ulp of f0 moves v by 1e-8 to 2e-8), so they are
    all excused; at +-ONEHOT_FAR ulp it is clear of the edge and the class is
    fixed.  The special values and a log-uniform sample, which carries the cap."""
    f0, k, off = R.onehot_edges(bins)
    assert len(f0) == 7 * min(bins + 1, 512) and (f0 > 0).all()
    v = R.f0_norm(torch.from_numpy(f0).double()).numpy()
    dist = np.abs(v - k / bins)
    near = np.abs(off) <= 2
    assert (dist[near] < R.ONEHOT_EDGE).all() and (dist[~near] > R.ONEHOT_EDGE).all()
    assert dist[~near].max() < 0.5 / 4096
    cls = R.f0_classes(torch.from_numpy(f0).double(), bins).numpy()
    above = np.where(k < bins, k, bins)
    below = np.where(k > 0, k - 1, bins)
    assert np.array_equal(cls[off == R.ONEHOT_FAR], above[off == R.ONEHOT_FAR])
    assert np.array_equal(cls[off == -R.ONEHOT_FAR], below[off == -R.ONEHOT_FAR])
    assert ((cls == above) | (cls == below)).all()
    special = torch.tensor(R.ONEHOT_SPECIAL, dtype=torch.float32)
    assert R.f0_classes(special.double(), bins).tolist() == [bins] * len(special)
    s = R.onehot_sample(771)
    vs = R.f0_norm(torch.from_numpy(s).double()).numpy() * bins
    close = np.abs(vs - np.round(vs)) / bins < R.ONEHOT_EDGE
    assert close.sum() <= R.ONEHOT_CAP * len(s)
    ks = R.f0_classes(torch.from_numpy(s).double(), bins).numpy()
    assert (ks == bins).any() and (ks < bins).any()
