"""The pitch tests' CPU reference (tests/pitch_ref.py) checked on the host: its
FFT-route d(tau) against a direct float64 evaluation of the three sums of the
definition, its search against a plain loop, the class-256 catch-alls of the
one-hot, the frame counts, and that the fp32 run of the restatement itself
stays inside the caps the GPU tests grant (2 % of frames excused, 1 % of the
one-hot table's periods).  No GPU."""
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
