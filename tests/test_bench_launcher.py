"""bench.py's --gpus N launcher (no GPU): N ranks really start, the rank-0
line reports them, and a WORLD_SIZE that disagrees with --gpus is refused."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _json_line(out: str):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus_2_launches_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["steps"] == 3


def test_gpus_1_runs_in_process():
    r = subprocess.run([sys.executable, BENCH, "--dry-run"], env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 1 and line["ranks_seen"] == 1


def test_world_size_mismatch_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-run"],
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2
    assert "WORLD_SIZE=2" in r.stderr


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs' writer: whole float32 arrays under the byte budget; over
    it, the same seeded sample of each array on every call, within the budget."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    rng = np.random.default_rng(0)
    t = {"latents": torch.from_numpy(rng.standard_normal((3, 5, 7))),            # float64 in, float32 out
         "audio": torch.from_numpy(rng.standard_normal((3, 1, 1001)).astype(np.float32))}
    bench.dump_outputs(str(tmp_path / "a"), 0, 1, t)
    for k, v in t.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(v.shape)
        assert np.array_equal(got, v.float().numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    bench.dump_outputs(str(tmp_path / "b"), 0, 1, t)
    bench.dump_outputs(str(tmp_path / "c"), 1, 2, t)
    total = 0
    for k, v in t.items():
        got = np.load(tmp_path / "b" / f"{k}.npy")
        assert got.dtype == np.float32 and got.ndim == 1 and 0 < got.size < v.numel()
        assert np.isin(got, v.float().numpy()).all()
        assert np.array_equal(got, np.load(tmp_path / "c" / f"{k}_rank1.npy"))
        total += got.nbytes
    assert total <= 4096


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_outputs(tmp_path):
    """A plain run: the headline fields, --steps timed steps, none of the --full
    legs, and the last timed step's outputs as float32 .npy files."""
    import numpy as np
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and "fp32" in line["dtype"]
    assert line["ms_per_step"] > 0
    # value = samples of the timed steps / their wall time (both rounded in the line)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / (16 * 65536) - 1) < 1e-3
    for k in ("roofline", "pipelined", "f32_exact", "split16_auto", "configs", "cpu_baseline"):
        assert line[k] is None, k
    audio = np.load(tmp_path / "out" / "audio.npy")
    latents = np.load(tmp_path / "out" / "latents.npy")
    assert audio.dtype == np.float32 and audio.shape == (16, 1, 65536)
    sys.path.insert(0, REPO)
    from rave_amd import config as rcfg
    cfg = rcfg.v2()
    assert latents.dtype == np.float32 and latents.shape == (16, cfg.dec_in, 65536 // cfg.hop)
    assert np.isfinite(audio).all() and np.isfinite(latents).all() and np.abs(audio).max() > 0


def test_bad_gpu_count_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "0", "--dry-run"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0
