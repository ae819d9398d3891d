"""bench.py launcher plumbing (CPU only): `--gpus N` without a launcher starts N ranks itself,
and a launcher whose WORLD_SIZE disagrees with --gpus is refused.  --dry-run stops every rank
right after the world-size check, before any GPU or model work.  Plus --dump-outputs: the writer on host
tensors, and (GPU) one plain run on a small slide."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(kw)
    return env


def test_gpus_n_spawns_n_ranks():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--dry-run"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(s) for s in p.stdout.splitlines() if s.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1, 2]
    assert all(d["world"] == 3 for d in lines)


def test_world_size_mismatch_is_refused():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"],
                       env=_env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2
    assert "WORLD_SIZE=3" in p.stderr


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """dump_outputs / named_outputs on host tensors: one float32 .npy per returned embedding, named by layer
    (and by slide for the mixed batch), values unchanged."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    out = [torch.full((1, 4), float(k), dtype=torch.bfloat16) for k in range(3)]
    bench.dump_outputs(str(tmp_path / "a"), bench.named_outputs(out, False))
    assert sorted(os.listdir(tmp_path / "a")) == ["embed00.npy", "embed01.npy", "embed02.npy"]
    a = np.load(tmp_path / "a" / "embed02.npy")
    assert a.dtype == np.float32 and a.shape == (1, 4) and (a == 2.0).all()
    bench.dump_outputs(str(tmp_path / "b"), bench.named_outputs([out, out], True), prefix="rank1_")
    assert sorted(os.listdir(tmp_path / "b"))[-1] == "rank1_slide01_embed02.npy" and len(os.listdir(tmp_path / "b")) == 6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) on a 1,024-tile slide: --steps sets the timed steps, the line carries the
    headline keys and none of the --full parts, and --dump-outputs holds the 13 finite [1, 768] embeddings."""
    import numpy as np
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--tiles", "1024",
                        "--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip())
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "tiles/s" and r["dtype"] == "bf16"
    assert r["higher_is_better"] is True and r["ms_per_step"] > 0
    assert abs(r["value"] - 1024 / (r["ms_per_step"] / 1e3)) <= 1e-3 * r["value"]
    for k in ("roofline", "kernel_ms_per_step", "cpu_baseline", "cpu_full_forwards", "c4_256k_same_gpu"):
        assert k not in r
    assert sorted(os.listdir(d)) == ["embed%02d.npy" % k for k in range(13)]
    for f in os.listdir(d):
        a = np.load(d / f)
        assert a.dtype == np.float32 and a.shape == (1, 768) and np.isfinite(a).all()


def test_single_gpu_runs_in_process():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run"], env=_env(), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip()) == {"rank": 0, "world": 1}
