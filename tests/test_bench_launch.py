"""bench.py's multi-rank launch: ``python bench.py --gpus N``
without a torch.distributed environment starts N ranks itself (a
torch.distributed.run child process) and the line reports the N ranks the
all-reduce saw (CPU only: --dry-run with the gloo backend); and what a plain
run prints and ``--dump-outputs`` writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_spawns_two_ranks():
    out = _run("--gpus", "2", "--backend", "gloo", "--dry-run", "--steps", "5", "--warmup", "1")
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["steps"] == 5


def test_bench_single_rank_dry_run():
    out = _run("--dry-run", "--steps", "3", "--warmup", "1")
    assert out["n_gpus"] == 1 and out["ranks_seen"] == 1


def test_bench_dry_run_dumps_outputs(tmp_path):
    out = _run("--dry-run", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "d"))
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    x = np.load(tmp_path / "d" / "x.npy")
    assert x.dtype == np.float32
    np.testing.assert_allclose(x, np.float32(1.0001) ** 3, rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_bench_plain_run_and_dump(cuda, tmp_path, det):
    """A plain run times --steps steps, reports ms_per_step, leaves the --full
    blocks out and dumps what the last step returned, the loss and PSNR of the
    line; with --deterministic also the parameters that step updated (which
    moved from the bench's seeded init)."""
    line = _run("--steps", "3", "--warmup", "1", "--settle", "4", "--splats", "2000",
                "--dump-outputs", str(tmp_path), *(["--deterministic"] if det else []))
    assert line["steps"] == 3 and line["unit"] == "train-iters/s" and line["dtype"] == "f32"
    assert line["ms_per_step"] == pytest.approx(1e3 / line["value"], rel=1e-2)
    assert line["train_iter_path"].startswith("fused")
    for k in ("roofline", "kernels", "shape", "render", "op_path", "alpha", "config0_cpu"):
        assert k not in line
    params = ["xyz", "cholesky", "features_dc"] if det else []
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(n + ".npy" for n in ["loss", "psnr"] + params)
    z = {n: np.load(tmp_path / (n + ".npy")) for n in ["loss", "psnr"] + params}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in z.values())
    assert float(z["psnr"]) == pytest.approx(line["psnr_after_iters"], abs=1e-5)
    assert float(z["psnr"]) == pytest.approx(10 * np.log10(1.0 / float(z["loss"])), abs=1e-4)
    if det:
        # the seeded init (make_frame_model seed 1000), 8 Adan steps of lr 1e-3 on:
        # moved, and by far less than two draws of the init differ (O(1))
        from gsvc_amd.frame import make_frame_model
        init = make_frame_model(1080, 1920, 2000, "cpu", seed=1000)
        for n in params:
            p = getattr(init, "_features_dc" if n == "features_dc" else "_" + n).detach().numpy()
            assert z[n].shape == p.shape and 0 < np.abs(z[n] - p).max() < 0.1, n
