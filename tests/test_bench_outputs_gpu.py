"""GPU: bench.py's plain run, --dump-outputs and --full, at a small size.

A plain run reports the headline only (no figure that takes runs of its own);
--dump-outputs writes what the last timed step left — the unknown arrays the Steps update
in place and the cost — which must equal what the same number of Steps gives through
OptSolver on the same seeded inputs; --full adds the roofline and per-kernel figures to the
same headline fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SIZE, STEPS, WARMUP, LITER = 160, 3, 1, 10
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "init_kernel", "step_kernels", "pure_apply_us", "apply_unknowns_per_s", "cpu_baseline")


def run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--size", str(SIZE), "--steps", str(STEPS),
                        "--warmup", str(WARMUP)] + extra, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    (line,) = [x for x in p.stdout.splitlines() if x.startswith("{")]
    return json.loads(line)


@pytest.mark.gpu
def test_plain_run_dumps_what_the_steps_computed(tmp_path):
    import torch

    from opt_amd import OptSolver, workloads

    out = tmp_path / "dump"
    r = run(["--dump-outputs", str(out)])
    assert all(k in r for k in HEADLINE) and not any(k in r for k in FULL_ONLY)
    assert r["steps"] == STEPS and r["warmup"] == WARMUP and r["unit"] == "unknowns/s" and r["dtype"] == "f32"
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(3 * SIZE * SIZE * LITER / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert sorted(os.listdir(out)) == ["Angle.npy", "Offset.npy", "cost.npy"]
    got = {k: np.load(out / (k + ".npy")) for k in ("Offset", "Angle", "cost")}
    assert got["Offset"].dtype == np.float32 and got["Offset"].shape == (2 * SIZE * SIZE,)
    assert got["Angle"].dtype == np.float32 and got["Angle"].shape == (SIZE * SIZE,)
    assert got["cost"].dtype == np.float64 and got["cost"].shape == (1,)
    # the same seeded inputs, WARMUP + STEPS Steps through the solver
    w = workloads.image_warping(SIZE, SIZE, seed=1234)
    prm = [torch.from_numpy(w[k]).cuda() for k in ("Offset", "Angle", "UrShape", "Constraints", "Mask")] + \
          [w["w_fitSqrt"], w["w_regSqrt"]]
    s = OptSolver([SIZE, SIZE], os.path.join(ROOT, "energies", "image_warping.t"), "gaussNewtonGPU")
    s.set_solver_params({"nIterations": WARMUP + 2 * STEPS + 1, "lIterations": LITER})
    s.init(prm)
    for _ in range(WARMUP + STEPS):
        s.step()
    torch.cuda.synchronize()
    assert np.array_equal(got["Offset"], prm[0].cpu().numpy())
    assert np.array_equal(got["Angle"], prm[1].cpu().numpy())
    assert got["cost"][0] == s.cost()
    assert not np.array_equal(got["Offset"], w["Offset"])   # the Steps moved the unknowns


@pytest.mark.gpu
def test_full_run_adds_the_kernel_figures():
    r = run(["--full", "--no-cpu-baseline"])
    assert all(k in r for k in HEADLINE)
    assert r["roofline"]["launches"] > 0 and r["roofline"]["avg_us"] > 0
    assert r["init_kernel"]["launches"] == STEPS and r["pure_apply_us"] > 0
    assert set(r["step_kernels"]) <= {"iw_jtf_apply", "iw_pcg", "iw_update", "iw_cost"} and r["step_kernels"]
    assert "cpu_baseline" not in r
