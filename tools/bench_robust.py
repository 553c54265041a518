#!/usr/bin/env python3
"""What a robust loss costs: each energy of energies/robust/ against the same file with plain
Energy terms, at DESIGN §3.6's sizes, fp32, gaussNewtonGPU, lIterations = 10 (for information,
no bar):

* bundle adjustment, 1 000 cameras / 100 000 points / 1 000 000 observations
  (tools/bench_schur.py's problem): energies/robust/bundle_adjustment_huber.t at a = 0.02
  against that file with its RobustEnergy statement written as Energy (block preconditioner
  in both; the unused Param stays, so both take the same problemparams);
* the pose graph, 10^6 poses / 1 998 000 constraints (tools/bench_pose_graph.py's grid world):
  energies/robust/pose_graph_2d_cauchy.t against energies/pose_graph_2d.t.

One process, the two files of a pair interleaved on the same inputs:

* the GN step in ms (host clock around a call that ends in a device synchronise; median of
  --reps after a warm-up step);
* in a pass of its own, the plan's per-kernel timer: the apply in us per PCG iteration
  (`gen_apply`: the timer entry that spans gen_apply and gen_apply_graph), `jtf`, `cost`,
  and `gen_loss_weights` per call with its calls per Init + Step (Init, Step start, after the
  update);
* the share of loss blocks with rho' < 1 at the start (OptAMD_EvalLossWeights) and the bytes
  the weights add: (1 + slots with unknowns) * 4 + 4 * slots per edge;
* the cost after each of --steps GN steps.

    python tools/bench_robust.py [--problems bundle,pose_graph] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("jtf", "gn_init", "blk_init", "step2", "blk_step2", "step3", "gen_apply", "gen_loss_weights", "precompute",
           "update", "cost")


def measure(dims, files, fresh, args, torch, OptSolver, slots_with_unknowns):
    solvers = {}
    for k, f in files.items():
        s = OptSolver(dims, f, "gaussNewtonGPU")
        assert s.family() == "generic"
        s.set_solver_params({"nIterations": args.steps, "lIterations": args.iters})
        solvers[k] = s

    def one_step(s):
        s.init(fresh())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for s in solvers.values():   # warm-up: code objects, incidence lists, inverse positions
        one_step(s)
    times = {k: [] for k in solvers}
    for _ in range(args.reps):   # interleaved
        for k, s in solvers.items():
            times[k].append(one_step(s))
    for k, s in solvers.items():
        out[k] = {"step_ms": sorted(times[k]), "step_ms_median": float(np.median(times[k])),
                  "cost_after_steps": s.profiled_solve(fresh())}
    # the kernel table, in a pass of its own (event pairs around every launch slow the step)
    for k, s in solvers.items():
        s.set_kernel_timing(1)
        for _ in range(3):
            one_step(s)
        table = {}
        for n in KERNELS:
            cnt, ms = s.kernel_stat(n)
            if cnt:
                table[n] = {"launches": cnt, "us_per_launch": 1e3 * ms / cnt}
        s.set_kernel_timing(0)
        out[k]["kernels"] = table
        out[k]["apply_us_per_iteration"] = table.get("gen_apply", {}).get("us_per_launch", 0.0)
    r = solvers["robust"]
    g = r.loss_groups()[0]
    rho1 = r.loss_weights(fresh())
    out["robust"]["loss_group"] = g
    out["robust"]["blocks_with_rho1_below_1"] = float((rho1 < 1).float().mean())
    out["robust"]["weight_bytes_per_edge"] = (1 + slots_with_unknowns) * 4 + 4 * slots_with_unknowns
    lw = out["robust"]["kernels"].get("gen_loss_weights", {})
    out["robust"]["loss_weights_us_per_call"] = lw.get("us_per_launch", 0.0)
    out["robust"]["loss_weights_calls_per_init_and_step"] = lw.get("launches", 0) / 3.0   # Init; Step start, after the update
    out["robust_step_over_plain"] = out["robust"]["step_ms_median"] / out["plain"]["step_ms_median"]
    out["robust_apply_over_plain"] = out["robust"]["apply_us_per_iteration"] / max(out["plain"]["apply_us_per_iteration"], 1e-30)
    for s in solvers.values():
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="bundle,pose_graph")
    ap.add_argument("--cameras", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--per-point", type=int, default=10)
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--huber", type=float, default=0.02)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from opt_amd import OptSolver
    from opt_amd.harness import problems
    if not torch.cuda.is_available():
        sys.exit("bench_robust: no GPU (nothing is measured without one)")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tmp = tempfile.mkdtemp()
    out = {"library": os.environ.get("OPT_AMD_LIB", "in-tree"), "pcg_iterations": args.iters, "precision": "fp32",
           "solver": "gaussNewtonGPU", "device": torch.cuda.get_device_name(0)}
    todo = [p for p in args.problems.split(",") if p]
    if "bundle" in todo:
        from bench_schur import problem
        w = problem(args.cameras, args.points, args.per_point, seed=1)
        robust = os.path.join(ROOT, "energies", "robust", "bundle_adjustment_huber.t")
        text = open(robust).read()
        stmt = 'RobustEnergy("huber", huber, '
        assert text.count(stmt) == 1
        plain = os.path.join(tmp, "bundle_adjustment_block_plain.t")
        open(plain, "w").write(text.replace(stmt, "Energy("))
        consts = [dev(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
        start = [dev(w[k]) for k in ("CamR", "CamT", "X")]

        def fresh():
            return [w["w_cam"], w["w_pt"]] + [u.clone() for u in start] + consts + [float(args.huber)]

        out["bundle"] = dict(cameras=w["NC"], points=w["NP"], observations=w["NO"], huber=args.huber,
                             **measure([w["NC"], w["NP"], w["NO"]], {"plain": plain, "robust": robust}, fresh, args,
                                       torch, OptSolver, slots_with_unknowns=2))
        del w, consts, start
        torch.cuda.empty_cache()
    if "pose_graph" in todo:
        from bench_pose_graph import grid_world
        V, edges, fixed = grid_world(args.side)
        w, dims = problems.pose_graph_2d(V, edges, fixed, w_anchor=10.0)
        del V, edges
        consts = problems.pose_graph_2d_params(w, dev)

        def fresh():
            return [consts[0], consts[1].clone()] + consts[2:]

        files = {"plain": os.path.join(ROOT, "energies", "pose_graph_2d.t"),
                 "robust": os.path.join(ROOT, "energies", "robust", "pose_graph_2d_cauchy.t")}
        out["pose_graph"] = dict(poses=dims[0], constraints=dims[1], cauchy=1.5,
                                 **measure(dims, files, fresh, args, torch, OptSolver, slots_with_unknowns=2))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
