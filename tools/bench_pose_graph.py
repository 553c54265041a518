"""A synthetic grid-world 2-D pose graph at size on energies/pose_graph_2d.t (for information,
no bar): S x S poses on a unit grid, a constraint from every pose to its right and to its
upper neighbour (about 2 S^2), noisy measurements, random SPD information matrices, start
poses off the truth with headings on different turns. fp32 Gauss-Newton steps with
--iters PCG iterations: the wall time of one step and the plan's kernel table.

The plan's table names the passes, not the kernels: `gen_apply` is one J^T J p (the prior's
gen_apply and the constraints' gen_apply_graph together), `jtf` one J^T F with the
preconditioner (gen_jtf and gen_jtf_graph together).

  python tools/bench_pose_graph.py [--side 1000] [--iters 10] [--reps 5] [--out FILE]

--variants scalar,block,explicit instead runs, in one process and interleaved, the shipped file,
its UsePreconditioner("block") variant and energies/normal_matrix/pose_graph_2d_explicit.t
(NormalMatrix("explicit")) on the same inputs: the GN step in ms (median of --reps after a
warm-up), then in a pass of its own the plan's per-kernel timer — the apply in us per PCG
iteration (`normal_spmv` for the explicit form, `gen_apply` for the others), `normal_eblk` and
`normal_assemble` per step — the host symbolic phase in ms, the shape and bytes of H, the SpMV's
bytes (values, column indices, row pointers, p gathered once per block, Ap) over its time against
the 6.29 TB/s float4 copy rate, and the cost after each of 5 GN steps. A library from before the
statement (OPT_AMD_LIB) knows only scalar and block. The `cholesky` variant
(energies/direct/pose_graph_2d_cholesky.t) is the direct step: its table adds `dense_fill`,
`dense_factor`, `dense_solve`, the factorisation's flop rate on n^3 / 3 and direct_info() (at a
size whose dense storage does not fit: the memory fall-back, and the explicit plan's Step).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from opt_amd import OptSolver  # noqa: E402
from opt_amd.harness import problems  # noqa: E402


def grid_world(S, seed=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    N = S * S
    truth = np.stack([xx.reshape(-1), yy.reshape(-1), rng.uniform(-np.pi, np.pi, N)], 1).astype(np.float64)
    idx = (xx + S * yy)
    i = np.concatenate([idx[:, :-1].reshape(-1), idx[:-1, :].reshape(-1)])
    j = np.concatenate([idx[:, 1:].reshape(-1), idx[1:, :].reshape(-1)])
    order = rng.permutation(len(i))
    i, j = i[order], j[order]
    E = len(i)
    c, s = np.cos(truth[i, 2]), np.sin(truth[i, 2])
    dt = truth[j, :2] - truth[i, :2]
    dth = truth[j, 2] - truth[i, 2]
    z = np.stack([c * dt[:, 0] + s * dt[:, 1], -s * dt[:, 0] + c * dt[:, 1], np.arctan2(np.sin(dth), np.cos(dth))], 1)
    z += rng.normal(0, 1, (E, 3)) * [0.02, 0.02, 0.01]
    B = rng.normal(0, 1, (E, 3, 3))
    info = 4.0 * (np.einsum("eab,ecb->eac", B, B) + 2.0 * np.eye(3))
    V = truth + rng.normal(0, 1, (N, 3)) * [0.1, 0.1, 0.08]
    V[:, 2] += 2 * np.pi * rng.integers(-1, 2, N)
    return V, (np.stack([i, j], 1), z, info), [0]


def run_variants(a):
    import tempfile
    V, edges, fixed = grid_world(a.side)
    w, dims = problems.pose_graph_2d(V, edges, fixed, w_anchor=10.0)
    del V, edges
    shipped = os.path.join(ROOT, "energies", "pose_graph_2d.t")
    text = open(shipped).read()
    assert "UsePreconditioner(true)" in text
    block = os.path.join(tempfile.mkdtemp(), "pose_graph_2d_block.t")
    open(block, "w").write(text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    files = {"scalar": shipped, "block": block,
             "explicit": os.path.join(ROOT, "energies", "normal_matrix", "pose_graph_2d_explicit.t"),
             "cholesky": os.path.join(ROOT, "energies", "direct", "pose_graph_2d_cholesky.t")}
    names = [v for v in a.variants.split(",") if v]
    cuda = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    consts = problems.pose_graph_2d_params(w, cuda)

    def fresh():
        return [consts[0], consts[1].clone()] + consts[2:]

    solvers = {}
    for name in names:
        s = OptSolver(dims, files[name], "gaussNewtonGPU")
        assert s.family() == "generic"
        s.set_solver_params({"nIterations": a.steps, "lIterations": a.iters})
        solvers[name] = s

    def one_step(s):
        s.init(fresh())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"library": os.environ.get("OPT_AMD_LIB", "in-tree"), "poses": dims[0], "constraints": dims[1],
           "pcg_iterations": a.iters, "precision": "fp32", "solver": "gaussNewtonGPU",
           "device": torch.cuda.get_device_name(0)}
    for s in solvers.values():   # warm-up: code objects, incidence lists, the pattern
        one_step(s)
    times = {k: [] for k in solvers}
    for _ in range(a.reps):      # interleaved
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
        for n in ("jtf", "gn_init", "blk_init", "step2", "blk_step2", "step3", "gen_apply", "normal_eblk", "normal_assemble",
                  "normal_spmv", "dense_fill", "dense_factor", "dense_solve", "update", "cost"):
            cnt, ms = s.kernel_stat(n)
            if cnt:
                table[n] = {"launches": cnt, "us_per_launch": 1e3 * ms / cnt}
        s.set_kernel_timing(0)
        out[k]["kernels"] = table
        out[k]["apply_us_per_iteration"] = table.get("normal_spmv" if k in ("explicit", "cholesky") else "gen_apply", {}).get("us_per_launch", 0.0)
        if k == "cholesky":
            n, f = 3 * dims[0], table.get("dense_factor", {}).get("us_per_launch", 0.0)
            # (min_pivot_ratio is inf before the first factorisation: a string, so the record stays JSON)
            out[k]["direct_info"] = {a: (v if v == v and abs(v) != float("inf") else str(v)) if isinstance(v, float) else v
                                     for a, v in s.direct_info().items()}
            out[k]["factor_TFLOPs"] = n ** 3 / 3 / (f * 1e-6) / 1e12 if f else 0.0
    if "explicit" in solvers:
        # the symbolic phase alone: a fresh plan, its incidence lists built by a cost evaluation
        # first, then the bind-and-pattern call (OptAMD_NormalMatrix without arrays)
        from opt_amd.api import ParamPack
        s2 = OptSolver(dims, files["explicit"], "gaussNewtonGPU")
        prm = fresh()
        s2.eval_cost(prm)
        pk = ParamPack(prm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = s2.lib.OptAMD_NormalMatrix(s2.plan, pk.ptr, None, None, None)
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        rows, dim, nnzb = s2.normal_matrix_shape()
        e = out["explicit"]
        e["symbolic_build_ms"] = ms
        if hasattr(s2.lib, "OptAMD_PlanSymbolicInfo"):   # (a library from before the device builder has none)
            info = dict(kv.split("=") for kv in s2.symbolic_info().split())
            e["symbolic_path"], e["symbolic_transient_bytes"] = info["path"], int(info["transient_bytes"])
        e["block_rows"], e["block_dim"], e["blocks"] = rows, dim, nnzb
        e["matrix_bytes"] = nnzb * dim * dim * 4
        # what one SpMV moves: values, column indices, row pointers, p once per block, Ap and p once per row
        e["spmv_bytes"] = nnzb * dim * dim * 4 + nnzb * 4 + (rows + 1) * 4 + nnzb * dim * 4 + 2 * rows * dim * 4
        spmv = e["kernels"].get("normal_spmv", {}).get("us_per_launch", 0.0)
        e["spmv_TB_per_s"] = e["spmv_bytes"] / (spmv * 1e-6) / 1e12 if spmv else 0.0
        e["spmv_over_copy_rate"] = e["spmv_TB_per_s"] / 6.29   # the float4 copy rate measured on this chip
        s2.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--variants", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.variants:
        return run_variants(a)
    V, edges, fixed = grid_world(a.side)
    w, dims = problems.pose_graph_2d(V, edges, fixed, w_anchor=10.0)
    del V, edges
    cuda = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    s = OptSolver(dims, os.path.join(ROOT, "energies", "pose_graph_2d.t"), "gaussNewtonGPU")
    assert s.family() == "generic"
    s.set_solver_params({"nIterations": 1, "lIterations": a.iters})

    def one_step():
        prm = problems.pose_graph_2d_params(w, cuda)
        s.init(prm)
        c0 = s.cost()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, c0, s.cost()

    one_step()   # warm-up: code object, incidence lists
    runs = [one_step() for _ in range(a.reps)]
    out = {"poses": dims[0], "constraints": dims[1], "pcg_iterations": a.iters, "precision": "fp32",
           "solver": "gaussNewtonGPU", "device": torch.cuda.get_device_name(0),
           "step_ms": sorted(r[0] for r in runs), "step_ms_median": float(np.median([r[0] for r in runs])),
           "cost_before": runs[0][1], "cost_after_step": runs[0][2]}
    # the kernel table, in a pass of its own (event pairs around every launch slow the step)
    s.set_kernel_timing(1)
    for _ in range(3):
        one_step()
    table = {}
    for n in ("jtf", "gn_init", "gen_apply", "step2", "step3", "update", "cost", "precompute"):
        cnt, ms = s.kernel_stat(n)
        if cnt:
            table[n] = {"launches": cnt, "us_per_launch": 1e3 * ms / cnt}
    out["kernels"] = table
    out["kernel_report"] = s.kernel_report().splitlines()
    s.set_kernel_timing(0)
    print(json.dumps({k: v for k, v in out.items() if k != "kernel_report"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
