#!/usr/bin/env python3
"""Schur-complement PCG (Eliminate(X)), matrix-free and explicitly formed
(ReducedSystem("explicit")), against the scalar and block preconditioners on
bundle adjustment at DESIGN §3.6's size: 1 000 cameras, 100 000 points, 1 000 000
observations (10 distinct random cameras per point), fp32, gaussNewtonGPU.

One process, the variants interleaved (energies/bundle_adjustment.t, its
UsePreconditioner("block") variant, energies/bundle_adjustment_schur.t and
energies/bundle_adjustment_schur_explicit.t; same inputs):

* the GN step in ms at lIterations = 10 (host clock around a call that ends in a device
  synchronise; median of --reps after a warm-up step);
* the apply in us per PCG iteration from the plan's per-kernel timer, in a pass of its own:
  `schur_elim` + `schur_apply` for Schur, `schur_spmv` for the explicit form, `gen_apply` (the
  timer entry that spans gen_apply and gen_apply_graph) for the others; with them the
  once-per-step `schur_rhs` / `schur_back` and the explicit form's `schur_eblk` /
  `schur_assemble`;
* explicit: the host symbolic phase in ms (a fresh plan whose incidence lists are built, then
  the pattern alone), the shape of S, and the SpMV's bytes (blocks x C^2 x 4) over its time;
* the cost after each of 5 GN steps at lIterations = 10.

The `cholesky` variant (energies/direct/bundle_adjustment_schur_cholesky.t, not in the default
set: --variants explicit,cholesky) is the direct step: its table adds `dense_fill`,
`dense_factor`, `dense_solve`, the factorisation's flop rate on n^3 / 3 and direct_info().

--variants picks a subset (a library from before the statement knows no Schur file: run it
with OPT_AMD_LIB and --variants scalar,block to alternate two builds in one session).
--design-table prints the markdown rows for DESIGN §3.6 from the JSON files given.

    python tools/bench_schur.py --out profiles/schur.json
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


def rot(ang):
    a, b, g = ang[:, 0], ang[:, 1], ang[:, 2]
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    return np.stack([cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                     sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca,
                     -sb, cb * sa, cb * ca], -1).reshape(-1, 3, 3)


def problem(NC, NP, per_point, seed):
    """Points in the unit cube seen from cameras near (0, 0, 5); each point by `per_point`
    distinct cameras drawn from all of them (the geometry of the tests' bundle())."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (NP, 3))
    R = rng.normal(0, 0.15, (NC, 3))
    T = np.array([0, 0, 5.0]) + rng.normal(0, 0.3, (NC, 3))
    cam = rng.integers(0, NC, (NP, per_point))
    while True:   # redraw the rows that name a camera twice
        s = np.sort(cam, 1)
        dup = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(1))
        if not len(dup):
            break
        cam[dup] = rng.integers(0, NC, (len(dup), per_point))
    cam = cam.reshape(-1)
    pt = np.repeat(np.arange(NP), per_point)
    order = rng.permutation(len(cam))
    cam, pt = cam[order].astype(np.int32), pt[order].astype(np.int32)
    NO = len(cam)
    q = np.einsum("nij,nj->ni", rot(R)[cam], X[pt]) + T[cam]
    Obs = q[:, :2] / q[:, 2:3] + rng.normal(0, 1e-3, (NO, 2))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(NC=NC, NP=NP, NO=NO, c=cam, p=pt, o=np.arange(NO, dtype=np.int32), Obs=f32(Obs), w_cam=0.1, w_pt=0.1,
                CamR=f32(R + rng.normal(0, 0.02, R.shape)), CamT=f32(T + rng.normal(0, 0.05, T.shape)),
                X=f32(X + rng.normal(0, 0.05, X.shape)), max_cam_edges=int(np.bincount(cam, minlength=NC).max()))


def design_table(paths):
    runs = [json.load(open(p)) for p in paths]
    print("| run | variant | GN step ms | apply us / PCG iteration | cost after GN steps 1..5 |")
    print("|---|---|---|---|---|")
    for p, r in zip(paths, runs):
        for v in ("scalar", "block", "schur", "explicit", "cholesky"):
            if v in r:
                print("| %s | %s | %.2f | %.0f | %s |" % (os.path.basename(p), v, r[v]["step_ms_median"], r[v]["apply_us_per_iteration"],
                                                      " ".join("%.5g" % c for c in r[v]["cost_after_steps"][1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--per-point", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--variants", default="scalar,block,schur,explicit")
    ap.add_argument("--out", default="")
    ap.add_argument("--design-table", nargs="+", default=None)
    args = ap.parse_args()
    if args.design_table:
        return design_table(args.design_table)

    import torch
    from opt_amd import OptSolver
    if not torch.cuda.is_available():
        sys.exit("bench_schur: no GPU (nothing is measured without one)")
    w = problem(args.cameras, args.points, args.per_point, seed=1)
    shipped = os.path.join(ROOT, "energies", "bundle_adjustment.t")
    text = open(shipped).read()
    assert "UsePreconditioner(true)" in text
    block = os.path.join(tempfile.mkdtemp(), "bundle_adjustment_block.t")
    open(block, "w").write(text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    files = {"scalar": shipped, "block": block, "schur": os.path.join(ROOT, "energies", "bundle_adjustment_schur.t"),
             "explicit": os.path.join(ROOT, "energies", "bundle_adjustment_schur_explicit.t"),
             "cholesky": os.path.join(ROOT, "energies", "direct", "bundle_adjustment_schur_cholesky.t")}
    names = [v for v in args.variants.split(",") if v]

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    consts = [dev(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
    start = [dev(w[k]) for k in ("CamR", "CamT", "X")]

    def fresh():
        return [w["w_cam"], w["w_pt"]] + [u.clone() for u in start] + consts

    solvers = {}
    for name in names:
        s = OptSolver([w["NC"], w["NP"], w["NO"]], files[name], "gaussNewtonGPU")
        s.set_solver_params({"nIterations": args.steps, "lIterations": args.iters})
        solvers[name] = s

    def one_step(s):
        s.init(fresh())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.step()
        return (time.perf_counter() - t0) * 1e3

    out = {"library": os.environ.get("OPT_AMD_LIB", "in-tree"), "cameras": w["NC"], "points": w["NP"], "observations": w["NO"],
           "max_edges_per_camera": w["max_cam_edges"], "pcg_iterations": args.iters, "precision": "fp32",
           "device": torch.cuda.get_device_name(0)}
    for s in solvers.values():   # warm-up: code objects, incidence lists
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
        for n in ("jtf", "gn_init", "blk_init", "step2", "blk_step2", "step3", "gen_apply", "schur_rhs", "schur_elim",
                  "schur_apply", "schur_back", "schur_eblk", "schur_assemble", "schur_spmv", "dense_fill", "dense_factor",
                  "dense_solve", "update", "cost"):
            cnt, ms = s.kernel_stat(n)
            if cnt:
                table[n] = {"launches": cnt, "us_per_launch": 1e3 * ms / cnt}
        s.set_kernel_timing(0)
        us = lambda n: table.get(n, {}).get("us_per_launch", 0.0)
        out[k]["kernels"] = table
        out[k]["apply_us_per_iteration"] = (us("schur_elim") + us("schur_apply") if k == "schur" else
                                            us("schur_spmv") if k == "explicit" else 0.0 if k == "cholesky" else us("gen_apply"))
        if k == "cholesky":
            n = 6 * w["NC"]
            # (min_pivot_ratio is inf before the first factorisation: a string, so the record stays JSON)
            out[k]["direct_info"] = {a: (v if v == v and abs(v) != float("inf") else str(v)) if isinstance(v, float) else v
                                     for a, v in s.direct_info().items()}
            out[k]["factor_TFLOPs"] = n ** 3 / 3 / (us("dense_factor") * 1e-6) / 1e12 if us("dense_factor") else 0.0
    if "explicit" in solvers:
        # the symbolic phase alone: a fresh plan, its incidence lists built by a cost evaluation
        # first, then the bind-and-pattern call (OptAMD_ReducedMatrix without arrays)
        from opt_amd.api import ParamPack
        s2 = OptSolver([w["NC"], w["NP"], w["NO"]], files["explicit"], "gaussNewtonGPU")
        prm = fresh()
        s2.eval_cost(prm)
        pk = ParamPack(prm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = s2.lib.OptAMD_ReducedMatrix(s2.plan, pk.ptr, None, None, None)
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        rows, dim, nnzb = s2.reduced_matrix_shape()
        e = out["explicit"]
        e["symbolic_build_ms"] = ms
        if hasattr(s2.lib, "OptAMD_PlanSymbolicInfo"):   # (a library from before the device builder has none)
            info = dict(kv.split("=") for kv in s2.symbolic_info().split())
            e["symbolic_path"], e["symbolic_transient_bytes"] = info["path"], int(info["transient_bytes"])
        e["block_rows"], e["block_dim"], e["blocks"] = rows, dim, nnzb
        e["spmv_bytes"] = nnzb * dim * dim * 4
        spmv = e["kernels"].get("schur_spmv", {}).get("us_per_launch", 0.0)
        e["spmv_TB_per_s"] = e["spmv_bytes"] / (spmv * 1e-6) / 1e12 if spmv else 0.0
        e["spmv_over_copy_rate"] = e["spmv_TB_per_s"] / 6.29   # the float4 copy rate measured on this chip
        s2.close()
    if "schur" in out and "explicit" in out:
        out["explicit_apply_over_schur_apply"] = out["explicit"]["apply_us_per_iteration"] / out["schur"]["apply_us_per_iteration"]
    if "schur" in out and "scalar" in out:
        out["schur_apply_over_full_apply"] = out["schur"]["apply_us_per_iteration"] / out["scalar"]["apply_us_per_iteration"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
