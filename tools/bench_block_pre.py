#!/usr/bin/env python3
"""Block-Jacobi against the scalar preconditioner on a synthetic bundle problem.

Builds about 2048 cameras, 200 k points and 8 observations per point (every camera's
incidence list stays at a few hundred edges: the graph gather walks one list per lane), and
runs ONE Gauss-Newton step of 30 PCG iterations with energies/bundle_adjustment.t and with
its UsePreconditioner("block") variant: same inputs, one process, the runs interleaved.

Records, per variant: the rz history of the step (r.M^-1 r, each with its own M), the
iterations needed to reduce rz by 1e4, the wall time of the step (host clock around a call
that ends in a device synchronise, median of --reps after a warm-up step), and from a
separate pass with the plan's per-kernel timer (OptAMD_KernelReport) the time of the
preconditioner kernels (gn_init + step2 against gn_init + blk_init + blk_step2) next to the
gather (gen_apply). Prints one JSON object and writes it to --out.

    python tools/bench_block_pre.py --out profiles/block_pre.json
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
SC_BASE, SC_SLOTS = 8, 7   # stencil_plan.h: rz_i at kScBase + kSlots * i


def rot(ang):
    a, b, g = ang[:, 0], ang[:, 1], ang[:, 2]
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    return np.stack([cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                     sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca,
                     -sb, cb * sa, cb * ca], -1).reshape(-1, 3, 3)


def problem(NC, NP, per_point, seed):
    """Points in the unit cube seen from cameras near (0, 0, 5); each point by `per_point`
    distinct cameras out of a window of 32 consecutive ones."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (NP, 3))
    R = rng.normal(0, 0.15, (NC, 3))
    T = np.array([0, 0, 5.0]) + rng.normal(0, 0.3, (NC, 3))
    off = np.argsort(rng.random((NP, 32)), 1)[:, :per_point]
    cam = ((rng.integers(0, NC, NP)[:, None] + off) % NC).reshape(-1)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=2048)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--per-point", type=int, default=8)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--double", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from opt_amd import OptSolver
    if not torch.cuda.is_available():
        sys.exit("bench_block_pre: no GPU (nothing is measured without one)")
    w = problem(args.cameras, args.points, args.per_point, seed=1)
    shipped = os.path.join(ROOT, "energies", "bundle_adjustment.t")
    text = open(shipped).read()
    assert "UsePreconditioner(true)" in text
    tmp = tempfile.mkdtemp()
    block = os.path.join(tmp, "bundle_adjustment_block.t")
    open(block, "w").write(text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))

    T = np.float64 if args.double else np.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    consts = [dev(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
    start = [dev(w[k].astype(T)) for k in ("CamR", "CamT", "X")]

    def fresh():
        unk = [u.clone() for u in start]
        return [w["w_cam"], w["w_pt"]] + unk + consts

    solvers = {}
    for name, path in (("scalar", shipped), ("block", block)):
        s = OptSolver([w["NC"], w["NP"], w["NO"]], path, "gaussNewtonGPU", double_precision=args.double)
        s.set_solver_params({"nIterations": 1, "lIterations": args.iters})
        solvers[name] = s

    def one_step(s):
        prm = fresh()
        s.init(prm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.step()
        return (time.perf_counter() - t0) * 1e3

    out = {"cameras": w["NC"], "points": w["NP"], "observations": w["NO"], "max_edges_per_camera": w["max_cam_edges"],
           "pcg_iterations": args.iters, "precision": "fp64" if args.double else "fp32", "device": torch.cuda.get_device_name(0)}
    for s in solvers.values():   # warm-up: code objects, incidence lists
        one_step(s)
    times = {k: [] for k in solvers}
    for _ in range(args.reps):   # interleaved
        for k, s in solvers.items():
            times[k].append(one_step(s))
    for k, s in solvers.items():
        sc = s.scalars(SC_BASE + SC_SLOTS * (args.iters + 2))
        rz = [sc[SC_BASE + SC_SLOTS * i] for i in range(args.iters + 1)]
        hit = [i for i, v in enumerate(rz) if v <= 1e-4 * rz[0]]
        out[k] = {"rz": rz, "iterations_to_1e-4": hit[0] if hit else None, "cost_after_step": s.cost(),
                  "step_ms": sorted(times[k]), "step_ms_median": float(np.median(times[k]))}
    # the kernel table, in a pass of its own (event pairs around every launch slow the step)
    for k, s in solvers.items():
        s.set_kernel_timing(1)
        for _ in range(3):
            one_step(s)
        names = ["jtf", "gn_init", "step2", "step3", "gen_apply", "blk_init", "blk_step2", "update", "cost", "precompute"]
        table = {}
        for n in names:
            cnt, ms = s.kernel_stat(n)
            if cnt:
                table[n] = {"launches": cnt, "us_per_launch": 1e3 * ms / cnt}
        s.set_kernel_timing(0)
        out[k]["kernels"] = table
    ks, kb = out["scalar"]["kernels"], out["block"]["kernels"]
    us = lambda t, n: t.get(n, {}).get("us_per_launch", 0.0)
    it_s = us(ks, "gen_apply") + us(ks, "step2") + us(ks, "step3")
    it_b = us(kb, "gen_apply") + us(kb, "blk_step2") + us(kb, "step3")
    setup_s = us(ks, "jtf") + us(ks, "gn_init")
    setup_b = us(kb, "jtf") + us(kb, "gn_init") + us(kb, "blk_init")
    out["per_iteration_us"] = {"scalar": it_s, "block": it_b}
    out["setup_us"] = {"scalar": setup_s, "block": setup_b}
    out["preconditioner_share_of_iteration"] = {"scalar": us(ks, "step2") / it_s if it_s else None,
                                                "block": us(kb, "blk_step2") / it_b if it_b else None}
    # block pays once the iterations it saves cost more than its dearer set-up and iterations:
    # setup_b + k_b it_b < setup_s + k_s it_s; with k_b = k_s - saved: saved > this many
    k_s = out["scalar"]["iterations_to_1e-4"] or args.iters
    if it_b:
        out["break_even_iterations_saved"] = ((setup_b - setup_s) + k_s * (it_b - it_s)) / it_b
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
