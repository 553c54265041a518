"""OptSolver.covariance at size (for information, no bar): fp32 Gauss-Newton plans on
energies/direct/*_cholesky.t, the bundle problem of tools/bench_schur.py (100 points per camera,
10 observations per point) and the grid-world pose graph of tools/bench_pose_graph.py.

Three selections, interleaved in one process, --alternations times: `all` (every diagonal block),
`last` (the one element at the end of the ordering: one tile column of work) and `first` (the
one at the start: a full-length chain for one tile-row). Per selection: the wall time of the
call in ms, and from the plan's event-pair timer in a pass of its own `cov_fill`, `cov_factor`,
`cov_forward` and `cov_gram` in us per call, beside `dense_factor` of a direct Step of the same
plan; the forward chain's flop rate on its own count (2 * 64^3 per tile product: one diagonal and
nt - k - 1 trailing products per live tile-row and panel); direct_info().

  python tools/bench_covariance.py --problem ba --size 1000 [--alternations 2] [--out FILE]
  python tools/bench_covariance.py --problem pg --size 71
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def forward_flops(n, C, elements):
    """DenseSelection::forward_flops (dense_cholesky.hip) restated."""
    nt, per = -(-n // 64), 64 // C
    e = sorted(set(elements))
    starts = [e[k] * C // 64 for k in range(0, len(e), per)]
    return sum((nt - s) * (nt - s + 1) / 2 for s in starts) * 2.0 * 64 ** 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", choices=("ba", "pg"), required=True)
    ap.add_argument("--size", type=int, required=True, help="cameras, or the side of the pose grid")
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from opt_amd import OptSolver
    if not torch.cuda.is_available():
        sys.exit("bench_covariance: no GPU (nothing is measured without one)")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    if a.problem == "ba":
        from bench_schur import problem
        w = problem(a.size, 100 * a.size, 10, seed=1)
        s = OptSolver([w["NC"], w["NP"], w["NO"]], os.path.join(ROOT, "energies", "direct", "bundle_adjustment_schur_cholesky.t"),
                      "gaussNewtonGPU")
        consts = [dev(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
        start = [dev(w[k]) for k in ("CamR", "CamT", "X")]
        fresh = lambda: [w["w_cam"], w["w_pt"]] + [u.clone() for u in start] + consts  # noqa: E731
        elements, C = w["NC"], 6
    else:
        from bench_pose_graph import grid_world
        from opt_amd.harness import problems
        V, edges, fixed = grid_world(a.size)
        w, dims = problems.pose_graph_2d(V, edges, fixed, w_anchor=10.0)
        s = OptSolver(dims, os.path.join(ROOT, "energies", "direct", "pose_graph_2d_cholesky.t"), "gaussNewtonGPU")
        consts = problems.pose_graph_2d_params(w, dev)
        p0 = consts[1].clone()

        def fresh():
            prm = list(consts)
            prm[1] = p0.clone()
            return prm
        elements, C = a.size * a.size, 3
    s.set_solver_params({"nIterations": 2, "lIterations": 10})
    n = elements * C
    selections = {"all": None, "last": [elements - 1], "first": [0]}
    out = {"problem": a.problem, "size": a.size, "elements": elements, "n": n, "precision": "fp32",
           "device": torch.cuda.get_device_name(0), "alternations": []}

    def stat(names):
        return {k: s.kernel_stat(k) for k in names}

    names = ("cov_fill", "cov_factor", "cov_forward", "cov_gram", "dense_factor")
    prm = fresh()
    s.init(prm)
    s.step()                                                       # warm-up: code objects, the pattern, the tiles
    for sel in selections.values():
        s.covariance(prm, elements=sel)
    for _ in range(a.alternations):
        rec = {}
        for name, sel in selections.items():                      # wall time, interleaved
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.covariance(prm, elements=sel)
            rec[name] = {"call_ms": (time.perf_counter() - t0) * 1e3}
        s.set_kernel_timing(1)
        before = stat(names)
        prm2 = fresh()
        s.init(prm2)
        s.step()
        after = stat(names)
        rec["dense_factor_us"] = 1e3 * (after["dense_factor"][1] - before["dense_factor"][1]) / max(
            1, after["dense_factor"][0] - before["dense_factor"][0])
        for name, sel in selections.items():
            before = stat(names)
            s.covariance(prm, elements=sel)
            after = stat(names)
            for k in names[:4]:
                rec[name][k + "_us"] = 1e3 * (after[k][1] - before[k][1])
            fl = forward_flops(n, C, range(elements) if sel is None else sel)
            rec[name]["forward_flops"] = fl
            rec[name]["forward_TFLOPs"] = fl / (rec[name]["cov_forward_us"] * 1e-6) / 1e12 if rec[name]["cov_forward_us"] else 0.0
        s.set_kernel_timing(0)
        out["alternations"].append(rec)
    out["direct_info"] = {k: (v if not isinstance(v, float) or (v == v and abs(v) != float("inf")) else str(v))
                          for k, v in s.direct_info().items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
