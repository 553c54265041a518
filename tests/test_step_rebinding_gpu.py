"""The Step-boundary contract on every family: a caller may rewrite or rebind any bound
array (the unknowns included) and change any scalar parameter between two
Opt_ProblemStep calls (Opt.h:64-65; the reference re-reads every pointer at each Step),
so whatever a plan derives from the bound arrays and keeps for itself must be rebuilt
from the arrays bound at THIS Step (stencil_plan.h, HasRefreshCaches). ComputedArrays
alone keep the reference's schedule (Init, after update, after revert).

One table-driven test: init, then four GN steps of 10 PCG iterations with a deterministic
mutation before steps 1, 2 and 3 (step 0 runs on the arrays as initialised), against the C
oracle replaying the same mutations one GN step at a time (oracle.<family>_solve(w, 1,
lit), unknowns fed back). `in_place` rewrites the bound tensors (every data_ptr() is the
same at the end); `rebind` passes fresh copies of EVERY array, the unknowns included, at
each mutated step.

Bars. fp64 rows: the family's own fp64 solve-vs-oracle bars for an unmutated solve. fp32
rows: the family's fp32 solve bars, or, where larger, twice the oracle's own shift when
the unknowns are perturbed by one ulp (relative, two seeds, the larger) — the fp32 noise
floor of the replay, as tests/test_image_warping_gpu.py::
test_in_place_updates_between_steps_match_oracle computes it. optical_flow starts at
X = 0, where a relative perturbation changes nothing; there the perturbation is applied
to the unknowns the oracle returns from step 0 (the first point at which it is one), so
step 0 itself is held to the fixed fp32 bar.

That a path ignoring a mutation cannot pass is asserted from the oracle alone: the replay
without the mutations differs from the replay with them by at least 1e-2 relative in the
cost of every step after the first mutation.

Materialized plans (useMaterializedJTJ, with and without useFusedJTJ) run the ARAP row in
fp64 as well: its mutation before step 2 re-wires v0 / v1, which changes the column
structure of J and with it every pattern csr.h derives from J (StencilPlan::materialize
rebuilds them when the Op's topology generation moves). Those rows first run the unmutated
solve against the unmutated replay at the same bars, as a control of the path itself.

shape_from_shading: only w_p / w_s / w_g, edgeMaskR / edgeMaskC and the values of D_i
where it is already > 0 (kept > 0) are mutated — weights before step 1, edge masks before
step 2, D_i before step 3. X, Im, the signs of D_i, f_*, u_* and L_* feed the ComputedArrays
B_I and valid, which by contract are NOT refreshed at Step start: a change to those between
Steps is not seen until the next update, while the one-step oracle replay recomputes them,
so the two would disagree for a reason that is no defect."""
import functools
import os

import numpy as np
import pytest

from opt_amd import OptSolver, workloads
from oracle import oracle
from tests import test_arap_gpu as arap_t
from tests import test_optical_flow_gpu as of_t
from tests import test_poisson_gpu as pie_t
from tests import test_sfs_gpu as sfs_t
from tests.iw_helpers import ROOT, rel_err

pytestmark = pytest.mark.gpu
NSTEPS, LIT = 4, 10
MOVED = 1e-2   # least relative change of every post-mutation cost, mutated vs unmutated replay


def E(name):
    return os.path.join(ROOT, "energies", name + ".t")


# A mutation is a list of (key, "add" | "set", value): the same list drives the oracle's
# numpy dict and the solver's parameter list. Scalars are only ever "set".


# ------------------------------------------------------------------------ optical_flow
class OpticalFlow:
    name, energy, family = "optical_flow", E("optical_flow"), "optical_flow"
    unknowns = ["X"]
    index = {"w_fitSqrt": 0, "w_regSqrt": 1, "X": 2, "I": 3, "I_hat": 4, "I_hat_dx": 5, "I_hat_dy": 6}
    # fp32 / fp64 bars of tests/test_optical_flow_gpu.py::test_solve_matches_oracle
    cost_tol = {False: 2e-5, True: 1e-8}
    unk_tol = {False: {"X": 1e-4}, True: {"X": 1e-7}}

    def __init__(self, W, H):
        self.W, self.H, self.dims = W, H, [W, H]

    def base(self):
        return workloads.optical_flow(self.W, self.H, seed=8, sigma=5.0, max_flow=0.5)

    def mutation(self, k, w):
        W, H = self.W, self.H
        ops = []
        if k in (1, 3):
            ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
            d = np.stack([np.sin(2 * np.pi * (xs / W + 0.1 * k)), np.cos(2 * np.pi * (ys / H + 0.2 * k))], -1)
            ops.append(("X", "add", (0.25 * d).astype(np.float32).reshape(-1)))
        if k == 2:
            w2 = workloads.optical_flow(W, H, seed=8, sigma=5.0, max_flow=1.0)
            ops += [(key, "set", w2[key]) for key in ("I_hat", "I_hat_dx", "I_hat_dy")]
        if k == 3:
            ops.append(("w_fitSqrt", "set", float(np.float32(1.5 * w["w_fitSqrt"]))))
        return ops

    def params(self, w, double, host=False):
        return of_t.params(w, double, host=host)

    def oracle_step(self, w, double):
        X, c = oracle.of_solve(w, 1, LIT, double=double)
        w["X"] = X
        return c[1]


# --------------------------------------------------------------- poisson_image_editing
class Poisson:
    name, energy, family = "poisson", E("poisson_image_editing"), "poisson_image_editing"
    unknowns = ["X"]
    index = {"X": 0, "T": 1, "M": 2}
    # tests/test_poisson_gpu.py: test_solve_matches_oracle / test_double_precision_matches_double_oracle
    cost_tol = {False: 1e-5, True: 1e-8}
    unk_tol = {False: {"X": 1e-5}, True: {"X": 1e-8}}

    def __init__(self, W, H):
        self.W, self.H, self.dims = W, H, [W, H]

    def base(self):
        return workloads.poisson_image_editing(self.W, self.H, seed=7)

    def mutation(self, k, w):
        W, H = self.W, self.H
        if k == 1:   # sigma = 4: sigma = 2 moves the next cost by 6e-3 only, below MOVED
            return [("X", "add", np.random.default_rng(50 + k).normal(0, 4, 4 * W * H).astype(np.float32))]
        if k == 2:
            return [("T", "set", workloads.poisson_image_editing(W, H, seed=19)["T"])]
        if k == 3:   # a rectangle straddling the disk's edge: solved pixels become fixed and back
            M = w["M"].reshape(H, W).copy()
            r = M[H // 4: H // 2, W // 8: W // 2]
            M[H // 4: H // 2, W // 8: W // 2] = np.where(r == 0, 255.0, 0.0).astype(np.float32)
            return [("M", "set", M.reshape(-1))]
        return []

    def params(self, w, double, host=False):
        assert not host
        prm = pie_t.dev(w)
        if double:
            import torch
            prm[0] = torch.from_numpy(w["X"].astype(np.float64)).cuda()
        return prm

    def oracle_step(self, w, double):
        X, c = oracle.pie_solve(w, 1, LIT, double=double)
        w["X"] = X
        return c[1]


# ------------------------------------------------------------------ shape_from_shading
class ShapeFromShading:
    name, energy, family = "sfs", E("shape_from_shading"), "shape_from_shading"
    unknowns = ["X"]
    index = {"w_p": 0, "w_s": 1, "w_g": 2, "X": 16, "D_i": 17, "Im": 18, "edgeMaskR": 19, "edgeMaskC": 20}
    # tests/test_sfs_gpu.py: test_solve_matches_oracle_synthetic / test_fp64_solve_matches_fp64_oracle
    cost_tol = {False: 1e-4, True: 1e-8}
    unk_tol = {False: {"X": 1e-4}, True: {"X": 1e-8}}

    def __init__(self, W, H):
        self.W, self.H, self.dims = W, H, [W, H]

    def base(self):
        return sfs_t.synthetic(self.W, self.H, seed=12)

    def mutation(self, k, w):
        n = self.W * self.H
        rng = np.random.default_rng(60 + k)
        if k == 1:
            p = w["params"]
            return [("w_p", "set", float(np.float32(3.0 * p[0]))), ("w_s", "set", float(np.float32(0.25 * p[1]))),
                    ("w_g", "set", float(np.float32(4.0 * p[2])))]
        if k == 2:
            return [("edgeMaskR", "set", (rng.uniform(size=n) < 0.5).astype(np.uint8)),
                    ("edgeMaskC", "set", (rng.uniform(size=n) < 0.5).astype(np.uint8))]
        if k == 3:   # valid depths scaled by 0.9 .. 1.1: still > 0, invalid ones untouched
            D = w["D_i"]
            s = (1.0 + 0.1 * np.sin(np.arange(n) * 0.37 + 1.0) * rng.uniform(0.5, 1.0, n)).astype(np.float32)
            Dn = np.where(D > 0, D * s, D).astype(np.float32)
            assert np.array_equal(Dn > 0, D > 0)
            return [("D_i", "set", Dn)]
        return []

    def params(self, w, double, host=False):
        assert not host
        return sfs_t.params64(w) if double else sfs_t.params(w)

    def oracle_step(self, w, double):
        X, c = oracle.sfs_solve(w, 1, LIT, lm=False, double=double)
        w["X"] = X
        return c[1]


def _sfs_set_scalar(w, key, v):
    p = w["params"].copy()
    p[{"w_p": 0, "w_s": 1, "w_g": 2}[key]] = v
    w["params"] = p


# --------------------------------------------------------------- arap_mesh_deformation
class Arap:
    name, energy, family = "arap", E("arap_mesh_deformation"), "arap_mesh_deformation"
    unknowns = ["Offset", "Angle"]
    index = {"w_fitSqrt": 0, "w_regSqrt": 1, "Offset": 2, "Angle": 3, "UrShape": 4, "Constraints": 5, "v0": 7, "v1": 8}
    # tests/test_arap_gpu.py: test_solve_matches_oracle / test_fp64_solve_matches_fp64_oracle
    cost_tol = {False: 1e-4, True: 1e-8}
    unk_tol = {False: {"Offset": 1e-4, "Angle": 1e-3}, True: {"Offset": 1e-8, "Angle": 1e-8}}

    def __init__(self, nx, ny):
        self.nx, self.ny = nx, ny
        w = self.base()
        self.dims = [w["N"], w["E"]]

    def base(self):
        return arap_t.perturbed(self.nx, self.ny, seed=21)

    def mutation(self, k, w):
        if k == 0:
            return []
        rng = np.random.default_rng(40 + k)   # the noise of test_graph_caches_follow_array_updates_between_steps
        ops = [("Angle", "add", (0.3 * rng.normal(size=w["Angle"].size)).astype(np.float32)),
               ("UrShape", "add", (0.05 * rng.normal(size=w["UrShape"].size)).astype(np.float32))]
        if k == 2:   # every third edge becomes a duplicate of a kept edge: same E, indices in range
            Ecount = w["E"]
            drop = np.flatnonzero(np.arange(Ecount) % 3 == 0)
            kept = np.flatnonzero(np.arange(Ecount) % 3 != 0)
            src = kept[(7 * np.arange(drop.size)) % kept.size]
            v0, v1 = w["v0"].copy(), w["v1"].copy()
            v0[drop], v1[drop] = v0[src], v1[src]
            assert v0.min() >= 0 and v1.min() >= 0 and max(v0.max(), v1.max()) < w["N"]
            ops += [("v0", "set", v0), ("v1", "set", v1)]
        if k == 3:   # one handle (a finite interior constraint) moves
            C = w["Constraints"].reshape(-1, 3).copy()
            interior = np.flatnonzero(np.isfinite(C[:, 0]))
            interior = interior[(interior >= self.nx) & (interior < w["N"] - self.nx)]
            C[interior[0]] += np.array([0.2, -0.15, 0.1], np.float32)
            ops.append(("Constraints", "set", C.reshape(-1)))
        return ops

    def params(self, w, double, host=False):
        return arap_t.params(w, host=host, double=double)

    def oracle_step(self, w, double):
        O, A, c = oracle.arap_solve(w, 1, LIT, double=double)
        w["Offset"], w["Angle"] = O, A
        return c[1]


CASES = {
    "of64x48": OpticalFlow(64, 48),
    "of130x7": OpticalFlow(130, 7),     # 62-column strip edges: 130 = 2 * 62 + 6
    "pie64x48": Poisson(64, 48),
    "sfs97x61": ShapeFromShading(97, 61),
    "arap20x13": Arap(20, 13),          # 260 vertices: no multiple of 64
}


def _err(u, a, b, double):
    """The families' own measures: rel_err, but the absolute difference for ARAP's fp32
    angles (tests/test_arap_gpu.py::test_solve_matches_oracle)."""
    if u == "Angle" and not double:
        return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return rel_err(a, b)


# ----------------------------------------------------------------- the oracle's replay
def _apply_oracle(case, w, ops, double):
    dt = np.float64 if double else np.float32
    for key, op, v in ops:
        if key in ("w_p", "w_s", "w_g"):
            _sfs_set_scalar(w, key, v)
        elif op == "add":
            t = dt if key in case.unknowns else w[key].dtype
            w[key] = (w[key].astype(t) + v.astype(t)).astype(t)
        else:
            w[key] = v.copy() if isinstance(v, np.ndarray) else v


def _replay(case, double, mutate=True, ulp=0):
    """Costs after each of NSTEPS one-step oracle solves and the final dict."""
    dt = np.float64 if double else np.float32
    w = case.base()
    for u in case.unknowns:
        w[u] = w[u].astype(dt)

    def perturb():
        rng = np.random.default_rng(ulp)
        u = case.unknowns[0]
        w[u] = (w[u] * (1 + 2.0 ** -24 * rng.standard_normal(w[u].size))).astype(dt)

    pending = bool(ulp)
    costs = []
    for k in range(NSTEPS):
        if pending and np.any(w[case.unknowns[0]] != 0):
            perturb()
            pending = False
        if mutate:
            _apply_oracle(case, w, case.mutation(k, w), double)
        costs.append(case.oracle_step(w, double))
    return np.array(costs), w


@functools.lru_cache(maxsize=None)
def reference(cname, double):
    """(costs, final dict, per-step cost floor, per-unknown floor) of the mutated replay and
    the condition that the mutations matter; computed once per case and precision, shared
    by the hand-written and generated rows and by both `how`."""
    case = CASES[cname]
    ref, wo = _replay(case, double)
    plain, _ = _replay(case, double, mutate=False)
    moved = np.abs(ref - plain) / plain
    floor = np.zeros(NSTEPS)
    ufloor = {u: 0.0 for u in case.unknowns}
    if not double:
        reps = [_replay(case, double, ulp=s) for s in (1, 2)]
        floor = np.max([np.abs(r - ref) / ref for r, _ in reps], axis=0)
        for u in case.unknowns:
            ufloor[u] = max(_err(u, w2[u], wo[u], double) for _, w2 in reps)
    return ref, wo, floor, ufloor, moved


# ------------------------------------------------------------------- the solver's side
def _to_np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else t


def _apply_solver(case, prm, ops, how, kept):
    import torch

    if how == "rebind":   # fresh buffers for EVERY array, the unknowns included; the old ones
        for i, p in enumerate(prm):   # stay allocated (no address comes back) with their old content
            if isinstance(p, torch.Tensor):
                kept.append(p)
                prm[i] = p.clone()
    for key, op, v in ops:
        i = case.index[key]
        p = prm[i]
        if isinstance(p, torch.Tensor):
            d = torch.from_numpy(np.ascontiguousarray(v)).to(device=p.device, dtype=p.dtype)
            p.add_(d) if op == "add" else p.copy_(d)
        elif isinstance(p, np.ndarray):   # backend_cpu host arrays
            if op == "add":
                p += v.astype(p.dtype)
            else:
                p[...] = v
        else:
            prm[i] = v


def _run(case, double, how, host=False, kind="gaussNewtonGPU", family=None, trial=None, mat=None, mutate=True):
    """init + NSTEPS steps with the case's mutations (none with mutate=False); (costs,
    {unknown: final values}). mat: None for a matrix-free plan, "fused" / "unfused" for a
    materialized one (useMaterializedJTJ with / without useFusedJTJ)."""
    import torch

    s = OptSolver(case.dims, case.energy, kind, double_precision=double,
                  backend="backend_cpu" if host else "backend_cuda",
                  materialized=mat is not None, fused_jtj=mat == "fused")
    assert (s.materialized_nonzeros() is not None) == (mat is not None)
    assert s.family() == (family or case.family)
    s.set_solver_params({"nIterations": NSTEPS, "lIterations": LIT})
    w = case.base()
    prm = case.params(w, double, host=host)
    s.init(prm)
    ptrs = [p.data_ptr() for p in prm if isinstance(p, torch.Tensor)]
    costs, kept = [], []
    for k in range(NSTEPS):
        # the mutation's values come from the case's own base arrays, not from the solver
        ops = case.mutation(k, w) if mutate else []
        _apply_oracle(case, w, [o for o in ops if o[0] not in case.unknowns], double)
        if ops:
            _apply_solver(case, prm, ops, how, kept)
        assert s.step(prm)
        costs.append(s.cost())
        if trial is not None:   # LM: the step's model cost and the cost at its trial point
            trial.append(s.scalars(2))
    now = [p.data_ptr() for p in prm if isinstance(p, torch.Tensor)]
    if how == "in_place" or not mutate:
        assert now == ptrs   # every update was in place
    else:
        assert not host and all(a != b for a, b in zip(now, ptrs))
    out = {u: np.array(_to_np(prm[case.index[u]])) for u in case.unknowns}
    s.close()
    return np.array(costs), out


def _check(case, cname, double, costs, unk):
    ref, wo, floor, ufloor, moved = reference(cname, double)
    assert np.all(moved[1:] >= MOVED), ("the mutations do not move the oracle enough", moved)
    drift = np.abs(costs - ref) / ref
    bar = np.maximum(2 * floor, case.cost_tol[double])
    udrift = {u: _err(u, unk[u], wo[u], double) for u in case.unknowns}
    ubar = {u: max(2 * ufloor[u], case.unk_tol[double][u]) for u in case.unknowns}
    print(f"{cname} double={double}: cost drift {drift} bar {bar} (oracle 1-ulp floor {floor}); "
          f"unknowns {udrift} bar {ubar}; mutated vs unmutated oracle {moved}")
    assert np.all(drift <= bar), (drift, bar)
    for u in case.unknowns:
        assert udrift[u] <= ubar[u], (u, udrift[u], ubar[u])


ROWS = [(c, gen, dbl, None)
        for c, paths, dbls in (("of64x48", (True, False), (False, True)), ("of130x7", (True, False), (False, True)),
                               ("pie64x48", (False, True), (False, True)), ("sfs97x61", (False, True), (False, True)),
                               ("arap20x13", (False,), (False, True)))
        for gen in paths for dbl in dbls]
# ARAP on materialized plans (fp64): the mutation before step 2 re-wires v0 / v1, and J's
# column structure — hence the J^T and J^T J patterns, the SELL copies and the product map
# of csr.h — comes from those arrays
ROWS += [("arap20x13", False, True, m) for m in ("fused", "unfused")]


@functools.lru_cache(maxsize=None)
def _materialized_control(cname, double, mat):
    """The unmutated solve on a materialized plan against the unmutated oracle replay, at
    the family's own bars: the materialized path itself agrees with the (matrix-free)
    oracle before anything is re-wired. Once per plan kind."""
    case = CASES[cname]
    costs, unk = _run(case, double, "in_place", mat=mat, mutate=False)
    ref, wo = _replay(case, double, mutate=False)
    drift = np.abs(costs - ref) / ref
    udrift = {u: _err(u, unk[u], wo[u], double) for u in case.unknowns}
    print(f"{cname} double={double} materialized {mat}, no mutation: cost drift {drift}, unknowns {udrift}")
    return drift, udrift


@pytest.mark.parametrize("how", ["in_place", "rebind"])
@pytest.mark.parametrize("cname,generated,double,mat", ROWS,
                         ids=[f"{c}-{'generated' if g else 'handwritten'}-{'fp64' if d else 'fp32'}"
                              + (f"-materialized-{m}" if m else "") for c, g, d, m in ROWS])
def test_arrays_changed_between_steps_match_oracle(monkeypatch, cname, generated, double, mat, how):
    """See the module docstring (mutations, bars, the shape_from_shading restriction). The
    materialized rows first hold the unmutated solve to the same bars (the control)."""
    if generated:
        monkeypatch.setenv("OPT_AMD_GENERIC", "1")
    case = CASES[cname]
    if mat:
        drift, udrift = _materialized_control(cname, double, mat)
        assert np.all(drift <= case.cost_tol[double]), drift
        for u in case.unknowns:
            assert udrift[u] <= case.unk_tol[double][u], (u, udrift[u])
    costs, unk = _run(case, double, how, family="generic" if generated else None, mat=mat)
    _check(case, cname, double, costs, unk)


@pytest.mark.parametrize("cname,generated", [("of64x48", True), ("arap20x13", False)])
def test_host_buffers_changed_between_steps_equal_device_path(monkeypatch, cname, generated):
    """backend_cpu (host staging, re-uploaded at every bind): numpy arrays rewritten in place
    between Steps give bitwise the device-pointer run of the same case, as the families'
    test_host_buffers_equal_device_path assert on unchanged arrays; the device run is held
    to the oracle as above."""
    if generated:
        monkeypatch.setenv("OPT_AMD_GENERIC", "1")
    case = CASES[cname]
    double = generated   # generated optical_flow in fp64, hand-written ARAP in fp32
    fam = "generic" if generated else None
    cd, ud = _run(case, double, "in_place", family=fam)
    ch, uh = _run(case, double, "in_place", host=True, family=fam)
    np.testing.assert_array_equal(ch, cd)
    for u in case.unknowns:
        np.testing.assert_array_equal(uh[u], ud[u])
    _check(case, cname, double, cd, ud)


def test_generated_optical_flow_lm_sample_cache_forms_agree(monkeypatch):
    """LM, generated optical_flow, fp64, the same mutations: the per-Step sample cache
    (OPT_AMD_GEN_SAMPLE_CACHE=1, the default) against the samples evaluated inside the
    residuals (=0), on fresh plans — per lua.cpp the same expressions on the same inputs.
    This is a consistency check between two forms of one path, NOT the reference (LM's
    trust-region radius is plan state, so the oracle cannot replay it one step at a time);
    the GN rows above carry the parity with the oracle. It is also the only GPU run of the
    =0 form.

    On this problem LM rejects its steps (the oracle's LM rejects the first four from X = 0
    as well, and after a flow edit the trial cost is far above the plan's previous cost,
    which is plan state as in the reference), so the accepted-cost sequence and the final X
    alone would say little: the model cost and the trial-point cost each Step computed
    (the plan's first two scalar slots) are compared too, and they must change from Step
    to Step as the arrays do."""
    monkeypatch.setenv("OPT_AMD_GENERIC", "1")
    case = CASES["of64x48"]
    out, trial = {}, {}
    for c in ("1", "0"):
        monkeypatch.setenv("OPT_AMD_GEN_SAMPLE_CACHE", c)
        trial[c] = []
        out[c] = _run(case, True, "in_place", kind="LMGPU", family="generic", trial=trial[c])
    print("LM costs, cache on / off:", out["1"][0], out["0"][0])
    print("LM model / trial costs, cache on / off:", trial["1"], trial["0"])
    np.testing.assert_allclose(out["1"][0], out["0"][0], rtol=case.cost_tol[True])
    assert rel_err(out["1"][1]["X"], out["0"][1]["X"]) < case.unk_tol[True]["X"]
    np.testing.assert_allclose(trial["1"], trial["0"], rtol=case.cost_tol[True])
    t = np.array(trial["0"])
    assert np.all(np.abs(np.diff(t[:, 1])) / t[1:, 1] >= MOVED), t
