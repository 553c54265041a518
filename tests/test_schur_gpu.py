"""GPU: Eliminate(X) — PCG on the Schur complement S = B - E M^-1 E^T of bundle adjustment's
points (energies/bundle_adjustment_schur.t), against the float64 AD oracle
(oracle.examples_ad.Model): its dense J gives A = J^T J = [[B, E], [E^T, C]], b = -J^T F and
from them S, the reduced right-hand side and the back-substitution, all in numpy.

Inputs: the bundle() construction of tests/test_multispace_gpu.py, restated here, at its
sizes (5 cameras, 131 points) and (70, 9). Tolerances are that file's: fp32 vectors within
2e-5 of the largest magnitude, scalars 1e-5, solves 1e-4; fp64 1e-9 / 1e-9 / 1e-8.

Converged inner solves: lIterations is the first count at which a numpy PCG on S with the
block-Jacobi(B) preconditioner has a relative residual below 1e-10 (asserted to be at most
twice the reduced dimension), and q_tolerance is set so that LM's exit test never fires
(zeta < -1e30), so the solver's step is the dense solve of the full system and can be
compared with numpy's and with the oracle's loop run to convergence."""
import os

import numpy as np
import pytest

from opt_amd import OptSolver, api
from oracle import examples_ad as ad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = os.path.join(ROOT, "energies", "bundle_adjustment.t")
SCHUR = os.path.join(ROOT, "energies", "bundle_adjustment_schur.t")
SIZES = [(5, 131), (70, 9)]
NO_EXIT = -1e30      # q_tolerance: zeta < NO_EXIT never holds


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def zeros(n, double):
    import torch
    return torch.zeros(n, device="cuda", dtype=torch.float64 if double else torch.float32)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def tols(double):
    return (1e-9, 1e-9, 1e-8) if double else (2e-5, 1e-5, 1e-4)


def rot(ang):
    """L.Rotate3D's matrix (lib.t:84-97) for an (n, 3) array of angles -> (n, 3, 3)."""
    a, b, g = ang[:, 0], ang[:, 1], ang[:, 2]
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    return np.stack([cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                     sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca,
                     -sb, cb * sa, cb * ca], -1).reshape(-1, 3, 3)


# ------------------------------------------------------------------ the bundle problem
_BUNDLE = {}


def bundle(NC, NP):
    """Inputs (all rounded to fp32) of the bundle problem; built once per size."""
    if (NC, NP) in _BUNDLE:
        return _BUNDLE[(NC, NP)]
    rng = np.random.default_rng(1000 * NC + NP)
    X = rng.uniform(-1, 1, (NP, 3))
    R = rng.normal(0, 0.15, (NC, 3))
    T = np.array([0, 0, 5.0]) + rng.normal(0, 0.3, (NC, 3))
    cam, pt = [np.zeros(NP, np.int64)], [np.arange(NP)]          # camera 0 sees every point
    for c in range(1, NC - 1):                                   # the last camera sees none
        k = max(3, NP // 3)
        cam.append(np.full(k, c))
        pt.append(rng.choice(NP - 1, k, replace=False))          # point NP-1: seen once
    cam, pt = np.concatenate(cam), np.concatenate(pt)
    order = rng.permutation(len(cam))
    cam, pt = cam[order].astype(np.int32), pt[order].astype(np.int32)
    NO = len(cam)
    q = np.einsum("nij,nj->ni", rot(R)[cam], X[pt]) + T[cam]
    obs_slot = rng.permutation(NO).astype(np.int32)               # Obs in an order of its own
    Obs = np.zeros((NO, 2))
    Obs[obs_slot] = q[:, :2] / q[:, 2:3] + rng.normal(0, 1e-3, (NO, 2))
    w = dict(NC=NC, NP=NP, NO=NO, c=cam, p=pt, o=obs_slot, Obs=f32(Obs), w_cam=0.1, w_pt=0.1,
             CamR=f32(R + rng.normal(0, 0.02, R.shape)), CamT=f32(T + rng.normal(0, 0.05, T.shape)),
             X=f32(X + rng.normal(0, 0.05, X.shape)))
    _BUNDLE[(NC, NP)] = w
    return w


def bundle_model(w):
    import torch
    m = ad.Model([("CamR", w["CamR"]), ("CamT", w["CamT"]), ("X", w["X"])],
                 {"CamR0": w["CamR"], "CamT0": w["CamT"], "X0": w["X"], "Obs": w["Obs"]})
    wc, wp = float(np.float32(w["w_cam"])), float(np.float32(w["w_pt"]))
    ic, ip = np.arange(w["NC"]), np.arange(w["NP"])
    m.term(lambda r, r0: wc * (r - r0), [("u", "CamR", ic), ("c", "CamR0", ic)], 3)
    m.term(lambda t, t0: wc * (t - t0), [("u", "CamT", ic), ("c", "CamT0", ic)], 3)
    m.term(lambda x, x0: wp * (x - x0), [("u", "X", ip), ("c", "X0", ip)], 3)

    def reproject(r, t, x, ob):
        q = ad._rotate3d(r, x) + t
        return torch.stack([q[0] / q[2] - ob[0], q[1] / q[2] - ob[1]])

    m.term(reproject, [("u", "CamR", w["c"]), ("u", "CamT", w["c"]), ("u", "X", w["p"]), ("c", "Obs", w["o"])], 2)
    return m


def bundle_params(w, double, host=False):
    T = np.float64 if double else np.float32
    put = (lambda a: np.ascontiguousarray(a)) if host else cuda
    unk = [put(w[k].astype(T)) for k in ("CamR", "CamT", "X")]
    prm = [w["w_cam"], w["w_pt"]] + unk + [put(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
    return prm, unk


def solver(w, kind="gaussNewtonGPU", double=False, path=SCHUR, **kw):
    return OptSolver([w["NC"], w["NP"], w["NO"]], path, kind, double_precision=double, **kw)


def unknowns_of(unk):
    return np.concatenate([np.asarray(u.cpu().numpy() if hasattr(u, "cpu") else u, np.float64).reshape(-1) for u in unk])


# ------------------------------------------------------------------ numpy restatements
def guarded_invert(d):
    return 1.0 / (1.0 + np.sqrt(d)) ** 2


def lm_ctc(diag, radius, min_d=float(np.float32(1e-6)), max_d=float(np.float32(1e32))):
    """lm_init_kernel, first step (the plan's own rule): SSq = guarded_invert(diag),
    CtC = clamp(diag / radius, min_lm / (SSq radius), max_lm / (SSq radius))."""
    ssq = guarded_invert(diag)
    clampm = (1.0 / ssq) / radius
    return np.clip(diag / radius, min_d * clampm, max_d * clampm)


def linearise(model):
    """(A = J^T J dense, b = -J^T F, diag as the reference forms it) at the model's unknowns."""
    J = model.jacobian()
    F = model.residuals()
    return (J.T @ J).toarray(), -(J.T @ F), model.diag_access.copy()


def pivot_ratio(M):
    """Smallest Cholesky pivot over the largest diagonal entry (0 where the factorisation
    stops): what the eliminated blocks' rule compares with sqrt(eps)."""
    mx = M.diagonal().max()
    if not mx > 0:
        return 0.0
    L = np.zeros_like(M)
    worst = np.inf
    for j in range(len(M)):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        worst = min(worst, d / mx)
        if not d > 0:
            return max(worst, 0.0)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return worst


class Reduced:
    """The reduced system of A delta = b: retained unknowns first (nr of them), the eliminated
    ones in blocks of `C`. add: LM's diagonal. held: eliminated elements with M^-1 = 0."""

    def __init__(self, A, b, nr, C=3, Cr=6, add=None, held=()):
        n = len(b)
        self.nr, self.n, self.C, self.Cr = nr, n, C, Cr
        A = A + (np.diag(add) if add is not None else 0.0)
        self.B, self.E, self.b = A[:nr, :nr], A[:nr, nr:], b
        Cm = A[nr:, nr:]
        assert not Cm[np.kron(np.eye((n - nr) // C), np.ones((C, C))) == 0].any()    # block-diagonal
        self.Minv = np.zeros((n - nr, n - nr))
        for e in range((n - nr) // C):
            ix = np.arange(C * e, C * e + C)
            if e not in held:
                self.Minv[np.ix_(ix, ix)] = np.linalg.inv(Cm[np.ix_(ix, ix)])
        self.S = self.B - self.E @ self.Minv @ self.E.T
        self.rhs = b[:nr] - self.E @ (self.Minv @ b[nr:])

    def back(self, dr):
        return np.concatenate([dr, self.Minv @ (self.b[self.nr:] - self.E.T @ dr)])

    def block_jacobi(self):
        C = self.Cr
        P = np.zeros_like(self.B)
        for e in range(self.nr // C):
            ix = np.arange(C * e, C * e + C)
            P[np.ix_(ix, ix)] = np.linalg.inv(self.B[np.ix_(ix, ix)])
        return P

    def pcg_count(self, tol=1e-10):
        """First iteration count at which PCG on S (block-Jacobi of B) has |r| / |rhs| < tol."""
        P = self.block_jacobi()
        r = self.rhs.copy()
        z = P @ r
        p = z.copy()
        rz = r @ z
        x = np.zeros(self.nr)
        for k in range(1, 4 * self.nr + 1):
            Ap = self.S @ p
            alpha = rz / (p @ Ap)
            x += alpha * p
            r -= alpha * Ap
            if np.linalg.norm(r) < tol * np.linalg.norm(self.rhs):
                return k
            z = P @ r
            rz_new = r @ z
            p = z + (rz_new / rz) * p
            rz = rz_new
        return 4 * self.nr + 1


def cam_perm(w):
    """Unknown order of the plan (CamR | CamT | X) -> cameras' six channels together | X."""
    NC = w["NC"]
    e, c3 = np.arange(NC)[:, None], np.arange(3)[None, :]
    cams = np.concatenate([3 * e + c3, 3 * NC + 3 * e + c3], 1).reshape(-1)
    return np.concatenate([cams, np.arange(6 * NC, 6 * NC + 3 * w["NP"])])


def reduced_of(w, A, b, **kw):
    """Reduced system in camera-major order, and the permutation back to the plan's order."""
    pm = cam_perm(w)
    add = kw.pop("add", None)
    return Reduced(A[np.ix_(pm, pm)], b[pm], 6 * w["NC"], add=None if add is None else add[pm], **kw), pm


_LIN = {}


def start_system(NC, NP):
    key = (NC, NP)
    if key not in _LIN:
        _LIN[key] = linearise(bundle_model(bundle(NC, NP)))
    return _LIN[key]


def converged_count(R):
    L = R.pcg_count()
    print("PCG on S: %d iterations to 1e-10 (reduced dimension %d)" % (L, R.nr))
    assert L <= 2 * R.nr
    return L


# ------------------------------------------------------------------ the reduced apply
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_reduced_apply_matches_the_oracles_schur_complement(NC, NP, kind, double):
    """Measured float32 restatement errors of S p (numpy, same formula, against float64):
    all below 2e-5 at these sizes, so the fp32 bar is the project's 2e-5."""
    w = bundle(NC, NP)
    A, b, diag = start_system(NC, NP)
    add = lm_ctc(diag, 1e4) if kind == "LMGPU" else None
    R, pm = reduced_of(w, A, b, add=add)
    n, nr = len(b), 6 * NC
    p = np.random.default_rng(NC + NP).normal(size=n)
    if not double:
        p = p.astype(np.float32).astype(np.float64)
    Sp_ref = np.zeros(n)
    Sp_ref[pm[:nr]] = R.S @ p[pm][:nr]
    # the same formula in float32: the bar moves only if float32 itself cannot reach 2e-5
    B32, E32, Mi32, p32 = f32(R.B), f32(R.E), f32(R.Minv), f32(p[pm][:nr])
    err32 = rel_err(B32 @ p32 - E32 @ (Mi32 @ (E32.T @ p32)), Sp_ref[pm[:nr]])
    vec = tols(double)[0]
    bar = vec if double or err32 <= vec else 4 * err32
    s = solver(w, kind, double)
    prm, _ = bundle_params(w, double)
    T = np.float64 if double else np.float32
    out = []
    for garbage in (0.0, np.nan, 1e30):
        pg = p.copy()
        pg[nr:] = garbage
        Sp = zeros(n, double)
        Sp += 7.0                                   # (the eliminated entries must be written)
        s.apply_reduced(prm, cuda(pg.astype(T)), Sp)
        out.append(Sp.cpu().numpy())
    print("S p", rel_err(out[0], Sp_ref), "bar", bar, "float32 restatement", err32)
    assert rel_err(out[0], Sp_ref) < bar
    assert not out[0][nr:].any()
    assert out[0].tobytes() == out[1].tobytes() == out[2].tobytes()


@pytest.mark.parametrize("NC,NP", SIZES)
def test_layout_and_entry_points(NC, NP, tmp_path):
    w = bundle(NC, NP)
    blk = tmp_path / "ba_block.t"
    blk.write_text(open(BA).read().replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    s, sb, ss = solver(w, double=True), solver(w, double=True, path=str(blk)), solver(w, double=True, path=BA)
    assert s.family() == "generic"
    assert s.eliminated() == [0, 0, 1]
    assert sb.eliminated() == [0, 0, 0] and ss.eliminated() == [0, 0, 0]
    assert s.lib.OptAMD_PlanEliminated(None, 4, None) == -1
    assert s.unknown_layout() == sb.unknown_layout() == ([0, 3 * NC, 6 * NC], [NC, NC, NP], [3, 3, 3])
    assert s.preconditioner_blocks() == sb.preconditioner_blocks() == ([0, 0, 1], [0, 3, 0], 2)
    prm, _ = bundle_params(w, True)
    A, _, _ = start_system(NC, NP)
    n = s.unknown_count()
    p = np.random.default_rng(7).normal(size=n)
    Ap = zeros(n, True)
    pAp = s.apply_jtj(prm, cuda(p), Ap)              # still the full J^T J p
    print("J^T J p", rel_err(Ap.cpu().numpy(), A @ p))
    assert rel_err(Ap.cpu().numpy(), A @ p) < 1e-9
    assert pAp == pytest.approx(float(p @ A @ p), rel=1e-9)
    for other in (sb, ss):                           # no reduced system without the statement
        with pytest.raises(api.OptError, match="OptAMD_ApplyReduced failed"):
            other.apply_reduced(prm, cuda(p), Ap)


def test_materialized_paths_are_refused_by_name(capfd):
    w = bundle(5, 131)
    capfd.readouterr()
    for kw in ({"materialized": True}, {"materialized": True, "fused_jtj": True}, {"fused_jtj": True}):
        with pytest.raises(api.OptError, match="Opt_ProblemPlan failed"):
            solver(w, **kw)
        assert "useMaterializedJTJ / useFusedJTJ) with Eliminate" in capfd.readouterr().err
    s = solver(w)
    group = s.lib.OptAMD_LocalGroupCreate(2)
    with pytest.raises(api.OptError, match="OptAMD_PlanSetDecomposition failed"):
        s.set_decomposition(s.lib.OptAMD_LocalGroupRank(group, 0), 0, 1)
    s.lib.OptAMD_LocalGroupDestroy(group)
    assert "no row-slab decomposition with the block preconditioner" in capfd.readouterr().err


# ------------------------------------------------------------------ one converged GN step
@pytest.mark.parametrize("NC,NP", SIZES)
def test_one_converged_gn_step_is_the_dense_solve(NC, NP):
    w = bundle(NC, NP)
    A, b, _ = start_system(NC, NP)
    R, _ = reduced_of(w, A, b)
    L = converged_count(R)
    s = solver(w, double=True)
    s.set_solver_params({"nIterations": 1, "lIterations": L})
    prm, unk = bundle_params(w, True)
    x0 = unknowns_of(unk)
    s.solve(prm)
    x1, ref = unknowns_of(unk), x0 + np.linalg.solve(A, b)
    off = [0, 3 * NC, 6 * NC, len(b)]
    for k, name in enumerate(("CamR", "CamT", "X")):
        sl = slice(off[k], off[k + 1])
        print(name, "unknowns", rel_err(x1[sl], ref[sl]), "delta", rel_err(x1[sl] - x0[sl], ref[sl] - x0[sl]))
        assert rel_err(x1[sl], ref[sl]) < 1e-8


# ------------------------------------------------------------------ whole solves
_DENSE = {}


def dense_gn(NC, NP, steps=3):
    """Costs of dense Gauss-Newton steps, and the largest converged PCG count over them."""
    if (NC, NP) not in _DENSE:
        w = bundle(NC, NP)
        m = bundle_model(w)
        costs, L = [m.cost()], 0
        for _ in range(steps):
            A, b, _ = linearise(m)
            L = max(L, converged_count(reduced_of(w, A, b)[0]))
            m.set(m.get() + np.linalg.solve(A, b))
            costs.append(m.cost())
        _DENSE[(NC, NP)] = (costs, L)
    return _DENSE[(NC, NP)]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_gn_solve_matches_dense_gauss_newton(NC, NP, double):
    w = bundle(NC, NP)
    ref, L = dense_gn(NC, NP)
    s = solver(w, double=double)
    s.set_solver_params({"nIterations": 3, "lIterations": L})
    prm, _ = bundle_params(w, double)
    costs = s.profiled_solve(prm)
    print("costs", costs, "dense", ref, "lIterations", L)
    assert len(costs) == 4
    np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])


_LM = {}


def oracle_lm(NC, NP, steps=5):
    """ad.solve(lm=True) run to convergence inside every step (2 n PCG iterations on the full
    system, no exit test), and the converged count for S at the start (LM's diagonal at the
    first radius) or at any dense GN step, whichever is larger."""
    if (NC, NP) not in _LM:
        w = bundle(NC, NP)
        A, b, diag = start_system(NC, NP)
        L = max(converged_count(reduced_of(w, A, b, add=lm_ctc(diag, 1e4))[0]), dense_gn(NC, NP)[1])
        _LM[(NC, NP)] = (list(ad.solve(bundle_model(w), steps, 2 * len(b), lm=True, q_tolerance=NO_EXIT)), L)
    return _LM[(NC, NP)]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_lm_solve_matches_the_oracle(NC, NP, double):
    w = bundle(NC, NP)
    ref, L = oracle_lm(NC, NP)
    s = solver(w, "LMGPU", double)
    s.set_solver_params({"nIterations": 5, "lIterations": L, "q_tolerance": NO_EXIT})
    prm, _ = bundle_params(w, double)
    costs = s.profiled_solve(prm)
    print("costs", costs, "oracle", ref, "lIterations", L)
    # The oracle accepts three steps and then stops inside the fourth: its cost change there,
    # 3e-10 of the cost, is below function_tolerance (1e-6). In fp64 the plan decides the same.
    # In fp32 a change of 3e-10 is below the format's resolution (6e-8): the fourth step's new
    # cost equals the old one, which LM reads as a rejected step, not as a stop. So: every
    # step the oracle took is decided as the oracle decided it, fp64 also stops where it
    # stopped, and fp32 may only append rejected steps (the cost bitwise unchanged).
    k = len(ref)
    assert len(costs) == k if double else len(costs) >= k
    assert [b < a for a, b in zip(costs[:k], costs[1:k])] == [b < a for a, b in zip(ref, ref[1:])]   # accept / reject
    np.testing.assert_allclose(costs[:k], ref, rtol=tols(double)[2])
    assert all(c == costs[k - 1] for c in costs[k:])


# ------------------------------------------------------------------ elements held fixed
def without_point_edges(w, point):
    """The problem with every observation of `point` dropped (Obs re-packed in edge order)."""
    keep = w["p"] != point
    v = dict(w)
    v["c"], v["p"] = w["c"][keep], w["p"][keep]
    v["Obs"] = np.ascontiguousarray(w["Obs"][w["o"][keep]])
    v["NO"] = int(keep.sum())
    v["o"] = np.arange(v["NO"], dtype=np.int32)
    return v


@pytest.mark.parametrize("drop", [False, True])
def test_rank_deficient_points_are_held_fixed(drop):
    """w_pt = 0: a point seen once has a rank-2 block (last pivot of order eps), a point seen
    never a zero block; both get M^-1 = 0 and delta = 0 exactly, and the rest is the dense
    solve of the system without their columns."""
    w = dict(bundle(5, 131))
    w["w_pt"] = 0.0
    if drop:
        w = without_point_edges(w, 130)              # point NP-1: seen by camera 0 alone
    NC, NP = w["NC"], w["NP"]
    seen = np.bincount(w["p"], minlength=NP)
    held = set(np.flatnonzero(seen <= 1).tolist())
    assert 130 in held and (seen[130] == 0) == drop and len(held) > 1
    A, b, _ = linearise(bundle_model(w))
    ratios = np.array([pivot_ratio(A[6 * NC + 3 * e: 6 * NC + 3 * e + 3, 6 * NC + 3 * e: 6 * NC + 3 * e + 3]) for e in range(NP)])
    others = np.array([e not in held for e in range(NP)])
    print("pivot ratios: held max %.3e, others min %.3e" % (ratios[~others].max(), ratios[others].min()))
    assert ratios[others].min() > 1e-4               # no block sits near the sqrt(eps) threshold
    assert ratios[~others].max() < 1e-12
    R, _ = reduced_of(w, A, b, held=held)
    L = converged_count(R)
    s = solver(w, double=True)
    s.set_solver_params({"nIterations": 1, "lIterations": L})
    prm, unk = bundle_params(w, True)
    x0 = unknowns_of(unk)
    s.solve(prm)
    x1 = unknowns_of(unk)
    cols = np.ones(len(b), bool)
    for e in held:
        cols[6 * NC + 3 * e: 6 * NC + 3 * e + 3] = False
    ref = x0.copy()
    ref[cols] += np.linalg.solve(A[np.ix_(cols, cols)], b[cols])
    assert x1[~cols].tobytes() == x0[~cols].tobytes()              # delta = 0 exactly
    print("free unknowns", rel_err(x1[cols], ref[cols]), "delta", rel_err(x1[cols] - x0[cols], ref[cols] - x0[cols]))
    assert rel_err(x1[cols], ref[cols]) < 1e-8
    assert not np.array_equal(x1[cols], x0[cols])


# ------------------------------------------------------------------ Exclude in the eliminated space
EXCLUDED = """
local N, M, E = Dim("N", 0), Dim("M", 1), Dim("E", 2)
local X  = Unknown("X", opt_float2, {N}, 0)
local Y  = Unknown("Y", opt_float2, {M}, 1)
local A  = Array("A", opt_float2, {N}, 2)
local Mk = Array("Mk", opt_float, {N}, 3)
local T  = Array("T", opt_float2, {E}, 4)
local G  = Graph("G", {E}, "i", {N}, 5, "k", {M}, 6, "e", {E}, 7)
Eliminate(X)
Exclude(eq(Mk(0), 1))
Energy(0.3 * (X(0) - A(0)))
Energy(0.3 * Y(0))
Energy(X(G.i) + 2 * Y(G.k) - T(G.e))
"""


def test_excluded_elements_of_the_eliminated_space_stay(tmp_path):
    path = tmp_path / "excluded.t"
    path.write_text(EXCLUDED)
    N, M, E = 37, 5, 300
    rng = np.random.default_rng(5)
    X, Y, A = rng.normal(size=(N, 2)), rng.normal(size=(M, 2)), rng.normal(size=(N, 2))
    T = rng.normal(size=(E, 2))
    Mk = (rng.uniform(size=N) < 0.3).astype(np.float32)
    i, k = rng.integers(0, N, E).astype(np.int32), rng.integers(0, M, E).astype(np.int32)
    assert 0 < Mk.sum() < N
    m = ad.Model([("X", X), ("Y", Y)], {"A": f32(A), "T": f32(T)})
    m.term(lambda x, a: 0.3 * (x - a), [("u", "X", np.arange(N)), ("c", "A", np.arange(N))], 2)
    m.term(lambda y: 0.3 * y, [("u", "Y", np.arange(M))], 2)
    m.term(lambda x, y, t: x + 2 * y - t, [("u", "X", i), ("u", "Y", k), ("c", "T", np.arange(E))], 2)
    Am, b, _ = linearise(m)
    act = np.concatenate([np.repeat(Mk == 0, 2), np.ones(2 * M, bool)])
    ref = m.get()
    ref[act] += np.linalg.solve(Am[np.ix_(act, act)], b[act])
    pm = np.concatenate([np.arange(2 * N, 2 * N + 2 * M), np.arange(2 * N)])      # retained (Y) first
    L = converged_count(Reduced(Am[np.ix_(pm, pm)], b[pm], 2 * M, C=2, Cr=2, held=set(np.flatnonzero(Mk == 1).tolist())))
    s = OptSolver([N, M, E], str(path), "gaussNewtonGPU", double_precision=True)
    assert s.eliminated() == [1, 0]
    s.set_solver_params({"nIterations": 1, "lIterations": L})
    Xd, Yd = cuda(X), cuda(Y)
    s.solve([Xd, Yd, cuda(f32(A)), cuda(Mk), cuda(f32(T)), cuda(i), cuda(k), cuda(np.arange(E, dtype=np.int32))])
    x1 = np.concatenate([Xd.cpu().numpy().reshape(-1), Yd.cpu().numpy().reshape(-1)])
    assert x1[~act].tobytes() == m.get()[~act].tobytes()
    print("active unknowns", rel_err(x1[act], ref[act]))
    assert rel_err(x1[act], ref[act]) < 1e-8


# ------------------------------------------------------------------ determinism, backends, contracts
def test_schur_solves_are_bitwise_reproducible():
    w = bundle(5, 131)
    out = []
    for _ in range(2):
        s = solver(w, "LMGPU")
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = bundle_params(w, False)
        costs = s.profiled_solve(prm)
        out.append((np.array(costs), [u.cpu().numpy() for u in unk]))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    for a, b in zip(out[0][1], out[1][1]):
        assert a.tobytes() == b.tobytes()
    assert out[0][0][-1] < 0.2 * out[0][0][0]


def test_backend_cpu_with_host_arrays_equals_backend_cuda():
    w = bundle(5, 131)
    res = {}
    for backend in ("backend_cuda", "backend_cpu"):
        s = solver(w, backend=backend)
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = bundle_params(w, False, host=backend == "backend_cpu")
        cost = s.solve(prm)
        res[backend] = (cost, [np.asarray(u.cpu().numpy() if hasattr(u, "cpu") else u) for u in unk])
    assert res["backend_cpu"][0] == res["backend_cuda"][0]
    for a, b in zip(res["backend_cpu"][1], res["backend_cuda"][1]):
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(res["backend_cpu"][1][2], w["X"])     # the host arrays were written back


def test_slot_index_outside_its_space_stops_the_solve():
    w = dict(bundle(5, 131))
    bad = w["p"].copy()
    bad[7] = w["NP"]
    w["p"] = bad
    s = solver(w)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = bundle_params(w, False)
    before = [u.clone() for u in unk]
    with pytest.raises(api.OptError, match=f"slot 'p': vertex index {w['NP']} outside"):
        s.init(prm)
    assert s.lib.Opt_ProblemStep(s.state, s.plan, s._pk.ptr) == 0
    with pytest.raises(api.OptError, match="outside"):
        s.step()
    for a, b in zip(before, unk):
        assert bool((a == b).all())


def test_rebinding_between_steps_matches_a_fresh_plan():
    """Step-boundary contract: the second Step runs on whatever is bound then — other
    arrays, other measurements, the edges in another order (incidence lists rebuilt)."""
    w = bundle(5, 131)
    sa = solver(w)
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = bundle_params(w, False)
    sa.init(prm)
    assert sa.step()
    state = [u.cpu().numpy().copy() for u in unk]
    order = np.random.default_rng(3).permutation(w["NO"])
    w2 = dict(w, c=w["c"][order], p=w["p"][order], o=w["o"][order], Obs=f32(w["Obs"] * 1.01),
              CamR=state[0], CamT=state[1], X=state[2])
    prm_a, unk_a = bundle_params(w2, False)
    for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):          # the priors stay where they were
        prm_a[k] = cuda(w[name])
    assert sa.step(prm_a)
    sb = solver(w)
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm_b, unk_b = bundle_params(w2, False)
    for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):
        prm_b[k] = cuda(w[name])
    sb.init(prm_b)
    assert sb.step()
    for a, b, c in zip(unk_a, unk_b, state):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert not np.array_equal(a.cpu().numpy(), c)
    assert sa.cost() == sb.cost()
