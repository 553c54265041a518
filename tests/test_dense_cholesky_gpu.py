"""GPU: the dense blocked Cholesky kernels (opt_amd/csrc/dense_cholesky.hip) through the
stand-alone entry point OptAMD_DenseCholesky (api.dense_cholesky), in fp32 and fp64.

The bars are Higham's backward-error bounds (Accuracy and Stability of Numerical Algorithms,
Theorems 10.3 and 10.4), not measurements; u is 2^-24 in fp32 and 2^-53 in fp64:
    |A - L L^T|_ij <= 2 (n + 1) u max_i a_ii
    |A x - b|_i   <= 2 (3 n + 1) u sum_j sqrt(a_ii a_jj) |x_j|
with the x of the second bar from numpy's float64 solve, not from the code under test. Each test
prints the measured ratio to its bar.

Sizes: one tile (1, 5, 63), an exact tile (64), one past a tile (65), two tiles (128), three
tiles with 63 rows of padding (129), four (200) and eight (449)."""
import numpy as np
import pytest

from opt_amd import api

pytestmark = pytest.mark.gpu
SIZES = (1, 5, 63, 64, 65, 128, 129, 200, 449)
DTYPES = (np.float32, np.float64)
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
_cache = {}


def spd(n, dt):
    """A = G G^T + n I with G a seeded normal matrix rounded to fp32; b seeded normal. Computed once
    per (n, dtype) and never written to."""
    if (n, dt) not in _cache:
        rng = np.random.default_rng(1000 + n)
        G = rng.standard_normal((n, n)).astype(np.float32).astype(np.float64)
        A = (G @ G.T + n * np.eye(n)).astype(dt)
        A = np.ascontiguousarray((A + A.T) / 2)
        b = rng.standard_normal(n).astype(dt)
        A.setflags(write=False)
        b.setflags(write=False)
        _cache[(n, dt)] = (A, b)
    return _cache[(n, dt)]


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
@pytest.mark.parametrize("n", SIZES)
def test_backward_error_and_shape(n, dt):
    A, b = spd(n, dt)
    L, x, info = api.dense_cholesky(A, b)
    assert info == -1
    assert L.shape == (n, n) and x.shape == (n,) and L.dtype == dt and x.dtype == dt
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
    A64, L64 = A.astype(np.float64), L.astype(np.float64)
    u = U[dt]
    bar_f = 2 * (n + 1) * u * A64.diagonal().max()
    err_f = np.abs(A64 - L64 @ L64.T).max()
    xref = np.linalg.solve(A64, b.astype(np.float64))
    d = np.sqrt(A64.diagonal())
    bar_s = 2 * (3 * n + 1) * u * d * (d @ np.abs(xref))
    err_s = np.abs(A64 @ x.astype(np.float64) - b.astype(np.float64))
    print(f"n={n} {np.dtype(dt).name}: |A-LL^T|/bar = {err_f / bar_f:.3e}, max |Ax-b|/bar = {(err_s / bar_s).max():.3e}")
    assert err_f <= bar_f
    assert np.all(err_s <= bar_s)


def integer_factor(n=129):
    """A lower-triangular L0 of small integers whose products the kernels form exactly: L0 =
    (I + M) D with D powers of two and M strictly lower; inside a diagonal tile M is non-zero only
    at (odd row, even column), so that tile's inverse is D^-1 (I - M), dyadic like every partial
    sum of the panel products. The tiles below the diagonal are dense and asymmetric."""
    rng = np.random.default_rng(7)
    M = np.tril(rng.integers(-2, 3, (n, n)), -1).astype(np.float64)
    i, j = np.indices((n, n))
    inside = (i // 64 == j // 64) & ~((i % 2 == 1) & (j % 2 == 0))
    M[inside] = 0
    M[(i // 64 == j // 64)] = np.clip(M[(i // 64 == j // 64)], -1, 1)
    D = np.diag(2.0 ** rng.integers(0, 3, n))
    return (np.eye(n) + M) @ D


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
def test_asymmetric_integer_factor_is_returned_exactly(dt):
    """A transposed operand tile or a wrong accumulator row map cannot pass: the panel and the
    trailing update multiply tiles that are not symmetric."""
    L0 = integer_factor()
    assert not np.array_equal(L0[64:128, :64], L0[64:128, :64].T)
    A = L0 @ L0.T
    assert np.abs(A).max() < 2 ** 22
    L, x, info = api.dense_cholesky(A.astype(dt), np.ones(129, dt))
    assert info == -1
    assert np.array_equal(L.astype(np.float64), L0)


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
@pytest.mark.parametrize("bad", (0.0, np.nan), ids=("zero", "nan"))
def test_pivot_failure_reports_the_row_and_leaves_the_outputs(bad, dt):
    A, b = spd(200, dt)
    A = A.copy()
    A[70, 70] = bad
    L = np.full((200, 200), 7, dt)
    x = np.full(200, 7, dt)
    _, _, info = api.dense_cholesky(A, b, L, x)
    assert info == 70
    assert np.all(L == 7) and np.all(x == 7)


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
def test_two_calls_agree_bitwise(dt):
    A, b = spd(449, dt)
    L1, x1, _ = api.dense_cholesky(A, b)
    L2, x2, _ = api.dense_cholesky(A, b)
    assert L1.tobytes() == L2.tobytes() and x1.tobytes() == x2.tobytes()


# ====================================================================== plans: bundle adjustment
# LinearSolver("cholesky") beside ReducedSystem("explicit") on the (5, 131) and (70, 9) fixtures
# of tests/test_schur_gpu.py (n = 30 and 420: one tile, and seven with 28 rows of padding). Both
# reduced matrices are positive definite in GN and LM (lambda_min 1e-2, cond 365 and 45; numpy's
# float32 Cholesky succeeds with a smallest pivot ratio of 0.15), so the reference itself never
# takes the fall-back on them.
import os

from tests import test_schur_explicit_gpu as sx
from tests.test_schur_gpu import (SIZES as BA_SIZES, bundle, bundle_params, cuda, dense_gn, f32, lm_ctc, oracle_lm,
                                  reduced_of, rel_err, solver, start_system, tols, unknowns_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA_CHOLESKY = os.path.join(ROOT, "energies", "direct", "bundle_adjustment_schur_cholesky.t")
PG_CHOLESKY = os.path.join(ROOT, "energies", "direct", "pose_graph_2d_cholesky.t")
KINDS = ["gaussNewtonGPU", "LMGPU"]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_plan_one_step_is_the_dense_solve_of_the_reduced_system(NC, NP, kind, double):
    """delta_r against numpy's float64 solve of the oracle's reduced system, the full delta against
    its back-substitution, relative to the largest entry. delta is read as the change of the
    unknowns. The float32 numpy restatement of the solve must stay below an eighth of the bar."""
    w = bundle(NC, NP)
    A, b, diag = start_system(NC, NP)
    add = lm_ctc(diag, 1e4) if kind == "LMGPU" else None
    R, pm = reduced_of(w, A, b, add=add)
    dr = np.linalg.solve(R.S, R.rhs)
    full = np.zeros(len(b))
    full[pm] = R.back(dr)
    bar = tols(double)[1]
    err32 = rel_err(np.linalg.solve(f32(R.S), f32(R.rhs)), dr)
    print("float32 restatement of the solve: %.3e (bar %.1e)" % (err32, bar))
    if not double:
        assert err32 < bar / 8
    s = solver(w, kind, double, path=BA_CHOLESKY)
    s.set_solver_params({"nIterations": 1, "lIterations": 10})
    prm, unk = bundle_params(w, double)
    x0 = unknowns_of(unk)
    costs = s.profiled_solve(prm)
    assert costs[1] < costs[0]                                     # (LM accepted the step)
    delta = unknowns_of(unk) - x0
    info = s.direct_info()
    print("delta_r %.3e full %.3e bar %.1e" % (rel_err(delta[pm][:R.nr], dr), rel_err(delta, full), bar), info)
    assert info["n"] == 6 * NC and info["tiles"] == (-(-6 * NC // 64)) * (-(-6 * NC // 64) + 1) // 2
    assert info["factorisations"] == 1 and info["fallbacks"] == 0 and info["reason"] == "none"
    assert 0 < info["min_pivot_ratio"] <= 1
    assert rel_err(delta[pm][:R.nr], dr) < bar
    assert rel_err(delta, full) < bar


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_plan_gn_solve_matches_dense_gauss_newton(NC, NP, double):
    w = bundle(NC, NP)
    ref, _ = dense_gn(NC, NP)
    out = []
    for L in (1, 50):                                              # lIterations only switches the solve on
        s = solver(w, double=double, path=BA_CHOLESKY)
        s.set_solver_params({"nIterations": 3, "lIterations": L})
        prm, unk = bundle_params(w, double)
        out.append((np.array(s.profiled_solve(prm)), unknowns_of(unk)))
    print("costs", out[0][0], "dense", ref)
    np.testing.assert_allclose(out[0][0], ref, rtol=tols(double)[2])
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_plan_lm_solve_matches_the_oracle(NC, NP, double):
    """As tests/test_schur_gpu.py::test_lm_solve_matches_the_oracle reads the oracle's steps."""
    w = bundle(NC, NP)
    ref, _ = oracle_lm(NC, NP)
    s = solver(w, "LMGPU", double, path=BA_CHOLESKY)
    s.set_solver_params({"nIterations": 5, "lIterations": 1})
    prm, _ = bundle_params(w, double)
    costs = s.profiled_solve(prm)
    print("costs", costs, "oracle", ref)
    k = len(ref)
    assert len(costs) == k if double else len(costs) >= k
    assert [b < a for a, b in zip(costs[:k], costs[1:k])] == [b < a for a, b in zip(ref, ref[1:])]
    np.testing.assert_allclose(costs[:k], ref, rtol=tols(double)[2])
    assert all(c == costs[k - 1] for c in costs[k:])


def cholesky_variant(tmp_path, path, statement):
    out = tmp_path / ("cholesky_" + os.path.basename(path))
    text = open(path).read()
    assert text.count(statement + "\n") == 1
    out.write_text(text.replace(statement + "\n", statement + '\nLinearSolver("cholesky")\n'))
    return str(out)


def steps(w, kind, double, path, L, n=3, prm_extra=()):
    s = solver(w, kind, double, path=path)
    s.set_solver_params({"nIterations": n, "lIterations": L})
    prm, unk = bundle_params(w, double)
    costs = s.profiled_solve(prm + list(prm_extra))
    return np.array(costs), unknowns_of(unk), [u.cpu().numpy() for u in unk], s


def test_plan_held_points_and_an_excluded_camera(tmp_path):
    """w_pt = 0 holds the points seen once; camera 2 is excluded (an identity row of the dense
    matrix). fp64: the explicit-PCG file run to convergence (100 iterations)."""
    w = dict(bundle(5, 131))
    w["w_pt"] = 0.0
    assert (np.bincount(w["p"], minlength=w["NP"]) == 1).any()
    mk = np.zeros(w["NC"], np.float32)
    mk[2] = 1
    ex = sx.excluded_variant(tmp_path, sx.EXPLICIT)
    ch = cholesky_variant(tmp_path, ex, 'ReducedSystem("explicit")')
    cp, xp, _, _ = steps(w, "gaussNewtonGPU", True, ex, 100, prm_extra=[cuda(mk)])
    cc, xc, uc, s = steps(w, "gaussNewtonGPU", True, ch, 1, prm_extra=[cuda(mk)])
    print("costs cholesky", cc, "pcg", cp, "unknowns", rel_err(xc, xp), s.direct_info())
    assert s.direct_info()["factorisations"] == 3
    assert rel_err(xc, xp) < tols(True)[1]
    for k, name in enumerate(("CamR", "CamT")):
        assert uc[k][2].tobytes() == w[name][2].astype(np.float64).tobytes()   # the excluded camera did not move


def test_plan_pivot_fall_back_is_the_explicit_plans_step():
    """w_cam = 0: the last camera sees no point, so its diagonal block of S is zero and the pivot
    of its first row fails; the Step is bitwise the explicit file's PCG Step. (Gauss-Newton: LM's
    clamped diagonal makes that block 1e-10 I, the matrix positive definite, and the direct step
    legitimate: measured smallest pivot ratio 0.36, no fall-back.)"""
    kind = "gaussNewtonGPU"
    w = dict(bundle(5, 131))
    w["w_cam"] = 0.0
    cc, xc, _, s = steps(w, kind, False, BA_CHOLESKY, 10, n=1)
    cp, xp, _, sp = steps(w, kind, False, sx.EXPLICIT, 10, n=1)
    info = s.direct_info()
    print(info)
    assert info["fallbacks"] == 1 and info["factorisations"] == 0 and info["reason"] == "pivot"
    assert cc.tobytes() == cp.tobytes() and xc.tobytes() == xp.tobytes()
    assert sp.direct_info() is None


def test_plan_memory_fall_back_is_the_explicit_plans_step(monkeypatch):
    w = bundle(70, 9)
    monkeypatch.setenv("OPT_AMD_DENSE_MAX_BYTES", "1")
    cc, xc, _, s = steps(w, "LMGPU", False, BA_CHOLESKY, 10)
    monkeypatch.delenv("OPT_AMD_DENSE_MAX_BYTES")
    cp, xp, _, _ = steps(w, "LMGPU", False, sx.EXPLICIT, 10)
    info = s.direct_info()
    print(info)
    assert info["fallbacks"] == len(cc) - 1 and info["factorisations"] == 0 and info["reason"] == "memory"
    assert cc.tobytes() == cp.tobytes() and xc.tobytes() == xp.tobytes()


def test_plan_cap_is_read_at_every_step(monkeypatch):
    """OPT_AMD_DENSE_MAX_BYTES lowered after a direct Step: the next Step falls back."""
    w = bundle(5, 131)
    s = solver(w, path=BA_CHOLESKY)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, _ = bundle_params(w, False)
    s.init(prm)
    assert s.step()
    ratio = s.direct_info()["min_pivot_ratio"]
    monkeypatch.setenv("OPT_AMD_DENSE_MAX_BYTES", "1")
    assert s.step()
    info = s.direct_info()
    assert (info["factorisations"], info["fallbacks"], info["reason"]) == (1, 1, "memory")
    assert info["min_pivot_ratio"] == ratio                        # still the last factorisation's


@pytest.mark.parametrize("in_place", [False, True])
def test_plan_rewiring_between_steps_matches_a_fresh_plan(in_place):
    """The edges in another order and other measurements at the second Step, rebound or written
    into the bound arrays: the Step is a fresh plan's first."""
    w = bundle(5, 131)
    sa = solver(w, path=BA_CHOLESKY)
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = bundle_params(w, False)
    sa.init(prm)
    assert sa.step()
    state = [u.cpu().numpy().copy() for u in unk]
    order = np.random.default_rng(3).permutation(w["NO"])
    w2 = dict(w, c=w["c"][order], p=w["p"][order], o=w["o"][order], Obs=f32(w["Obs"] * 1.01),
              CamR=state[0], CamT=state[1], X=state[2])
    prm_b, unk_b = bundle_params(w2, False)
    for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):          # the priors stay where they were
        prm_b[k] = cuda(w[name])
    if in_place:
        for k in (8, 9, 10, 11):
            prm[k].copy_(prm_b[k])
        assert sa.step()
        unk_a = unk
    else:
        prm_a, unk_a = bundle_params(w2, False)
        for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):
            prm_a[k] = cuda(w[name])
        assert sa.step(prm_a)
    sb = solver(w, path=BA_CHOLESKY)
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    sb.init(prm_b)
    assert sb.step()
    for a, b, c in zip(unk_a, unk_b, state):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert not np.array_equal(a.cpu().numpy(), c)
    assert sa.cost() == sb.cost()
    assert sa.direct_info()["factorisations"] == 2 and sb.direct_info()["factorisations"] == 1


def test_plan_runs_are_bitwise_reproducible():
    out = [steps(bundle(70, 9), "LMGPU", False, BA_CHOLESKY, 10)[:2] for _ in range(2)]
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][0][-1] < 0.2 * out[0][0][0]


# ====================================================================== plans: the pose graph
# LinearSolver("cholesky") beside NormalMatrix("explicit") on arrays(N) of
# tests/test_pose_graph_gpu.py, N = 21, 22, 43, 200 (n = 63, 66, 129, 600: one row short of a
# tile, two past it, one past two tiles, ten tiles with 40 rows of padding). All four factor in
# float32 numpy (pivot ratio >= 1.9e-3), but cond(H) reaches 2.8e8 and numpy's own float32 solve
# is off by 2.9e-4 at N = 200: fp32 is held to the backward error of its linear solve alone.
from tests import test_normal_matrix_gpu as nm
from tests.test_multispace_gpu import kernel_reference, zeros
from tests.test_pose_graph_gpu import arrays, model, params
from tests.test_pose_graph_gpu import solver as pg_solver

PG_SIZES = (21, 22, 43, 200)


def pg_step(w, kind, double, energy=PG_CHOLESKY, extra=(), n=1):
    s = pg_solver(w, kind, double, energy=energy)
    s.set_solver_params({"nIterations": n, "lIterations": 10})
    prm, P = params(w, double)
    prm = prm + list(extra)
    return s, prm, P


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", PG_SIZES)
def test_plan_pose_graph_fp32_backward_error_of_the_steps_solve(N, kind):
    """H from normal_matrix() of the same plan (+ LM's diagonal by the plan's rule at the first
    radius), b from eval_jtf, delta as the change of the unknowns; Higham's bound with the x of
    the bar from numpy's float64 solve."""
    w = arrays(N)
    s, prm, P = pg_step(w, kind, False)
    H, _ = nm.dense_of(*s.normal_matrix(prm))
    r, pre = zeros(3 * N, False), zeros(3 * N, False)
    s.eval_jtf(prm, r, pre)
    b = r.cpu().numpy().astype(np.float64)
    if kind == "LMGPU":
        H = H + np.diag(lm_ctc(H.diagonal().copy(), 1e4))
    x0 = P.cpu().numpy().astype(np.float64).reshape(-1)
    costs = s.profiled_solve(prm)
    assert costs[1] < costs[0]
    delta = P.cpu().numpy().astype(np.float64).reshape(-1) - x0
    info = s.direct_info()
    assert info["n"] == 3 * N and info["factorisations"] == 1 and info["fallbacks"] == 0
    n = 3 * N
    d = np.sqrt(H.diagonal())
    bar = 2 * (3 * n + 1) * U[np.float32] * d * (d @ np.abs(np.linalg.solve(H, b)))
    err = np.abs(H @ delta - b)
    print("N=%d %s: max |H delta - b| / bar = %.3e, min pivot ratio %.3e" % (N, kind, (err / bar).max(), info["min_pivot_ratio"]))
    assert np.all(err <= bar)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", PG_SIZES)
def test_plan_pose_graph_fp64_step_is_the_dense_solve(N, kind):
    w = arrays(N)
    m = model(w)
    ref = kernel_reference(("pg", N), m)
    J, b = ref[4], ref[1]
    H = (J.T @ J).toarray()
    if kind == "LMGPU":
        m.jacobian()                                               # (forms diag_access, the reference's diagonal)
        H = H + np.diag(lm_ctc(m.diag_access.copy(), 1e4))
    want = np.linalg.solve(H, b)
    s, prm, P = pg_step(w, kind, True)
    x0 = P.cpu().numpy().reshape(-1).copy()
    costs = s.profiled_solve(prm)
    assert costs[1] < costs[0]
    delta = P.cpu().numpy().reshape(-1) - x0
    print("N=%d %s: delta %.3e bar %.1e cond %.2e" % (N, kind, rel_err(delta, want), tols(True)[1], np.linalg.cond(H)))
    assert rel_err(delta, want) < tols(True)[1]


_PG_GN = {}


@pytest.mark.parametrize("N", PG_SIZES)
def test_plan_pose_graph_three_gn_steps_match_dense_gauss_newton(N):
    w = arrays(N)
    if N not in _PG_GN:
        m = model(w)
        costs = [m.cost()]
        for _ in range(3):
            J, F = m.jacobian(), m.residuals()
            m.set(m.get() + np.linalg.solve((J.T @ J).toarray(), -(J.T @ F)))
            costs.append(m.cost())
        _PG_GN[N] = costs
    s, prm, _ = pg_step(w, "gaussNewtonGPU", True, n=3)
    costs = s.profiled_solve(prm)
    print("costs", costs, "dense", _PG_GN[N])
    np.testing.assert_allclose(costs, _PG_GN[N], rtol=tols(True)[2])


def dense_lm(m, steps):
    """Levenberg-Marquardt on an oracle model with every linear system solved densely: the
    oracle's loop (oracle/solver_impl.h) — SSq from the first step's diagonal, CtC by lm_ctc at the
    current radius, the model cost without CtC, the accept rule, the radius update in float32
    and the stop at function_tolerance — with numpy's solve in place of PCG. Costs after init
    and after each completed step, as Opt_ProblemCurrentCost reports them."""
    min_rel, ftol, min_radius, max_radius = 1e-3, 1e-6, np.float32(1e-32), np.float32(1e16)
    radius, decrease = np.float32(1e4), np.float32(2.0)
    prev = m.cost()
    costs, ssq = [prev], None
    for _ in range(steps):
        J, F = m.jacobian(), m.residuals()
        diag = m.diag_access.copy()
        if ssq is None:
            ssq = 1.0 / (1.0 + np.sqrt(diag)) ** 2
        rad = float(radius)
        clampm = (1.0 / ssq) / rad
        ctc = np.clip(diag / rad, float(np.float32(1e-6)) * clampm, float(np.float32(1e32)) * clampm)
        d = np.linalg.solve((J.T @ J).toarray() + np.diag(ctc), -(J.T @ F))
        lin = F + J @ d
        model_cost = 0.5 * float(lin @ lin)
        x0 = m.get()
        m.set(x0 + d)
        new = m.cost()
        change, rel = prev - new, (prev - new) / (prev - model_cost)
        if change >= 0 and rel > min_rel:
            if change <= prev * ftol:
                break
            radius = min(np.float32(float(radius) / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3)), max_radius)
            decrease = np.float32(2.0)
            prev = new
        else:
            m.set(x0)
            radius = np.float32(radius / decrease)
            decrease = np.float32(2.0) * decrease
            if radius <= min_radius:
                break
        costs.append(prev)
    return costs


_PG_LM = {}


@pytest.mark.parametrize("N", PG_SIZES)
def test_plan_pose_graph_three_lm_steps_match_dense_levenberg_marquardt(N):
    """Three LM Steps in fp64: accept / revert and the radius update after a direct step, Step
    after Step, against dense_lm on the oracle model."""
    w = arrays(N)
    if N not in _PG_LM:
        _PG_LM[N] = dense_lm(model(w), 3)
    s, prm, _ = pg_step(w, "LMGPU", True, n=3)
    costs = s.profiled_solve(prm)
    print("costs", costs, "dense LM", _PG_LM[N], s.direct_info())
    assert len(costs) == len(_PG_LM[N])
    np.testing.assert_allclose(costs, _PG_LM[N], rtol=tols(True)[2])
    assert s.direct_info()["factorisations"] == len(costs) - 1 and s.direct_info()["fallbacks"] == 0
    assert costs[-1] < 0.2 * costs[0]


def test_plan_pose_graph_an_excluded_pose_stays(tmp_path):
    N = 40
    w = arrays(N)
    mk = np.zeros(N, np.float32)
    mk[7] = 1
    ex = nm.excluded_variant(tmp_path, PG_CHOLESKY, "cholesky_excluded.t")
    ref = kernel_reference(("pg", N), model(w))
    J, b = ref[4], ref[1]
    H = (J.T @ J).toarray()
    act = np.ones(3 * N, bool)
    act[21:24] = False
    want = np.zeros(3 * N)
    want[act] = np.linalg.solve(H[np.ix_(act, act)], b[act])
    s, prm, P = pg_step(w, "gaussNewtonGPU", True, energy=ex, extra=[cuda(mk)])
    x0 = P.cpu().numpy().reshape(-1).copy()
    s.solve(prm)
    x1 = P.cpu().numpy().reshape(-1)
    assert x1[21:24].tobytes() == x0[21:24].tobytes()
    print("delta", rel_err(x1 - x0, want), s.direct_info())
    assert s.direct_info()["factorisations"] == 1
    assert rel_err(x1 - x0, want) < tols(True)[1]


def test_plan_pose_graph_runs_are_bitwise_reproducible():
    out = []
    for _ in range(2):
        s, prm, P = pg_step(arrays(200), "LMGPU", False, n=3)
        out.append((np.array(s.profiled_solve(prm)), P.cpu().numpy().copy()))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


# ====================================================================== RobustEnergy beside the statement
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_plan_huber_bundle_step_is_the_weighted_dense_solve(tmp_path, NC, NP, double):
    """bundle_adjustment_huber.t with Eliminate, ReducedSystem("explicit") and the statement: one GN
    Step against numpy's float64 solve of the reduced system of the weighted J (the robustified
    oracle model of tests/test_robust_gpu.py), with the bars of the plain bundle's Step."""
    from tests import test_robust_gpu as rb
    from tests.test_schur_gpu import linearise
    w = bundle(NC, NP)
    text = open(rb.BA_HUBER).read()
    assert text.count(rb.BLOCK) == 1
    path = tmp_path / "ba_huber_cholesky.t"
    path.write_text(text.replace(rb.BLOCK, rb.BLOCK + '\nEliminate(X)\nReducedSystem("explicit")\nLinearSolver("cholesky")'))
    A, b, _ = linearise(rb.ba_model(w))
    R, pm = reduced_of(w, A, b)
    dr = np.linalg.solve(R.S, R.rhs)
    full = np.zeros(len(b))
    full[pm] = R.back(dr)
    s = rb.ba_solver(w, str(path), "gaussNewtonGPU", double)
    s.set_solver_params({"nIterations": 1, "lIterations": 10})
    prm, unk = rb.ba_params(w, double)
    x0 = unknowns_of(unk)
    s.solve(prm)
    delta = unknowns_of(unk) - x0
    bar = tols(double)[1]
    print("delta_r %.3e full %.3e bar %.1e" % (rel_err(delta[pm][:R.nr], dr), rel_err(delta, full), bar), s.direct_info())
    assert s.direct_info()["factorisations"] == 1 and s.direct_info()["fallbacks"] == 0
    assert rel_err(delta[pm][:R.nr], dr) < bar
    assert rel_err(delta, full) < bar
