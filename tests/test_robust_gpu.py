"""GPU: RobustEnergy (Huber / Cauchy losses with cached per-edge weights) on the generated
kernels, against the float64 reference of tests/robust_reference.py.

Problems: the pose graphs N = 40, 200 of tests/test_pose_graph_gpu.py under
energies/robust/pose_graph_2d_cauchy.t (Huber by substituting the kind in the file text) at
a = 1.5, and the bundles (5, 131), (70, 9) of tests/test_multispace_gpu.py under
energies/robust/bundle_adjustment_huber.t at a = 0.02 (as the float Param holds it). Before
the data is used the tests assert that at least 10 % of the loss blocks lie on each side of
sqrt(s) = a and none within a relative 1e-3 of it, so fp32 and fp64 take the same Huber
branch at the start; later a flip is harmless (rho and rho' are continuous at a^2).

Tolerances are tols() of tests/test_multispace_gpu.py: fp32 per-unknown outputs within 2e-5
of the largest magnitude, scalars 1e-5 relative, solves 1e-4; fp64 1e-9 / 1e-9 / 1e-8.

LM's teeth: with all steps accepted and the trust region at its lower factor the LM cost
sequence does not depend on the model cost, so beside the a = 1.5 cases the LM solves run
N = 40 under Cauchy at a = 0.5 (82 % of the blocks beyond a), where the float64 reference
with the uncorrected model cost 1/2 |F~ + J~ d|^2 ends 2.8e-4 away from the corrected one:
test_lm_reference_depends_on_the_model_cost asserts that before the GPU is compared."""
import os

import numpy as np
import pytest

from opt_amd import OptSolver, api
from tests import robust_reference as rr
from tests import test_normal_matrix_gpu as nm
from tests import test_schur_explicit_gpu as sx
from tests.test_multispace_gpu import (bundle, bundle_model, bundle_params, check_kernels, cuda, f32, kernel_reference,
                                       rel_err, tols, zeros)
from tests.test_pose_graph_gpu import arrays, model, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = os.path.join(ROOT, "energies", "pose_graph_2d.t")
PG_CAUCHY = os.path.join(ROOT, "energies", "robust", "pose_graph_2d_cauchy.t")
BA_HUBER = os.path.join(ROOT, "energies", "robust", "bundle_adjustment_huber.t")
A_PG = 1.5
A_BA = float(np.float32(0.02))
PG_SIZES = [40, 200]
BA_SIZES = [(5, 131), (70, 9)]
KINDS = ["gaussNewtonGPU", "LMGPU"]
PG_TERM, BA_TERM = 1, 3                  # the constraint / reprojection term of the oracle models
BLOCK = 'UsePreconditioner("block")'


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """Energy files derived from the two shipped ones by substitution, as the existing tests
    derive their block variants."""
    d = tmp_path_factory.mktemp("robust")
    pg, ba = open(PG_CAUCHY).read(), open(BA_HUBER).read()
    assert pg.count('"cauchy", 1.5') == 1 and pg.count("UsePreconditioner(true)") == 1 and ba.count(BLOCK) == 1
    out = {}

    def put(name, text):
        p = d / (name + ".t")
        p.write_text(text)
        out[name] = str(p)

    put("pg_huber", pg.replace('"cauchy", 1.5', '"huber", 1.5'))
    put("pg_cauchy_half", pg.replace('"cauchy", 1.5', '"cauchy", 0.5'))
    put("pg_cauchy_block", pg.replace("UsePreconditioner(true)", BLOCK))
    put("pg_cauchy_normal", pg.replace("UsePreconditioner(true)", 'NormalMatrix("explicit")'))
    put("ba_scalar", ba.replace(BLOCK, "UsePreconditioner(true)"))
    put("ba_schur", ba.replace(BLOCK, BLOCK + "\nEliminate(X)"))
    put("ba_schur_explicit", ba.replace(BLOCK, BLOCK + '\nEliminate(X)\nReducedSystem("explicit")'))
    out["pg_cauchy"], out["ba_block"] = PG_CAUCHY, BA_HUBER
    return out


def pg_energy(variants, kind, a=A_PG):
    return variants[{("cauchy", 1.5): "pg_cauchy", ("huber", 1.5): "pg_huber", ("cauchy", 0.5): "pg_cauchy_half"}[(kind, a)]]


def pg_model(N, kind, a=A_PG):
    return rr.robustify(model(arrays(N)), PG_TERM, kind, a)


def pg_solver(w, energy, kind="gaussNewtonGPU", double=False, **kw):
    return OptSolver([w["N"], w["E"]], energy, kind, double_precision=double, **kw)


def ba_model(w, a=A_BA):
    return rr.robustify(bundle_model(w), BA_TERM, "huber", a)


def ba_params(w, double, a=A_BA, host=False):
    prm, unk = bundle_params(w, double, host=host)
    return prm + [float(a)], unk


def ba_solver(w, energy, kind="gaussNewtonGPU", double=False, **kw):
    return OptSolver([w["NC"], w["NP"], w["NO"]], energy, kind, double_precision=double, **kw)


def scale_splits_the_blocks(m, a):
    """>= 10 % of the loss blocks on each side of sqrt(s) = a, none within a relative 1e-3."""
    q = np.sqrt(m.s()) / a
    above = float((q > 1).mean())
    print("blocks beyond a: %.3f, closest at %.2e" % (above, np.abs(q - 1).min()))
    assert 0.1 <= above <= 0.9 and np.abs(q - 1).min() > 1e-3
    return q > 1


_REF = {}


def robust_reference(key, build):
    """kernel_reference's tuple of the robustified model with the robust cost in place of
    1/2 |F~|^2, and the model (at its start); once per problem."""
    if key not in _REF:
        m = build()
        ref = list(kernel_reference(("robust",) + key, m))
        ref[0] = m.cost()
        _REF[key] = (tuple(ref), m)
    return _REF[key]


def unknowns(unk):
    unk = unk if isinstance(unk, (list, tuple)) else [unk]
    return np.concatenate([np.asarray(u.cpu().numpy() if hasattr(u, "cpu") else u, np.float64).reshape(-1) for u in unk])


# ------------------------------------------------------------------ 1. per kernel
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["huber", "cauchy"])
@pytest.mark.parametrize("N", PG_SIZES)
def test_pose_graph_kernels_match_the_reference(variants, N, kind, double):
    w = arrays(N)
    ref, m = robust_reference(("pg", N, kind), lambda: pg_model(N, kind))
    scale_splits_the_blocks(m, A_PG)
    plain = kernel_reference(("pg", N), model(w))[0]
    assert ref[0] < 0.95 * plain                                   # the loss is in force at the start
    s = pg_solver(w, pg_energy(variants, kind), double=double)
    assert s.family() == "generic"
    assert s.loss_groups() == [{"graph": 0, "residuals": 3, "kind": kind, "edges": w["E"]}]
    check_kernels(s, params(w, double)[0], ref, double, seed=N)


def block_solve(H, r, index):
    """z with z[idx] = H[idx, idx]^-1 r[idx] for every row idx of `index`."""
    z = np.zeros(len(r))
    for idx in index:
        z[idx] = np.linalg.solve(H[np.ix_(idx, idx)], r[idx])
    return z


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_bundle_kernels_and_block_preconditioner_match_the_reference(NC, NP, double):
    w = bundle(NC, NP)
    ref, m = robust_reference(("ba", NC, NP), lambda: ba_model(w))
    scale_splits_the_blocks(m, A_BA)
    s = ba_solver(w, BA_HUBER, double=double)
    assert s.family() == "generic" and s.preconditioner_blocks() == ([0, 0, 1], [0, 3, 0], 2)
    assert s.loss_groups() == [{"graph": 0, "residuals": 2, "kind": "huber", "edges": w["NO"]}]
    prm, _ = ba_params(w, double)
    r, _, _ = check_kernels(s, prm, ref, double, seed=NC)
    # z = M^-1 r with M the diagonal blocks of the weighted J^T J: 6 x 6 per camera, 3 x 3 per point
    H = (ref[4].T @ ref[4]).toarray()
    cams = [np.r_[3 * c:3 * c + 3, 3 * NC + 3 * c:3 * NC + 3 * c + 3] for c in range(NC)]
    pts = [np.arange(6 * NC + 3 * p, 6 * NC + 3 * p + 3) for p in range(NP)]
    n = len(ref[1])
    rv = np.random.default_rng(NP).normal(size=n).astype(np.float64 if double else np.float32)
    z = zeros(n, double)
    s.apply_preconditioner(prm, cuda(rv), z)
    z_ref = block_solve(H, rv.astype(np.float64), cams + pts)
    print("z", rel_err(z.cpu().numpy(), z_ref), "bar", tols(double)[0])
    assert rel_err(z.cpu().numpy(), z_ref) < tols(double)[0]


# ------------------------------------------------------------------ 2. rho'(s) per edge
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_loss_weights_on_the_pose_graph(variants, kind, double):
    N = 200
    w = arrays(N)
    m = pg_model(N, kind)
    beyond = scale_splits_the_blocks(m, A_PG)
    s = pg_solver(w, pg_energy(variants, kind), double=double)
    prm, unk = params(w, double)
    got = s.loss_weights(prm).cpu().numpy()
    assert got.shape == (w["E"],) and got.dtype == (np.float64 if double else np.float32)
    print("rho' at the start", rel_err(got, m.loss_rho1()))
    assert rel_err(got, m.loss_rho1()) < tols(double)[0]
    inside = (got > 0) & (got < 1)
    if kind == "huber":
        assert np.array_equal(inside, beyond) and (got[~beyond] == 1).all()
    else:
        assert inside[beyond].all() and (got <= 1).all() and (got > 0).all()
    # after a solve: at the unknowns the plan ended on
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    s.solve(prm)
    m.set(unknowns(unk))
    after = s.loss_weights(prm).cpu().numpy()
    print("rho' after the solve", rel_err(after, m.loss_rho1()), "moved by", np.abs(after - got).max())
    assert rel_err(after, m.loss_rho1()) < tols(double)[0]
    assert np.abs(after - got).max() > 0.1 and after.mean() > got.mean()       # most constraints became inliers
    with pytest.raises(api.OptError, match="loss group 1 of 1"):
        s.loss_weights(prm, group=1)


@pytest.mark.parametrize("double", [False, True])
def test_param_scale_is_read_again_between_steps(double):
    """The Huber scale is a Param: changed between two Steps, with no new plan, the weights and
    the next Step are those of the new scale; a scale <= 0 stops the solve by name."""
    w = bundle(5, 131)
    m = ba_model(w)
    beyond = scale_splits_the_blocks(m, A_BA)
    sa = ba_solver(w, BA_HUBER, double=double)
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = ba_params(w, double)
    w0 = sa.loss_weights(prm).cpu().numpy()
    assert rel_err(w0, m.loss_rho1()) < tols(double)[0]
    assert np.array_equal((w0 > 0) & (w0 < 1), beyond)
    sa.init(prm)
    assert sa.step()
    state = [u.cpu().numpy().copy() for u in unk]
    narrow = float(np.float32(0.05 * A_BA))                          # (after a step every block lies inside a = 0.02)
    prm_a = prm[:-1] + [narrow]
    m.set(unknowns(unk))
    w1 = sa.loss_weights(prm).cpu().numpy()
    m.loss[0]["a"] = narrow
    w2 = sa.loss_weights(prm_a).cpu().numpy()
    print("rho' at the new scale", rel_err(w2, m.loss_rho1()), "changed on", int((w1 != w2).sum()), "edges")
    assert rel_err(w2, m.loss_rho1()) < tols(double)[0]
    assert (w1 == 1).all() and (w2 <= w1).all() and (w2 < 0.95).sum() >= 5
    assert sa.step(prm_a)
    sb = ba_solver(w, BA_HUBER, double=double)
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    T = np.float64 if double else np.float32
    prm_b, unk_b = ba_params(dict(w, CamR=state[0].astype(T), CamT=state[1].astype(T), X=state[2].astype(T)), double, a=narrow)
    for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):          # the priors stay where they were
        prm_b[k] = cuda(w[name])
    for a_, b_ in zip(unk_b, state):
        assert a_.cpu().numpy().tobytes() == b_.tobytes()
    sb.init(prm_b)
    assert sb.step()
    for a_, b_, c_ in zip(unk, unk_b, state):
        assert a_.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes()
        assert not np.array_equal(a_.cpu().numpy(), c_)
    assert sa.cost() == sb.cost()
    for bad in (0.0, -0.02, float("nan")):
        sc = ba_solver(w, BA_HUBER, double=double)
        with pytest.raises(api.OptError, match="the scale Param 'huber' is"):
            sc.init(ba_params(w, double, a=bad)[0])
        assert sc.lib.Opt_ProblemStep(sc.state, sc.plan, sc._pk.ptr) == 0


# ------------------------------------------------------------------ 3. whole solves
PG_SOLVES = [(40, "huber", 1.5), (200, "cauchy", 1.5), (40, "cauchy", 0.5)]
_SOLVE = {}


def reference_costs(key, build, lm, corrected=True):
    k = key + (lm, corrected)
    if k not in _SOLVE:
        _SOLVE[k] = rr.solve(build(), 3, 10, lm=lm, corrected=corrected)
    return _SOLVE[k]


def test_lm_reference_depends_on_the_model_cost():
    """The reference's LM sequence without rho - rho' s in the model cost differs from the
    corrected one by more than the bar of the fp32 solves on at least one case the GPU runs."""
    worst = 0.0
    for N, kind, a in PG_SOLVES:
        seq = [reference_costs(("pg", N, kind, a), lambda: pg_model(N, kind, a), True, c) for c in (True, False)]
        d = np.inf if len(seq[0]) != len(seq[1]) else float(np.abs(seq[0] / seq[1] - 1).max())
        print(N, kind, a, "corrected", seq[0], "uncorrected", seq[1], "apart by", d)
        worst = max(worst, d)
    assert worst > 2 * tols(False)[2]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("solver_kind", KINDS)
@pytest.mark.parametrize("N,kind,a", PG_SOLVES)
def test_pose_graph_solves_match_the_reference(variants, N, kind, a, solver_kind, double):
    w = arrays(N)
    q = np.sqrt(pg_model(N, kind, a).s()) / a
    assert 0.1 <= (q > 1).mean() <= 0.9 and np.abs(q - 1).min() > 1e-3
    s = pg_solver(w, pg_energy(variants, kind, a), solver_kind, double)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    costs = s.profiled_solve(params(w, double)[0])
    ref = reference_costs(("pg", N, kind, a), lambda: pg_model(N, kind, a), solver_kind == "LMGPU")
    print("costs", costs, "reference", list(ref))
    assert len(costs) == len(ref)                                  # the same steps accepted
    np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])
    assert costs[-1] < 0.2 * costs[0]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("solver_kind", KINDS)
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_bundle_solves_match_the_reference(variants, NC, NP, solver_kind, double):
    """The scalar-preconditioner variant: the reference's PCG is preconditioned that way."""
    w = bundle(NC, NP)
    s = ba_solver(w, variants["ba_scalar"], solver_kind, double)
    assert s.preconditioner_blocks() == ([], [], 0)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    costs = s.profiled_solve(ba_params(w, double)[0])
    ref = reference_costs(("ba", NC, NP), lambda: ba_model(w), solver_kind == "LMGPU")
    print("costs", costs, "reference", list(ref))
    assert len(costs) == len(ref)
    np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])
    assert costs[-1] < 0.2 * costs[0]


# ------------------------------------------------------------------ 4. the Huber bundle's variants
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_bundle_variants_reach_the_same_iterates(variants, NC, NP, double):
    """Block preconditioner, Eliminate(X) and Eliminate(X) + ReducedSystem("explicit") solve the
    same weighted normal equations, by different PCG iterations (on the full system and on the
    Schur complement): their iterates agree where the linear solves have converged. In fp64 that
    is 100 PCG iterations: the preconditioned operators have at most 2 min(6 NC, 3 NP) + 1 <= 61
    distinct eigenvalues, so PCG has terminated by then. fp32 cannot run that long: once PCG has
    terminated exactly its next step divides 0 by 0, so fp32 runs 20 iterations (fewer than the
    28 at which the smaller Schur complement terminates), which leaves the block plan's first
    step 6e-6 (5, 131) and 4e-5 (70, 9) from the Schur plans', inside fp32's bar of 1e-4.
    The scalar variant solves the same problem and ends on the same cost."""
    w = bundle(NC, NP)
    costs = {}
    for name in ("ba_block", "ba_schur", "ba_schur_explicit", "ba_scalar"):
        s = ba_solver(w, variants[name], double=double)
        assert s.eliminated() == ([0, 0, 0] if name in ("ba_block", "ba_scalar") else [0, 0, 1])
        s.set_solver_params({"nIterations": 3, "lIterations": 100 if double else 20})
        costs[name] = np.array(s.profiled_solve(ba_params(w, double)[0]))
        print(name, costs[name])
        assert len(costs[name]) == 4 and costs[name][-1] < 0.2 * costs[name][0]
    for name in ("ba_schur", "ba_schur_explicit"):
        np.testing.assert_allclose(costs[name], costs["ba_block"], rtol=tols(double)[2])
    assert costs["ba_scalar"][0] == costs["ba_block"][0]
    assert costs["ba_scalar"][-1] == pytest.approx(costs["ba_block"][-1], rel=tols(double)[2])


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("solver_kind", KINDS)
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_reduced_matrix_is_the_weighted_schur_complement(variants, monkeypatch, NC, NP, solver_kind, double):
    w = bundle(NC, NP)
    monkeypatch.setattr(sx, "EXPLICIT", variants["ba_schur_explicit"])
    monkeypatch.setattr(sx, "bundle_params", lambda w_, d_: ba_params(w_, d_))
    sx.check_matrix(w, solver_kind, double, model=ba_model(w))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("N", PG_SIZES)
def test_normal_matrix_is_the_weighted_jtj(variants, N, double):
    w = arrays(N)
    ref, _ = robust_reference(("pg", N, "cauchy"), lambda: pg_model(N, "cauchy"))
    s = pg_solver(w, variants["pg_cauchy_normal"], double=double)
    prm, _ = params(w, double)
    nm.check_matrix(s, prm, ref[4], nm.graph_pattern(N, w["i"], w["j"]), double)
    nm.check_apply(s, prm, ref[4], double, seed=N)
    # and whole solves on H: the block variant's iterates
    out = {}
    for name in ("pg_cauchy_normal", "pg_cauchy_block"):
        sv = pg_solver(w, variants[name], double=double)
        sv.set_solver_params({"nIterations": 3, "lIterations": 10})
        out[name] = np.array(sv.profiled_solve(params(w, double)[0]))
    print(out)
    np.testing.assert_allclose(out["pg_cauchy_normal"], out["pg_cauchy_block"], rtol=tols(double)[2])


# ------------------------------------------------------------------ 5. the Step boundary
@pytest.mark.parametrize("name", ["ba_block", "ba_schur_explicit"])
def test_obs_rewritten_in_place_between_steps_matches_a_fresh_plan(variants, name):
    w = bundle(5, 131)
    sa = ba_solver(w, variants[name])
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = ba_params(w, False)
    sa.init(prm)
    assert sa.step()
    state = [u.cpu().numpy().copy() for u in unk]
    obs2 = f32(w["Obs"] + np.random.default_rng(5).normal(0, 0.01, w["Obs"].shape))
    w_before = sa.loss_weights(prm).cpu().numpy()
    prm[8].copy_(cuda(obs2))                                       # the same device array, rewritten
    assert np.abs(sa.loss_weights(prm).cpu().numpy() - w_before).max() > 0.1
    assert sa.step()
    sb = ba_solver(w, variants[name])
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm_b, unk_b = ba_params(dict(w, Obs=obs2, CamR=state[0], CamT=state[1], X=state[2]), False)
    for k, nm_ in zip((5, 6, 7), ("CamR", "CamT", "X")):
        prm_b[k] = cuda(w[nm_])
    sb.init(prm_b)
    assert sb.step()
    for a_, b_, c_ in zip(unk, unk_b, state):
        assert a_.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes()
        assert not np.array_equal(a_.cpu().numpy(), c_)
    assert sa.cost() == sb.cost()


@pytest.mark.parametrize("name", ["pg_cauchy", "pg_cauchy_normal"])
def test_graph_rewired_in_place_between_steps_matches_a_fresh_plan(variants, name):
    """The vertex arrays rewritten in place: incidence lists, inverse positions and weights are
    rebuilt, and the second Step is a fresh plan's first."""
    N = 40
    w = arrays(N)
    w2 = nm.rewired(w)
    sa = pg_solver(w, variants[name])
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = params(w, False)
    sa.init(prm)
    assert sa.step()
    state = unk.cpu().numpy().copy()
    for k, key in zip((4, 5, 6, 7, 8), ("Z", "U0", "U1", "i", "j")):
        prm[k].copy_(cuda(w2[key]))
    assert sa.step()
    sb = pg_solver(w, variants[name])
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm_b, unk_b = params(dict(w2, P=state), False)
    prm_b[2] = cuda(w["P0"])
    sb.init(prm_b)
    assert sb.step()
    assert unk.cpu().numpy().tobytes() == unk_b.cpu().numpy().tobytes()
    assert not np.array_equal(unk.cpu().numpy(), state)
    assert sa.cost() == sb.cost()
    assert sa.loss_weights(prm).cpu().numpy().tobytes() == sb.loss_weights(prm_b).cpu().numpy().tobytes()


# ------------------------------------------------------------------ 6. determinism, backends
def test_solves_are_bitwise_reproducible():
    w, b = arrays(200), bundle(5, 131)
    out = []
    for _ in range(2):
        s = pg_solver(w, PG_CAUCHY, "LMGPU")
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = params(w, False)
        c1 = s.profiled_solve(prm)
        s2 = ba_solver(b, BA_HUBER, "LMGPU")
        s2.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm2, unk2 = ba_params(b, False)
        c2 = s2.profiled_solve(prm2)
        out.append((np.array(c1 + c2), unknowns(unk), unknowns(unk2)))
    for a_, b_ in zip(out[0], out[1]):
        assert a_.tobytes() == b_.tobytes()
    assert not np.array_equal(out[0][1], w["P"].reshape(-1).astype(np.float64))


def test_backend_cpu_with_host_arrays_equals_backend_cuda():
    w, b = arrays(200), bundle(5, 131)
    res = {}
    for backend in ("backend_cuda", "backend_cpu"):
        host = backend == "backend_cpu"
        s = pg_solver(w, PG_CAUCHY, backend=backend)
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = params(w, False, host=host)
        c1 = s.solve(prm)
        s2 = ba_solver(b, BA_HUBER, backend=backend)
        s2.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm2, unk2 = ba_params(b, False, host=host)
        c2 = s2.solve(prm2)
        res[backend] = (c1, c2, unknowns(unk), unknowns(unk2))
    assert res["backend_cpu"][:2] == res["backend_cuda"][:2]
    for k in (2, 3):
        assert res["backend_cpu"][k].tobytes() == res["backend_cuda"][k].tobytes()
    assert not np.array_equal(res["backend_cpu"][2], w["P"].reshape(-1).astype(np.float64))   # written back


# ------------------------------------------------------------------ 7. the entry points on other plans
def test_entry_points_on_other_plans(capfd):
    w = arrays(40)
    s = pg_solver(w, PG)
    prm, _ = params(w, False)
    s.init(prm)
    assert s.loss_groups() == []
    out = zeros(w["E"], False)
    assert s.lib.OptAMD_EvalLossWeights(s.state, s.plan, api.ParamPack(prm).ptr, 0, api._ptr(out)) == 1
    with pytest.raises(api.OptError, match="OptAMD_EvalLossWeights failed"):
        s.loss_weights(prm)
    assert s.lib.OptAMD_PlanLossGroups(None, 4, None, None, None) == -1
    assert s.lib.OptAMD_PlanLossGroupEdges(s.plan, 0) == -1
    for kw in ({"materialized": True}, {"materialized": True, "fused_jtj": True}):
        capfd.readouterr()
        with pytest.raises(api.OptError, match="Opt_ProblemPlan failed"):
            pg_solver(w, PG_CAUCHY, **kw)
        assert "useMaterializedJTJ / useFusedJTJ) with RobustEnergy" in capfd.readouterr().err
    r = pg_solver(w, PG_CAUCHY)
    assert r.jacobian_shape()[1] == -1
    import torch
    rp = torch.zeros(16, dtype=torch.int32, device="cuda")
    capfd.readouterr()
    with pytest.raises(api.OptError, match="OptAMD_EvalJacobian failed"):
        r.eval_jacobian(prm, rp, rp, torch.zeros(16, device="cuda"))
    assert "no Jacobian assembly (OptAMD_EvalJacobian) for an energy with a RobustEnergy statement" in capfd.readouterr().err
