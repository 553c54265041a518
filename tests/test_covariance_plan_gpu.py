"""GPU: OptSolver.covariance (OptAMD_Covariance) on plans with LinearSolver("cholesky"), on the
fixtures of tests/test_dense_cholesky_gpu.py.

Truth: the refined float64 inverse (tests/test_covariance_kernels_gpu.py) of the plan's OWN
densified normal_matrix() / reduced_matrix() at the same unknowns, so only the new code is under
test. Bar: max |Sigma - A^-1| <= 2 (n + 1) u kappa_2(A) ||A^-1||_2, as in that file."""
import ctypes

import numpy as np
import pytest

from tests import test_dense_cholesky_gpu as dc
from tests.test_covariance_kernels_gpu import bar_of, block, refined_inverse
from tests.test_dense_cholesky_gpu import (BA_CHOLESKY, BA_SIZES, KINDS, PG_CHOLESKY, PG_SIZES, arrays, bundle, bundle_params,
                                           cholesky_variant, cuda, nm, pg_step, solver, sx, unknowns_of)

pytestmark = pytest.mark.gpu
U = {False: 2.0 ** -24, True: 2.0 ** -53}


def check_blocks(got, pairs, inv, C, bar, what):
    worst = max(np.abs(got[k].astype(np.float64) - block(inv, C, s, t)).max() for k, (s, t) in enumerate(pairs))
    print("%s: max |Sigma - A^-1| / bar = %.3e (bar %.3e)" % (what, worst / bar, bar))
    assert worst <= bar


def ba_plan(w, kind, double, path=BA_CHOLESKY, extra=(), n=3):
    s = solver(w, kind, double, path=path)
    s.set_solver_params({"nIterations": n, "lIterations": 10})
    prm, unk = bundle_params(w, double)
    return s, prm + list(extra), unk


# ====================================================================== accuracy
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", PG_SIZES)
def test_pose_graph_blocks_are_the_inverse_of_the_plans_h(N, kind, double):
    """All diagonal blocks, the pair (0, N - 1) and a pair of neighbours. LM: after one Step, so
    the radius and CtC are live, against the inverse of H without damping."""
    s, prm, _ = pg_step(arrays(N), kind, double, n=3)
    if kind == "LMGPU":
        s.init(prm)
        assert s.step()
    H, _ = nm.dense_of(*s.normal_matrix(prm))
    inv, bar = refined_inverse(H), bar_of(H, U[double])
    diag = s.covariance(prm)
    assert diag.shape == (N, 3, 3) and diag.dtype == (np.float64 if double else np.float32)
    check_blocks(diag, [(e, e) for e in range(N)], inv, 3, bar, "N=%d %s diagonal" % (N, kind))
    pairs = [(0, N - 1), (N // 2, N // 2 + 1), (N - 1, 0)]
    check_blocks(s.covariance(prm, pairs=pairs), pairs, inv, 3, bar, "N=%d %s pairs" % (N, kind))
    some = [N - 1, 0]
    check_blocks(s.covariance(prm, elements=some), [(e, e) for e in some], inv, 3, bar, "N=%d %s elements" % (N, kind))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_bundle_camera_blocks_are_the_inverse_of_the_plans_s(NC, NP, double):
    s, prm, _ = ba_plan(bundle(NC, NP), "gaussNewtonGPU", double)
    S, _ = sx.dense_of(*s.reduced_matrix(prm))
    inv, bar = refined_inverse(S), bar_of(S, U[double])
    check_blocks(s.covariance(prm), [(e, e) for e in range(NC)], inv, 6, bar, "NC=%d diagonal" % NC)
    pairs = [(0, NC - 1), (NC - 1, 0), (1, 2)]
    check_blocks(s.covariance(prm, pairs=pairs), pairs, inv, 6, bar, "NC=%d pairs" % NC)


def test_bundle_lm_plan_leaves_the_damping_out_of_the_eliminated_blocks_too():
    """An LM plan's reduced_matrix() carries LM's diagonal in M_e; covariance() does not: it is
    the inverse of the Gauss-Newton plan's S at the same unknowns."""
    w = bundle(5, 131)
    g, prm, _ = ba_plan(w, "gaussNewtonGPU", True)
    S, _ = sx.dense_of(*g.reduced_matrix(prm))
    s, prm, _ = ba_plan(w, "LMGPU", True)
    inv, bar = refined_inverse(S), bar_of(S, U[True])
    check_blocks(s.covariance(prm), [(e, e) for e in range(5)], inv, 6, bar, "LM plan against the undamped S")


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", BA_SIZES)
def test_huber_bundle_blocks_are_the_inverse_of_the_weighted_s(tmp_path, NC, NP, double):
    from tests import test_robust_gpu as rb
    w = bundle(NC, NP)
    text = open(rb.BA_HUBER).read()
    assert text.count(rb.BLOCK) == 1
    path = tmp_path / "ba_huber_cholesky.t"
    path.write_text(text.replace(rb.BLOCK, rb.BLOCK + '\nEliminate(X)\nReducedSystem("explicit")\nLinearSolver("cholesky")'))
    s = rb.ba_solver(w, str(path), "gaussNewtonGPU", double)
    prm, _ = rb.ba_params(w, double)
    S, _ = sx.dense_of(*s.reduced_matrix(prm))
    inv, bar = refined_inverse(S), bar_of(S, U[double])
    check_blocks(s.covariance(prm), [(e, e) for e in range(NC)], inv, 6, bar, "Huber NC=%d" % NC)


# ====================================================================== inactive elements
def without(A, C, e):
    """(inverse of A with element e's rows and columns deleted, embedded with zeros; its bar)"""
    keep = np.ones(len(A), bool)
    keep[e * C:(e + 1) * C] = False
    sub = A[np.ix_(keep, keep)]
    inv = np.zeros_like(A)
    inv[np.ix_(keep, keep)] = refined_inverse(sub)
    return inv, sub


@pytest.mark.parametrize("double", [False, True])
def test_an_excluded_pose_has_zero_blocks(tmp_path, double):
    N = 40
    mk = np.zeros(N, np.float32)
    mk[7] = 1
    ex = nm.excluded_variant(tmp_path, PG_CHOLESKY, "cholesky_excluded.t")
    s, prm, _ = pg_step(arrays(N), "gaussNewtonGPU", double, energy=ex, extra=[cuda(mk)])
    H, _ = nm.dense_of(*s.normal_matrix(prm))
    inv, sub = without(H, 3, 7)
    bar = bar_of(sub, U[double])
    diag = s.covariance(prm)
    assert np.all(diag[7] == 0)
    check_blocks(diag, [(e, e) for e in range(N)], inv, 3, bar, "excluded pose, diagonal")
    pairs = [(7, 8), (8, 7), (0, 7), (6, 8), (0, N - 1)]
    got = s.covariance(prm, pairs=pairs)
    assert np.all(got[:3] == 0)
    check_blocks(got, pairs, inv, 3, bar, "excluded pose, pairs")


@pytest.mark.parametrize("double", [False, True])
def test_an_excluded_camera_with_held_points_has_zero_blocks(tmp_path, double):
    w = dict(bundle(5, 131))
    w["w_pt"] = 0.0
    mk = np.zeros(w["NC"], np.float32)
    mk[2] = 1
    ch = cholesky_variant(tmp_path, sx.excluded_variant(tmp_path, sx.EXPLICIT), 'ReducedSystem("explicit")')
    s, prm, _ = ba_plan(w, "gaussNewtonGPU", double, path=ch, extra=[cuda(mk)])
    S, _ = sx.dense_of(*s.reduced_matrix(prm))
    inv, sub = without(S, 6, 2)
    bar = bar_of(sub, U[double])
    pairs = [(e, e) for e in range(5)] + [(2, 3), (1, 2), (0, 4)]
    got = s.covariance(prm, pairs=pairs)
    assert np.all(got[2] == 0) and np.all(got[5] == 0) and np.all(got[6] == 0)
    check_blocks(got, pairs, inv, 6, bar, "excluded camera")


# ====================================================================== failures
def test_rank_deficient_raises_with_the_row_and_leaves_the_next_step():
    """w_cam = 0 (Gauss-Newton): the last camera's block of S is zero, the pivot of row 24 fails."""
    w = dict(bundle(5, 131))
    w["w_cam"] = 0.0
    out = []
    for call in (True, False):
        s, prm, unk = ba_plan(w, "gaussNewtonGPU", False, n=1)
        s.init(prm)
        if call:
            with pytest.raises(np.linalg.LinAlgError, match=r"reason=pivot row=24 element=4 channel=0"):
                s.covariance(prm)
            assert s.direct_info()["covariances"] == 0
        s.step()
        out.append((unknowns_of(unk), s.cost()))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1] == out[1][1]


def two_steps(make, call):
    s, prm, unk = make()
    s.init(prm)
    assert s.step()
    if call:
        s.covariance(prm)
    assert s.step()
    return unknowns_of(unk), s.cost(), s.direct_info()["factorisations"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("problem", ["bundle", "pose_graph"])
def test_step_covariance_step_is_step_step(problem, kind):
    if problem == "bundle":
        make = lambda: ba_plan(bundle(70, 9), kind, False, n=4)
    else:
        make = lambda: pg_step(arrays(43), kind, False, n=4)
    a, b = two_steps(make, True), two_steps(make, False)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2] == 2


def test_cap_between_the_tiles_and_the_workspace_is_a_memory_error(monkeypatch):
    s, prm, _ = ba_plan(bundle(70, 9), "LMGPU", False, n=4)
    s.init(prm)
    assert s.step()
    tiles = s.direct_info()["bytes"]
    monkeypatch.setenv("OPT_AMD_DENSE_MAX_BYTES", str(tiles + 1000))
    with pytest.raises(MemoryError, match="reason=memory"):
        s.covariance(prm)
    assert s.step()
    info = s.direct_info()
    assert info["factorisations"] == 2 and info["fallbacks"] == 0 and info["covariances"] == 0
    monkeypatch.delenv("OPT_AMD_DENSE_MAX_BYTES")
    assert s.covariance(prm).shape == (70, 6, 6)                   # the cap is read at each call
    assert s.direct_info()["cov_bytes"] > 1000


@pytest.mark.parametrize("in_place", [False, True])
def test_rewiring_between_steps_matches_a_fresh_plan(in_place):
    """As test_plan_rewiring_between_steps_matches_a_fresh_plan of test_dense_cholesky_gpu.py
    re-wires: the edges in another order and other measurements after the first Step."""
    w = bundle(5, 131)
    sa, prm, unk = ba_plan(w, "gaussNewtonGPU", False, n=4)
    sa.init(prm)
    assert sa.step()
    before = sa.covariance(prm)
    state = [u.cpu().numpy().copy() for u in unk]
    order = np.random.default_rng(3).permutation(w["NO"])
    w2 = dict(w, c=w["c"][order], p=w["p"][order], o=w["o"][order], Obs=dc.f32(w["Obs"] * 1.01),
              CamR=state[0], CamT=state[1], X=state[2])
    prm_b, _ = bundle_params(w2, False)
    for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):          # the priors stay where they were
        prm_b[k] = cuda(w[name])
    if in_place:
        for k in (8, 9, 10, 11):
            prm[k].copy_(prm_b[k])
        got = sa.covariance(prm)
    else:
        prm_a, _ = bundle_params(w2, False)
        for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):
            prm_a[k] = cuda(w[name])
        got = sa.covariance(prm_a)
    sb, _, _ = ba_plan(w, "gaussNewtonGPU", False, n=4)
    want = sb.covariance(prm_b)
    assert got.tobytes() == want.tobytes()
    assert not np.array_equal(got, before)


def test_a_plan_without_the_statement_is_refused_by_name():
    w = bundle(5, 131)
    s, prm, _ = ba_plan(w, "gaussNewtonGPU", False, path=sx.EXPLICIT)
    with pytest.raises(ValueError, match="LinearSolver"):
        s.covariance(prm)
    from opt_amd.api import ParamPack, _ptr
    import torch
    pk = ParamPack(prm)
    r = np.zeros(1, np.int32)
    out = torch.zeros((1, 6, 6), device="cuda")
    assert s.lib.OptAMD_Covariance(s.state, s.plan, pk.ptr, 1, r.ctypes.data, r.ctypes.data, _ptr(out)) == 1
    buf = ctypes.create_string_buffer(256)
    assert s.lib.OptAMD_PlanError(s.plan, buf, 256) > 0 and b"LinearSolver" in buf.value


def test_null_plan_and_bad_index():
    w = bundle(5, 131)
    s, prm, _ = ba_plan(w, "gaussNewtonGPU", False)
    from opt_amd.api import ParamPack, _ptr
    import torch
    pk = ParamPack(prm)
    r = np.zeros(1, np.int32)
    out = torch.full((1, 6, 6), 7.0, device="cuda")
    assert s.lib.OptAMD_Covariance(s.state, None, pk.ptr, 1, r.ctypes.data, r.ctypes.data, _ptr(out)) == -1
    bad = np.array([5], np.int32)
    assert s.lib.OptAMD_Covariance(s.state, s.plan, pk.ptr, 1, bad.ctypes.data, r.ctypes.data, _ptr(out)) == -1
    buf = ctypes.create_string_buffer(256)
    assert s.lib.OptAMD_PlanError(s.plan, buf, 256) > 0 and b"out of range" in buf.value
    assert torch.all(out == 7.0)
    with pytest.raises(ValueError):
        s.covariance(prm, elements=[5])
    with pytest.raises(ValueError):
        s.covariance(prm, pairs=[(0, -1)])


def test_two_calls_agree_bitwise_and_are_counted():
    s, prm, _ = pg_step(arrays(200), "LMGPU", False, n=3)
    a = s.covariance(prm)
    b = s.covariance(prm)
    assert a.tobytes() == b.tobytes()
    info = s.direct_info()
    assert info["covariances"] == 2 and info["cov_bytes"] > 0 and info["n"] == 600
    assert list(info)[:7] == ["n", "tiles", "bytes", "factorisations", "fallbacks", "reason", "min_pivot_ratio"]
