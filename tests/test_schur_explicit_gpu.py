"""GPU: ReducedSystem("explicit") — the Schur complement S = B - E M^-1 E^T of bundle
adjustment's points assembled in block-CSR (energies/bundle_adjustment_schur_explicit.t) and
PCG on a block SpMV, against the float64 AD oracle's dense S (tests/test_schur_gpu.py: Reduced)
and against the matrix-free plan of energies/bundle_adjustment_schur.t.

Sizes (5, 131) and (70, 9) of tests/test_schur_gpu.py: camera 0 sees every point (a block row
of 5 / 70 blocks: below and above one 64-lane wave of entries), the last camera sees none (its
row is its diagonal block alone), point NP-1 is seen once. Tolerances are that file's tols():
matrices and vectors within 2e-5 (fp32) / 1e-9 (fp64) of the largest entry; the float32 numpy
restatement of S on these fixtures is off by at most 2.2e-7, so fp32 itself is no obstacle."""
import os

import numpy as np
import pytest

from opt_amd import api
from tests.test_schur_gpu import (SIZES, bundle, bundle_model, bundle_params, cuda, f32, linearise, lm_ctc, reduced_of,
                                  rel_err, solver, start_system, tols, unknowns_of, zeros)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPLICIT = os.path.join(ROOT, "energies", "bundle_adjustment_schur.t")
EXPLICIT = os.path.join(ROOT, "energies", "bundle_adjustment_schur_explicit.t")
KINDS = ["gaussNewtonGPU", "LMGPU"]


def expected_pattern(w):
    """Cameras that share a point, and every diagonal block: (NC, NC) bool."""
    D = np.zeros((w["NC"], w["NP"]))
    np.add.at(D, (w["c"], w["p"]), 1)
    return ((D @ D.T) > 0) | np.eye(w["NC"], dtype=bool)


def dense_of(row_ptr, col_ind, val):
    rp, ci, v = row_ptr.cpu().numpy(), col_ind.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    n, C = len(rp) - 1, v.shape[1]
    S, pat = np.zeros((n * C, n * C)), np.zeros((n, n), bool)
    for r in range(n):
        assert list(ci[rp[r]:rp[r + 1]]) == sorted(set(ci[rp[r]:rp[r + 1]]))     # ascending, no duplicates
        for k in range(rp[r], rp[r + 1]):
            S[r * C:(r + 1) * C, ci[k] * C:(ci[k] + 1) * C] = v[k]
            pat[r, ci[k]] = True
    return S, pat


def check_matrix(w, kind, double, model=None):
    A, b, diag = linearise(model) if model is not None else start_system(w["NC"], w["NP"])
    add = lm_ctc(diag, 1e4) if kind == "LMGPU" else None
    R, pm = reduced_of(w, A, b, add=add)
    S_ref = R.S - (np.diag(add[pm][:R.nr]) if add is not None else 0.0)       # LM's retained diagonal: the apply's
    s = solver(w, kind, double, path=EXPLICIT)
    assert s.reduced_matrix_shape() is None                                  # nothing bound yet
    prm, _ = bundle_params(w, double)
    S, pat = dense_of(*s.reduced_matrix(prm))
    assert s.reduced_matrix_shape() == (w["NC"], 6, int(pat.sum()))
    want = expected_pattern(w)
    assert np.array_equal(pat, want)
    assert not S_ref[~np.kron(want, np.ones((6, 6), bool))].any()            # the oracle's S has no other block
    big = np.abs(S_ref).max()
    worst = max(np.abs(S[6 * r:6 * r + 6, 6 * c:6 * c + 6] - S_ref[6 * r:6 * r + 6, 6 * c:6 * c + 6]).max()
                for r, c in zip(*np.nonzero(want)))
    print("S: worst block error %.3e of the largest entry, bar %.1e, %d blocks" % (worst / big, tols(double)[0], pat.sum()))
    assert worst / big < tols(double)[0]
    return s


# ------------------------------------------------------------------ (a) the assembled matrix
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("NC,NP", SIZES)
def test_reduced_matrix_is_the_oracles_schur_complement(NC, NP, kind, double):
    check_matrix(bundle(NC, NP), kind, double)


def test_entry_points_on_other_plans():
    w = bundle(5, 131)
    s = solver(w, path=IMPLICIT)
    prm, _ = bundle_params(w, False)
    s.init(prm)
    assert s.reduced_matrix_shape() is None
    with pytest.raises(api.OptError, match="OptAMD_ReducedMatrix failed"):
        s.reduced_matrix(prm)
    assert s.lib.OptAMD_PlanReducedMatrixShape(None, None, None, None) == -1


# ------------------------------------------------------------------ (b) the reduced apply
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("NC,NP", SIZES)
def test_reduced_apply_on_an_explicit_plan(NC, NP, kind, double):
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
    s = solver(w, kind, double, path=EXPLICIT)
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
    print("S p", rel_err(out[0], Sp_ref), "bar", tols(double)[0])
    assert rel_err(out[0], Sp_ref) < tols(double)[0]
    assert not out[0][nr:].any()
    assert out[0].tobytes() == out[1].tobytes() == out[2].tobytes()


# ------------------------------------------------------------------ (c) duplicated observations
def with_duplicates(w, k=6):
    """k observations measured twice: the same (camera, point) edge again, with its own Obs row."""
    idx = np.random.default_rng(11).choice(w["NO"], k, replace=False)
    v = dict(w)
    v["c"], v["p"] = np.concatenate([w["c"], w["c"][idx]]), np.concatenate([w["p"], w["p"][idx]])
    v["o"] = np.concatenate([w["o"], np.arange(w["NO"], w["NO"] + k, dtype=np.int32)])
    v["Obs"] = f32(np.concatenate([w["Obs"], w["Obs"][w["o"][idx]] + 1e-3]))
    v["NO"] = w["NO"] + k
    return v


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_duplicated_observations_are_more_pairs(NC, NP, double):
    w = with_duplicates(bundle(NC, NP))
    assert len(set(zip(w["c"].tolist(), w["p"].tolist()))) == w["NO"] - 6
    check_matrix(w, "gaussNewtonGPU", double, model=bundle_model(w))


# ------------------------------------------------------------------ (d) whole solves
def three_steps(w, kind, double, path, prm_extra=()):
    s = solver(w, kind, double, path=path)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = bundle_params(w, double)
    costs = s.profiled_solve(prm + list(prm_extra))
    return np.array(costs), unknowns_of(unk), [u.cpu().numpy() for u in unk]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("NC,NP", SIZES)
def test_solves_match_the_matrix_free_plan(NC, NP, kind, double):
    w = bundle(NC, NP)
    ce, xe, _ = three_steps(w, kind, double, EXPLICIT)
    ci, xi, _ = three_steps(w, kind, double, IMPLICIT)
    print("costs explicit", ce, "implicit", ci, "unknowns", rel_err(xe, xi))
    assert len(ce) == len(ci) == 4
    np.testing.assert_allclose(ce, ci, rtol=tols(double)[2])
    assert ce[-1] < 0.2 * ce[0]
    if double:
        assert rel_err(xe, xi) < 1e-8


# ------------------------------------------------------------------ (e) held points, an excluded camera
def excluded_variant(tmp_path, path):
    text = open(path).read()
    assert text.count("UsePreconditioner(true)") == 1
    text = text.replace("UsePreconditioner(true)",
                        'local Mk = Array("Mk", opt_float, {NC}, 12)\nExclude(eq(Mk(0), 1))\nUsePreconditioner(true)')
    out = tmp_path / os.path.basename(path)
    out.write_text(text)
    return str(out)


@pytest.mark.parametrize("double", [False, True])
def test_held_points_and_an_excluded_camera(tmp_path, double):
    """w_pt = 0 holds the points seen once (M^-1 = 0: Y = 0, their pairs add nothing); camera 2
    is excluded (its row of S p is 0, its unknowns stay). Expected: the matrix-free plan's."""
    w = dict(bundle(5, 131))
    w["w_pt"] = 0.0
    assert (np.bincount(w["p"], minlength=w["NP"]) == 1).any()
    mk = np.zeros(w["NC"], np.float32)
    mk[2] = 1
    res = {}
    for name, path in (("explicit", EXPLICIT), ("implicit", IMPLICIT)):
        res[name] = three_steps(w, "gaussNewtonGPU", double, excluded_variant(tmp_path, path), prm_extra=[cuda(mk)])
    (ce, xe, ue), (ci, xi, ui) = res["explicit"], res["implicit"]
    print("costs explicit", ce, "implicit", ci, "unknowns", rel_err(xe, xi))
    np.testing.assert_allclose(ce, ci, rtol=tols(double)[2])
    T = np.float64 if double else np.float32
    for k, name in enumerate(("CamR", "CamT")):
        assert ue[k][2].tobytes() == w[name][2].astype(T).tobytes()          # the excluded camera did not move
    once = np.flatnonzero(np.bincount(w["p"], minlength=w["NP"]) == 1)
    assert ue[2][once].tobytes() == w["X"][once].astype(T).tobytes()          # nor did the held points
    assert rel_err(xe, xi) < (1e-8 if double else 1e-4)


# ------------------------------------------------------------------ (f) determinism
def test_explicit_solves_are_bitwise_reproducible():
    w = bundle(70, 9)
    out = [three_steps(w, "LMGPU", False, EXPLICIT) for _ in range(2)]
    assert out[0][0].tobytes() == out[1][0].tobytes()
    for a, b in zip(out[0][2], out[1][2]):
        assert a.tobytes() == b.tobytes()
    assert out[0][0][-1] < 0.2 * out[0][0][0]


# ------------------------------------------------------------------ (g) the Step boundary
def rewired(w):
    """Another wiring: the camera that saw nothing takes over five observations, and the edges
    come in another order."""
    order = np.random.default_rng(3).permutation(w["NO"])
    c = w["c"][order].copy()
    c[:5] = w["NC"] - 1
    return dict(w, c=c, p=w["p"][order], o=w["o"][order])


@pytest.mark.parametrize("in_place", [False, True])
def test_rewiring_between_steps_matches_a_fresh_plan(in_place):
    w = bundle(5, 131)
    w2 = rewired(w)
    assert not np.array_equal(expected_pattern(w), expected_pattern(w2))
    sa = solver(w, path=EXPLICIT)
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = bundle_params(w, False)
    sa.init(prm)
    assert sa.step()
    assert np.array_equal(dense_of(*sa.reduced_matrix(prm))[1], expected_pattern(w))
    state = [u.cpu().numpy().copy() for u in unk]
    if in_place:                                                   # the same device arrays, rewritten
        prm_a, unk_a = prm, unk
        for k, name in zip((9, 10, 11), ("c", "p", "o")):
            prm_a[k].copy_(cuda(w2[name]))
    else:                                                          # other arrays bound
        prm_a, unk_a = bundle_params(dict(w2, CamR=state[0], CamT=state[1], X=state[2]), False)
        for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):      # the priors stay where they were
            prm_a[k] = cuda(w[name])
    assert sa.step(prm_a)
    sb = solver(w, path=EXPLICIT)
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm_b, unk_b = bundle_params(dict(w2, CamR=state[0], CamT=state[1], X=state[2]), False)
    for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):
        prm_b[k] = cuda(w[name])
    sb.init(prm_b)
    assert sb.step()
    for a, b, c in zip(unk_a, unk_b, state):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert not np.array_equal(a.cpu().numpy(), c)
    assert sa.cost() == sb.cost()
    Sa, pat_a = dense_of(*sa.reduced_matrix(prm_a))
    Sb, pat_b = dense_of(*sb.reduced_matrix(prm_b))
    assert np.array_equal(pat_a, expected_pattern(w2)) and np.array_equal(pat_b, pat_a)
    assert Sa.tobytes() == Sb.tobytes()
