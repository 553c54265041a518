"""GPU: NormalMatrix("explicit") — H = J^T J assembled in block-CSR
(energies/normal_matrix/pose_graph_2d_explicit.t) and PCG on the short-row block SpMV, against
the dense J^T J of the float64 AD oracle (tests/test_pose_graph_gpu.py: model) and against the
matrix-free plan of the UsePreconditioner("block") variant, whose preconditioner the statement
turns on.

Tolerances are tests/test_multispace_gpu.py's tols(): matrices and vectors within 2e-5 (fp32) /
1e-9 (fp64) of the largest entry, solves' costs 1e-4 / 1e-8. Sizes: N = 21 fills the 21 rows a
wave serves for 3 x 3 blocks exactly, N = 22 spills one row into the next wave; 40 and 200 are
the pose-graph fixtures (200: several waves, still one workgroup of 84 rows short of three)."""
import os

import numpy as np
import pytest

from opt_amd import OptSolver, api
from oracle import examples_ad as ad
from tests.test_multispace_gpu import cuda, f32, kernel_reference, rel_err, tols, zeros
from tests.test_pose_graph_gpu import PG, arrays, model, oracle_costs, params, solver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPLICIT = os.path.join(ROOT, "energies", "normal_matrix", "pose_graph_2d_explicit.t")
STATEMENT = 'NormalMatrix("explicit")'
KINDS = ["gaussNewtonGPU", "LMGPU"]
LONG_ROW, LONG_PAIRS = 64, 128         # gen::kNormalLongRow, gen::kSchurLongPairs


@pytest.fixture(scope="module")
def block_energy(tmp_path_factory):
    text = open(PG).read()
    assert text.count("UsePreconditioner(true)") == 1
    p = tmp_path_factory.mktemp("normal") / "pose_graph_2d_block.t"
    p.write_text(text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    return str(p)


def dense_of(row_ptr, col_ind, val, index=None):
    """The block-CSR matrix as a dense one in the unknown vector's layout: index[e, j] is the
    place of block row j of element e (default: one image, e * C + j)."""
    rp, ci, v = row_ptr.cpu().numpy(), col_ind.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    n, C = len(rp) - 1, v.shape[1]
    if index is None:
        index = np.arange(n * C).reshape(n, C)
    H, pat = np.zeros((n * C, n * C)), np.zeros((n, n), bool)
    for r in range(n):
        assert list(ci[rp[r]:rp[r + 1]]) == sorted(set(ci[rp[r]:rp[r + 1]]))     # ascending, no duplicates
        for k in range(rp[r], rp[r + 1]):
            H[np.ix_(index[r], index[ci[k]])] = v[k]
            pat[r, ci[k]] = True
    return H, pat


def graph_pattern(n, *slots):
    """Elements that share an edge, and every diagonal block."""
    pat = np.eye(n, dtype=bool)
    for a in slots:
        for b in slots:
            pat[a, b] = True
    return pat


def check_matrix(s, prm, J, want, double, index=None):
    """normal_matrix() against J^T J block by block; returns the dense H."""
    H_ref = (J.T @ J).toarray()
    H, pat = dense_of(*s.normal_matrix(prm), index=index)
    n = len(want)
    C = H.shape[0] // n
    if index is None:
        index = np.arange(n * C).reshape(n, C)
    assert s.normal_matrix_shape() == (n, C, int(pat.sum()))
    assert np.array_equal(pat, want)
    mask = np.zeros_like(H_ref, bool)
    for r, c in zip(*np.nonzero(want)):
        mask[np.ix_(index[r], index[c])] = True
    assert not H_ref[~mask].any()                                            # the oracle's J^T J has no other block
    big = np.abs(H_ref).max()
    worst = max(np.abs(H[np.ix_(index[r], index[c])] - H_ref[np.ix_(index[r], index[c])]).max()
                for r, c in zip(*np.nonzero(want)))
    print("H: worst block error %.3e of the largest entry, bar %.1e, %d blocks" % (worst / big, tols(double)[0], pat.sum()))
    assert worst / big < tols(double)[0]
    return H


def check_apply(s, prm, J, double, seed, active=None):
    n = J.shape[1]
    p = np.random.default_rng(seed).normal(size=n).astype(np.float64 if double else np.float32)
    Ap = zeros(n, double)
    Ap += 7.0
    pAp = s.apply_jtj(prm, cuda(p), Ap)
    ref = J.T @ (J @ p.astype(np.float64))
    if active is not None:
        ref = ref * active
    print("H p", rel_err(Ap.cpu().numpy(), ref), "bar", tols(double)[0])
    assert rel_err(Ap.cpu().numpy(), ref) < tols(double)[0]
    assert pAp == pytest.approx(float(p.astype(np.float64) @ ref), rel=10 * tols(double)[1])
    return Ap.cpu().numpy()


# ------------------------------------------------------------------ 1. H against the dense J^T J
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [40, 200])
def test_normal_matrix_is_the_oracles_jtj(N, kind, double):
    w = arrays(N)
    s = solver(w, kind, double, energy=EXPLICIT)
    assert s.family() == "generic" and s.preconditioner_blocks() == ([0], [0], 1)
    assert s.normal_matrix_shape() is None                                   # nothing bound yet
    prm, _ = params(w, double)
    J = kernel_reference(("pg", N), model(w))[4]
    check_matrix(s, prm, J, graph_pattern(N, w["i"], w["j"]), double)        # (LM's diagonal is not part of H)


# ------------------------------------------------------------------ 2. the apply against the block variant
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("N", [21, 22, 40, 200])
def test_apply_matches_the_block_variant(block_energy, N, double):
    w = arrays(N)
    p = np.random.default_rng(N).normal(size=3 * N).astype(np.float64 if double else np.float32)
    out = {}
    for name, energy in (("explicit", EXPLICIT), ("block", block_energy)):
        s = solver(w, double=double, energy=energy)
        prm, _ = params(w, double)
        Ap = zeros(3 * N, double)
        pAp = s.apply_jtj(prm, cuda(p), Ap)
        out[name] = (Ap.cpu().numpy(), pAp)
    print("H p against the gather", rel_err(out["explicit"][0], out["block"][0]), "bar", tols(double)[0])
    assert rel_err(out["explicit"][0], out["block"][0]) < tols(double)[0]
    assert out["explicit"][1] == pytest.approx(out["block"][1], rel=10 * tols(double)[1])


# ------------------------------------------------------------------ 3. other block sizes
FIVE = """
local N, E = Dim("N", 0), Dim("E", 1)
local A = Unknown("A", opt_float2, {N}, 0)
local B = Unknown("B", opt_float3, {N}, 1)
local A0 = Array("A0", opt_float2, {N}, 2)
local B0 = Array("B0", opt_float3, {N}, 3)
local Wt = Array("Wt", opt_float2, {E}, 4)
local G = Graph("G", {E}, "i", {N}, 5, "j", {N}, 6, "e", {E}, 7)
NormalMatrix("explicit")
Energy(0.5 * (A(0) - A0(0)))
Energy(0.7 * (B(0) - B0(0)))
local ai, aj, bi, bj, wt = A(G.i), A(G.j), B(G.i), B(G.j), Wt(G.e)
Energy(wt(0) * (ai(0) * bj(1) - aj(1) + sin(bi(2))))
Energy(wt(1) * (bi(0) - bj(0) * ai(1)))
"""


@pytest.mark.parametrize("double", [False, True])
def test_blocks_of_five_over_two_images(tmp_path, double):
    """opt_float2 + opt_float3 over one space (C = 5: 12 rows per wave), a two-slot graph with a
    duplicated edge, data over the edge space; 31 elements: three waves, the last one part full."""
    import torch
    N, E = 31, 70
    rng = np.random.default_rng(5)
    i = rng.integers(0, N, E).astype(np.int32)
    j = ((i + rng.integers(1, N, E)) % N).astype(np.int32)
    i[-1], j[-1] = i[0], j[0]
    A, B = f32(rng.normal(size=(N, 2))), f32(rng.normal(size=(N, 3)))
    A0, B0 = f32(A + 0.1 * rng.normal(size=A.shape)), f32(B + 0.1 * rng.normal(size=B.shape))
    Wt = f32(rng.uniform(0.5, 1.5, (E, 2)))
    e = np.arange(E, dtype=np.int32)
    m = ad.Model([("A", A), ("B", B)], {"A0": A0, "B0": B0, "Wt": Wt})
    ids = np.arange(N)
    m.term(lambda a, a0: 0.5 * (a - a0), [("u", "A", ids), ("c", "A0", ids)], 2)
    m.term(lambda b, b0: 0.7 * (b - b0), [("u", "B", ids), ("c", "B0", ids)], 3)
    m.term(lambda ai, aj, bi, bj, wt: torch.stack([wt[0] * (ai[0] * bj[1] - aj[1] + torch.sin(bi[2])),
                                                   wt[1] * (bi[0] - bj[0] * ai[1])]),
           [("u", "A", i), ("u", "A", j), ("u", "B", i), ("u", "B", j), ("c", "Wt", e)], 2)
    J = m.jacobian()
    path = tmp_path / "five.t"
    path.write_text(FIVE)
    T = np.float64 if double else np.float32
    s = OptSolver([N, E], str(path), "gaussNewtonGPU", double_precision=double)
    assert s.family() == "generic" and s.preconditioner_blocks() == ([0, 0], [0, 2], 1)
    prm = [cuda(A.astype(T)), cuda(B.astype(T)), cuda(A0), cuda(B0), cuda(Wt), cuda(i), cuda(j), cuda(e)]
    index = np.concatenate([np.arange(2 * N).reshape(N, 2), 2 * N + np.arange(3 * N).reshape(N, 3)], 1)
    check_matrix(s, prm, J, graph_pattern(N, i, j), double, index=index)
    assert s.normal_matrix_shape()[1] == 5
    check_apply(s, prm, J, double, seed=3)


@pytest.mark.parametrize("double", [False, True])
def test_a_mesh_energy_with_four_slots(tmp_path, double):
    """cotangent_mesh_smoothing.t with the statement: one index space, every edge couples four
    vertices (12 ordered pairs), the weights nonlinear in all of them."""
    from tests.test_generic_examples_gpu import cot_edges, mesh
    P, F = mesh()
    N = len(P)
    v = cot_edges(F)
    X = f32(P + 0.05 * np.random.default_rng(9).normal(size=P.shape))
    w = {"N": N, "X": X.astype(np.float64), "A": f32(P).astype(np.float64), "w_fitSqrt": 1.0, "w_regSqrt": 0.5,
         "v0": v[0], "v1": v[1], "v2": v[2], "v3": v[3]}
    J = ad.cotangent_mesh_smoothing(w).jacobian()
    text = open(os.path.join(ROOT, "energies", "cotangent_mesh_smoothing.t")).read()
    assert text.count("UsePreconditioner(true)") == 1
    path = tmp_path / "cot_explicit.t"
    path.write_text(text.replace("UsePreconditioner(true)", "UsePreconditioner(true)\n" + STATEMENT))
    s = OptSolver([N, len(v[0])], str(path), "gaussNewtonGPU", double_precision=double)
    assert s.family() == "generic"
    prm = [1.0, 0.5, cuda(X.astype(np.float64 if double else np.float32)), cuda(f32(P)), None] + [cuda(a) for a in v]
    check_matrix(s, prm, J, graph_pattern(N, *v), double)
    check_apply(s, prm, J, double, seed=4)


# ------------------------------------------------------------------ 4. a long row, parallel edges
def star_and_parallel():
    """The 200-pose fixture plus a star (pose 0 joined to 80 others: its row has more blocks than
    the SpMV's long-row threshold) and 140 parallel constraints between poses 5 and 6 (block
    (5, 6) sums more pairs than the assembly's one-wave form takes)."""
    w = dict(arrays(200))
    rng = np.random.default_rng(12)
    far = rng.choice(np.arange(10, 200), 80, replace=False)
    i = np.concatenate([np.zeros(80, np.int64), np.full(140, 5)]).astype(np.int32)
    j = np.concatenate([far, np.full(140, 6)]).astype(np.int32)
    V = w["P"].astype(np.float64)
    c, s = np.cos(V[i, 2]), np.sin(V[i, 2])
    dt = V[j, :2] - V[i, :2]
    d = V[j, 2] - V[i, 2]
    z = np.stack([c * dt[:, 0] + s * dt[:, 1], -s * dt[:, 0] + c * dt[:, 1], np.arctan2(np.sin(d), np.cos(d))], 1)
    z += rng.normal(0, 1, z.shape) * [0.02, 0.02, 0.01]
    U = np.triu(rng.normal(0, 0.3, (len(i), 3, 3))) + 1.5 * np.eye(3)
    w["i"], w["j"] = np.concatenate([w["i"], i]), np.concatenate([w["j"], j])
    w["Z"] = f32(np.concatenate([w["Z"], z]))
    w["U0"] = f32(np.concatenate([w["U0"], U[:, 0, :]]))
    w["U1"] = f32(np.concatenate([w["U1"], np.stack([U[:, 1, 1], U[:, 1, 2], U[:, 2, 2]], 1)]))
    w["E"] = len(w["i"])
    w["e"] = np.arange(w["E"], dtype=np.int32)
    return w


@pytest.mark.parametrize("double", [False, True])
def test_a_long_row_and_parallel_edges(double):
    w = star_and_parallel()
    counts, row_ptr, col_ind, pair_ptr, _ = api.normal_pattern(200, [w["i"], w["j"]])
    assert row_ptr[1] - row_ptr[0] > LONG_ROW and (np.diff(row_ptr)[1:] <= LONG_ROW).all()
    b56 = row_ptr[5] + list(col_ind[row_ptr[5]:row_ptr[6]]).index(6)
    assert pair_ptr[b56 + 1] - pair_ptr[b56] > LONG_PAIRS
    assert (np.diff(pair_ptr) > LONG_PAIRS).sum() == 2 and (np.diff(pair_ptr) <= LONG_PAIRS).sum() > 500
    J = model(w).jacobian()
    s = solver(w, double=double, energy=EXPLICIT)
    prm, _ = params(w, double)
    check_matrix(s, prm, J, graph_pattern(200, w["i"], w["j"]), double)
    assert s.normal_matrix_shape()[2] == counts["blocks"]
    check_apply(s, prm, J, double, seed=8)


# ------------------------------------------------------------------ 5. whole solves
def three_steps(w, kind, double, energy, extra=()):
    s = solver(w, kind, double, energy=energy)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = params(w, double)
    costs = s.profiled_solve(prm + list(extra))
    return np.array(costs), unk.cpu().numpy()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [40, 200])
def test_solves_match_the_block_variant(block_energy, N, kind, double):
    w = arrays(N)
    ce, xe = three_steps(w, kind, double, EXPLICIT)
    cb, xb = three_steps(w, kind, double, block_energy)
    ref = oracle_costs(N, kind)
    print("costs explicit", ce, "block", cb, "oracle", list(ref), "unknowns", rel_err(xe, xb))
    assert len(ce) == len(cb) == len(ref)                          # the same steps accepted
    np.testing.assert_allclose(ce, cb, rtol=tols(double)[2])
    assert ce[-1] < 0.2 * ce[0]
    if double:
        assert rel_err(xe, xb) < 1e-8


# ------------------------------------------------------------------ 6. excluded elements
def excluded_variant(tmp_path, path, name):
    text = open(path).read()
    assert text.count("UsePreconditioner(") == 1
    text = text.replace("UsePreconditioner(", 'local Mk = Array("Mk", opt_float, {N}, 10)\nExclude(eq(Mk(0), 1))\nUsePreconditioner(')
    out = tmp_path / name
    out.write_text(text)
    return str(out)


@pytest.mark.parametrize("double", [False, True])
def test_an_excluded_pose(tmp_path, block_energy, double):
    """Pose 7 is excluded: its rows of H p are 0 (its columns are not masked: the gather's
    contract), it does not move, and the solve is the block variant's with the same exclusion."""
    N = 40
    w = arrays(N)
    mk = np.zeros(N, np.float32)
    mk[7] = 1
    ex = excluded_variant(tmp_path, EXPLICIT, "explicit_excluded.t")
    bl = excluded_variant(tmp_path, block_energy, "block_excluded.t")
    J = kernel_reference(("pg", N), model(w))[4]
    act = np.ones(3 * N)
    act[21:24] = 0
    s = solver(w, double=double, energy=ex)
    prm, _ = params(w, double)
    Ap = check_apply(s, prm + [cuda(mk)], J, double, seed=2, active=act)
    assert not Ap[21:24].any() and Ap[:21].all() and Ap[24:].all()
    ce, xe = three_steps(w, "gaussNewtonGPU", double, ex, extra=[cuda(mk)])
    cb, xb = three_steps(w, "gaussNewtonGPU", double, bl, extra=[cuda(mk)])
    print("costs explicit", ce, "block", cb)
    np.testing.assert_allclose(ce, cb, rtol=tols(double)[2])
    T = np.float64 if double else np.float32
    assert xe[7].tobytes() == w["P"][7].astype(T).tobytes()
    assert not np.array_equal(xe[6], w["P"][6].astype(T))


# ------------------------------------------------------------------ 7. determinism
def test_explicit_solves_are_bitwise_reproducible():
    w = star_and_parallel()                                        # both assembly forms, both SpMV forms
    out = [three_steps(w, "LMGPU", False, EXPLICIT) for _ in range(2)]
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][0][-1] < out[0][0][0] and not np.array_equal(out[0][1], w["P"])


# ------------------------------------------------------------------ 8. re-wiring between Steps
def rewired(w):
    """Another wiring: the constraints in another order, five of them moved to other poses."""
    order = np.random.default_rng(3).permutation(w["E"])
    i, j = w["i"][order].copy(), w["j"][order].copy()
    j[:5] = (i[:5] + 7) % w["N"]
    return dict(w, i=i, j=j, Z=w["Z"][order], U0=w["U0"][order], U1=w["U1"][order])


@pytest.mark.parametrize("in_place", [False, True])
def test_rewiring_between_steps_matches_a_fresh_plan(in_place):
    N = 40
    w = arrays(N)
    w2 = rewired(w)
    assert not np.array_equal(graph_pattern(N, w["i"], w["j"]), graph_pattern(N, w2["i"], w2["j"]))
    sa = solver(w, energy=EXPLICIT)
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = params(w, False)
    sa.init(prm)
    assert sa.step()
    assert np.array_equal(dense_of(*sa.normal_matrix(prm))[1], graph_pattern(N, w["i"], w["j"]))
    state = unk.cpu().numpy().copy()
    if in_place:                                                   # the same device arrays, rewritten
        prm_a, unk_a = prm, unk
        for k, name in zip((4, 5, 6, 7, 8), ("Z", "U0", "U1", "i", "j")):
            prm_a[k].copy_(cuda(w2[name]))
    else:                                                          # other arrays bound
        prm_a, unk_a = params(dict(w2, P=state), False)
        prm_a[2] = cuda(w["P0"])                                   # the prior stays where it was
    assert sa.step(prm_a)
    sb = solver(w, energy=EXPLICIT)
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm_b, unk_b = params(dict(w2, P=state), False)
    prm_b[2] = cuda(w["P0"])
    sb.init(prm_b)
    assert sb.step()
    assert unk_a.cpu().numpy().tobytes() == unk_b.cpu().numpy().tobytes()
    assert not np.array_equal(unk_a.cpu().numpy(), state)
    assert sa.cost() == sb.cost()
    Ha, pat_a = dense_of(*sa.normal_matrix(prm_a))
    Hb, pat_b = dense_of(*sb.normal_matrix(prm_b))
    assert np.array_equal(pat_a, graph_pattern(N, w2["i"], w2["j"])) and np.array_equal(pat_b, pat_a)
    assert Ha.tobytes() == Hb.tobytes()


# ------------------------------------------------------------------ 9. the Step boundary
def test_unknowns_rewritten_between_steps_are_seen():
    """The caller overwrites P between two Steps: the second Step assembles H at the new poses,
    as a fresh plan started there does."""
    N = 40
    w = arrays(N)
    sa = solver(w, energy=EXPLICIT)
    sa.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm, unk = params(w, False)
    sa.init(prm)
    assert sa.step()
    moved = f32(w["P"] + 0.05 * np.random.default_rng(1).normal(size=w["P"].shape))
    unk.copy_(cuda(moved))
    assert sa.step()
    sb = solver(w, energy=EXPLICIT)
    sb.set_solver_params({"nIterations": 4, "lIterations": 10})
    prm_b, unk_b = params(dict(w, P=moved), False)
    prm_b[2] = cuda(w["P0"])
    sb.init(prm_b)
    assert sb.step()
    assert unk.cpu().numpy().tobytes() == unk_b.cpu().numpy().tobytes()
    assert sa.cost() == sb.cost()
    Ha, _ = dense_of(*sa.normal_matrix(prm))
    Hb, _ = dense_of(*sb.normal_matrix(prm_b))
    assert Ha.tobytes() == Hb.tobytes()


# ------------------------------------------------------------------ 10. the entry points on other plans
def test_entry_points_on_other_plans(block_energy, capfd):
    w = arrays(40)
    for energy in (PG, block_energy):
        s = solver(w, energy=energy)
        prm, _ = params(w, False)
        s.init(prm)
        assert s.normal_matrix_shape() is None
        with pytest.raises(api.OptError, match="OptAMD_NormalMatrix failed"):
            s.normal_matrix(prm)
    assert s.lib.OptAMD_PlanNormalMatrixShape(None, None, None, None) == -1
    # plan-level refusals of every block file stay, by name
    for kw in ({"materialized": True}, {"materialized": True, "fused_jtj": True}):
        capfd.readouterr()
        with pytest.raises(api.OptError, match="Opt_ProblemPlan failed"):
            solver(w, energy=EXPLICIT, **kw)
        assert 'useMaterializedJTJ / useFusedJTJ) with NormalMatrix("explicit")' in capfd.readouterr().err
    s = solver(w, energy=EXPLICIT)
    group = s.lib.OptAMD_LocalGroupCreate(2)
    with pytest.raises(api.OptError, match="OptAMD_PlanSetDecomposition failed"):
        s.set_decomposition(s.lib.OptAMD_LocalGroupRank(group, 0), 0, 1)
    s.lib.OptAMD_LocalGroupDestroy(group)
    assert "no row-slab decomposition with the block preconditioner" in capfd.readouterr().err
