"""GPU: the solver side of the materialized-Jacobian path (csr.h: sell_widths / sell_fill /
compose / sell_gather / sell_spmv, prod_map, pair_depth / pair_fill / ata_from_pairs and
both J^T J pattern paths) on irregular graphs, every row held to a reference.

The energy (tests/materialized_graph_helpers.py) has per-vertex fit rows and three rows per
edge over three freely chosen vertices, so the edge list decides the sparsity; the fixtures
reach every branch (tests/test_materialized_graph_fixture.py asserts that on the CPU). The
reference is the analytic J in float64 as a dense matrix, written from the energy's
partials; no tolerance below is tuned to the code under test."""
import numpy as np
import pytest

from opt_amd import OptSolver
from oracle import oracle
from tests import materialized_graph_helpers as mg
from tests.test_materialized_graph_fixture import WIRINGS

pytestmark = pytest.mark.gpu


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def params(g, w):
    """Device parameters in declared-index order."""
    mg.check_in_range(g)
    return [w["w_fit"], w["w_reg"], dev(w["X"]), dev(w["T"]), dev(w["Wt"]), dev(w["M"]),
            dev(g["a"]), dev(g["b"]), dev(g["c"])]


def solver(tmp_path, g, double, fused):
    s = OptSolver([g["N"], g["E"]], mg.write_energy(tmp_path), "gaussNewtonGPU", double_precision=double,
                  materialized=True, fused_jtj=fused)
    assert s.family() == "generic"
    assert s.jacobian_shape() == (mg.shape(g)[0], mg.shape(g)[2])
    return s


def dump(s, prm, g, double):
    import torch

    rows, _, nnz = mg.shape(g)
    rp = torch.full((rows + 1,), -1, dtype=torch.int32, device="cuda")
    ci = torch.full((nnz,), -1, dtype=torch.int32, device="cuda")
    v = torch.zeros(nnz, dtype=torch.float64 if double else torch.float32, device="cuda")
    s.eval_jacobian(prm, rp, ci, v)
    return rp.cpu().numpy(), ci.cpu().numpy(), v.cpu().numpy()


def run_apply(s, prm, p):
    import torch

    Ap = torch.full((p.size,), 7.0, dtype=torch.float64 if p.dtype == np.float64 else torch.float32, device="cuda")
    pAp = s.apply_jtj(prm, dev(p), Ap)
    return Ap.cpu().numpy(), pAp


def check_apply(g, w, p, double, Ap, pAp, what=""):
    """(c): componentwise against the dense float64 reference, excluded rows exactly 0."""
    ref, tol, rq, tq = mg.reference_apply(g, w, p, double)
    err = np.abs(Ap.astype(np.float64) - ref)
    worst = int(np.argmax(err - tol))
    print(f"{what} max err/tol {np.max(err[tol > 0] / tol[tol > 0]):.3g}; pAp err {abs(pAp - rq):.3g} tol {tq:.3g}")
    assert np.all(Ap[~mg.active(g, w)] == 0)
    assert np.all(err <= tol), (what, worst, Ap[worst], ref[worst], tol[worst])
    assert abs(pAp - rq) <= tq, (what, pAp, rq, tq)


def check_nonzeros(s, st, fused):
    """(b): exactly the stored nonzeros of J and of the structural J^T J pattern (stored
    zeros counted); an unfused plan forms no J^T J, so only J's count is held there."""
    nz = s.materialized_nonzeros()
    if fused:
        assert nz == (st["nnzJ"], st["nnzJTJ"]), (nz, st["nnzJ"], st["nnzJTJ"])
    else:
        assert nz[0] == st["nnzJ"], (nz, st["nnzJ"])


# ------------------------------------------------------------------------- a. assembly
@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", mg.VARIANTS)
def test_assembled_jacobian_matches_the_analytic_one(tmp_path, name, double):
    """rowPtr exact; columns non-decreasing inside a row, strictly increasing unless the
    variant repeats vertices inside an edge; the dense matrix of the dump (repeated
    columns summed) within 4 ulp of the plan's type per stored part: every entry is at
    most two roundings of exact inputs."""
    g = mg.variant(name)
    w = mg.inputs(g, double)
    rp, ci, v = dump(solver(tmp_path, g, double, True), params(g, w), g, double)
    rows, cols, nnz = mg.shape(g)
    np.testing.assert_array_equal(rp, mg.row_ptr(g))
    assert ci.min() >= 0 and ci.max() < cols
    inside = np.ones(nnz, bool)
    inside[rp[:-1]] = False   # first entry of every row
    step = np.diff(ci, prepend=0)[inside]
    if name == "dups":
        assert np.all(step >= 0) and np.any(step == 0)
    else:
        assert np.all(step > 0)
    D = np.zeros((rows, cols))
    np.add.at(D, (np.repeat(np.arange(rows), np.diff(rp)), ci), v.astype(np.float64))
    J, _, ulp = mg.analytic(g, w, double)
    if name != "dups":
        np.testing.assert_array_equal(D != 0, J != 0)
    assert np.all(np.abs(D - J) <= 4 * ulp), float(np.max(np.abs(D - J) / np.maximum(ulp, 1e-300)))


# -------------------------------------------------------------------- b + c. the apply
@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", mg.VARIANTS)
def test_apply_matches_dense_fp64_reference(tmp_path, name, fused, double):
    g = mg.variant(name)
    w = mg.inputs(g, double)
    p = mg.direction(g, w, double)
    s = solver(tmp_path, g, double, fused)
    Ap, pAp = run_apply(s, params(g, w), p)
    st = mg.pattern_stats(g)
    check_nonzeros(s, st, fused)
    check_apply(g, w, p, double, Ap, pAp, f"{name} fused={fused} double={double}:")


# ------------------------------------------------------------- d. the bitwise promise
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", ["moderate", "hub", "tiny"])
def test_apply_is_bitwise_the_cpu_restatement_on_irregular_rows(tmp_path, name, fused):
    """csr.h promises the reference CPU backend's results bit for bit (computeATA's
    summation order, applyAtoVector's): here on rows of every length, not only poisson's
    uniform ones. The dumped J goes through the oracle's restatement; the result is masked
    and compared exactly.

    `dups` is left out on purpose: the reference's getEntry / computeATA take the first of
    several entries with one column, so on rows with repeated columns the restatement is
    not the product J^T J, which the kernels (and test c) compute."""
    g = mg.variant(name)
    w = mg.inputs(g, False)
    p = mg.direction(g, w, False)
    s = solver(tmp_path, g, False, fused)
    prm = params(g, w)
    rp, ci, v = dump(s, prm, g, False)
    rows, cols, _ = mg.shape(g)
    if fused:
        rpA, ciA, vA = oracle.csr_ata(rows, cols, rp, ci, v)
        ref = oracle.csr_spmv(cols, cols, rpA, np.ascontiguousarray(ciA), np.ascontiguousarray(vA), p)
    else:
        Jp = oracle.csr_spmv(rows, cols, rp, ci, v, p)
        rpT, ciT, vT = oracle.csr_transpose(rows, cols, rp, ci, v)
        ref = oracle.csr_spmv(cols, rows, rpT, np.ascontiguousarray(ciT), np.ascontiguousarray(vT), Jp)
    ref = np.where(mg.active(g, w), ref, np.float32(0))
    Ap, _ = run_apply(s, prm, p)
    np.testing.assert_array_equal(Ap, ref)


# ------------------------------------------------------- e. the graph changes on one plan
@pytest.mark.parametrize("how", ["rebind", "in_place"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_patterns_follow_the_graph_bound_at_each_call(tmp_path, fused, how):
    """The Step-boundary contract lets a caller rewrite or rebind a graph's vertex arrays
    between calls, and J's column structure comes from them: one plan, four wirings in a
    row (a second random wiring with another nnz(J^T J); the hub, which moves the pattern
    build from the one-thread-per-row path to the general one and back and changes every
    buffer size; the first again), each call held to (b) and (c) for the graph bound at
    THAT call. tests/test_materialized_graph_fixture.py asserts on the CPU that the
    references of consecutive wirings differ by far more than the bound."""
    gs = [(label, mk()) for label, mk in WIRINGS]
    g0 = gs[0][1]
    w = mg.inputs(g0, False)
    p = mg.direction(g0, w, False)
    s = solver(tmp_path, g0, False, fused)
    prm = params(g0, w)
    ptrs = [t.data_ptr() for t in prm[2:]]
    keep = []
    for k, (label, g) in enumerate(gs):
        mg.check_in_range(g)
        if k > 0 and how == "rebind":   # fresh tensors; the old ones stay allocated with their content
            keep.append(prm[6:])
            prm[6:] = [dev(g["a"]), dev(g["b"]), dev(g["c"])]
        elif k > 0:
            for t, key in zip(prm[6:], "abc"):
                t.copy_(dev(g[key]))
        Ap, pAp = run_apply(s, prm, p)
        st = mg.pattern_stats(g)
        check_nonzeros(s, st, fused)
        check_apply(g, w, p, False, Ap, pAp, f"call {k} ({label}) fused={fused} {how}:")
    if how == "in_place":
        assert [t.data_ptr() for t in prm[2:]] == ptrs
