"""GPU: every form of the generated stencil kernels (gather, two-phase LDS tiles, the three
register strips) on the stencil zoo (tests/stencil_zoo.py: wide, one-sided, mixed-channel
and explicitly bounded stencils) against a float64 AD reference of each energy, per kernel
(cost, J^T F with the preconditioner, J^T J p) and in whole GN / LM solves; production-length
row blocks; pair loads at 4-byte-aligned addresses; row slabs exactly one halo tall; the
materialized Jacobian. Every case first asserts from OptSolver.generated_forms() that the
form it forced is the form the plan launches.

Tolerances are the project's bars (tests/test_multispace_gpu.py tols): fp32 per-unknown
outputs within 2e-5 of the largest magnitude, scalars within 1e-5 relative, solves within
1e-4; fp64 1e-9 / 1e-9 / 1e-8.

Whole solves are compared with solve_with_excluded_centres (tests/test_multispace_gpu.py)
rather than examples_ad.solve itself: the same C loop and the same Model, with the Exclude rule
examples_ad.solve lacks (cost over active centres only, masked J^T F and J^T J p)."""
import numpy as np
import pytest

from opt_amd import OptSolver
from tests import stencil_zoo as zoo
from tests.test_multispace_gpu import cuda, kernel_reference, rel_err, solve_with_excluded_centres, tols, zeros

pytestmark = pytest.mark.gpu
KNOBS = ("OPT_AMD_GEN_APPLY", "OPT_AMD_GEN_JTF", "OPT_AMD_GEN_COST")
GATHER = ("gather", "gather", "gather")
TILED = ("tiled", "strip", "strip")      # the tiles, with the strips a second time beside them
STRIP = ("strip", "strip", "strip")
PLANS = (GATHER, TILED, STRIP)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("zoo")
    return {name: zoo.write_energy(d, name) for name in zoo.ZOO}


def expected_forms(name, double, forced):
    """What a plan forced to `forced` launches: a form the generator did not emit falls back
    to the gather. B in fp64 has no apply / J^T F strip: its windows and accumulators (11
    channels' worth) pass the scatter strips' cap of 48 registers per lane in double."""
    sa, sj, sc = zoo.EMITTED[(name, double)][0]
    have = {"strip": (sa, sj, sc)}
    return tuple(f if f != "strip" or have["strip"][k] is not None else "gather" for k, f in enumerate(forced))


def solver(monkeypatch, files, name, W, H, double, forced, kind="gaussNewtonGPU", **kw):
    for knob, f in zip(KNOBS, forced):
        monkeypatch.setenv(knob, f)
    s = OptSolver([W, H], files[name], kind, double_precision=double, **kw)
    assert s.family() == "generic"
    g = s.generated_forms()
    assert (g["apply"], g["jtf"], g["cost"]) == expected_forms(name, double, forced), (g, forced)
    return s


def params(w, double, offset=0):
    """Device arrays in declaration order. offset: the 2-channel arrays (B's U and A) are views
    `offset` elements into larger tensors (1: a 4-byte-aligned, 8-byte-misaligned binding)."""
    import torch
    T = np.float64 if double else np.float32

    def put(a, shift):
        a = np.ascontiguousarray(a).reshape(-1)
        if not shift:
            return cuda(a)
        big = torch.zeros(a.size + shift, dtype=torch.from_numpy(a[:1]).dtype, device="cuda")
        big[shift:] = torch.from_numpy(a).cuda()
        return big[shift:]

    name = w["name"]
    if name == "B":
        return [put(w["V"].astype(T), 0), put(w["U"].astype(T), offset), put(w["A"].astype(np.float32), offset),
                cuda(w["M"]), zoo.PARAM_W]
    prm = [put(w["X"].astype(T), 0), put(w["A"].astype(np.float32), 0)]
    return prm + ([cuda(w["M"])] if "M" in w else [])


_REFS = {}


def reference(name, W, H):
    """The problem and kernel_reference's (cost, r, pre, r.pre.r, J, active) of its float64
    model, computed once per energy and size."""
    w = zoo.problem(name, W, H)
    key = ("zoo", name, W, H)
    if key not in _REFS:
        m, act, cost_rows = zoo.model(w)
        _REFS[key] = kernel_reference(key, m, active=act, use_pre=zoo.ZOO[name]["use_pre"], cost_rows=cost_rows)
    return w, _REFS[key]


def check_kernels(s, prm, ref, double, seed):
    """check_kernels of tests/test_multispace_gpu.py (the same six comparisons against the
    float64 J, the same bars) with p = 0 on excluded unknowns, Ap pre-filled with 7.0 and the
    excluded rows of r, pre and Ap exactly 0. Returns what the kernels wrote."""
    cost, r_ref, pre_ref, rz_ref, J, act = ref
    vec, sca, _ = tols(double)
    n = s.unknown_count()
    assert n == len(r_ref)
    c = s.eval_cost(prm)
    r, pre = zeros(n, double), zeros(n, double)
    r += 7.0
    pre += 7.0
    rz = s.eval_jtf(prm, r, pre)
    r, pre = r.cpu().numpy(), pre.cpu().numpy()
    p = (np.random.default_rng(seed).normal(size=n) * act).astype(np.float64 if double else np.float32)
    Ap = zeros(n, double)
    Ap += 7.0
    pAp = s.apply_jtj(prm, cuda(p), Ap)
    Ap = Ap.cpu().numpy()
    Ap_ref = (J.T @ (J @ p.astype(np.float64))) * act
    pAp_ref = float(p.astype(np.float64) @ Ap_ref)
    print("cost", abs(c - cost) / max(abs(cost), 1e-30), "r", rel_err(r, r_ref), "pre", rel_err(pre, pre_ref),
          "rz", abs(rz - rz_ref) / max(abs(rz_ref), 1e-30), "Ap", rel_err(Ap, Ap_ref),
          "pAp", abs(pAp - pAp_ref) / max(abs(pAp_ref), 1e-30))
    assert c == pytest.approx(cost, rel=sca)
    assert rel_err(r, r_ref) < vec and rel_err(pre, pre_ref) < vec
    assert rz == pytest.approx(rz_ref, rel=sca)
    assert rel_err(Ap, Ap_ref) < vec
    assert pAp == pytest.approx(pAp_ref, rel=sca)
    off = act == 0
    assert not r[off].any() and not pre[off].any() and not Ap[off].any()
    return c, r, pre, rz, Ap, pAp


# ------------------------------------------------------------ a. each form against the reference
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("size", range(7))
@pytest.mark.parametrize("name", sorted(zoo.ZOO))
def test_each_form_matches_the_reference(monkeypatch, files, name, size, double):
    from opt_amd import api
    f = api.generic_forms(files[name], False)
    S, (TX, TY) = f["strip_cols"], (f["tiles_x"], f["tiles_y"])
    assert f["has_strip"] == 1 and (S, (TX, TY)) == (zoo.EMITTED[(name, False)][0][0], zoo.EMITTED[(name, False)][1])
    W, H = zoo.sizes(name)[size]
    assert (W, H) == [(1, 1), (3, 2), (S - 1, 7), (S, 8), (S + 1, 9), (2 * S + 1, 17), (TX + 1, 2 * TY + 1)][size]
    assert W * H < 8000
    w, ref = reference(name, W, H)
    for forced in PLANS:
        s = solver(monkeypatch, files, name, W, H, double, forced)
        print(name, (W, H), "double" if double else "float", forced, end=" ")
        check_kernels(s, params(w, double), ref, double, seed=size)
        s.close()


# ------------------------------------------------------------ b. production row blocks
@pytest.mark.parametrize("name", ["A", "B"])
def test_strips_walk_row_blocks_longer_than_eight_rows(monkeypatch, files, name):
    """A grid of 8 workgroups (32 waves) over three column strips of 103 rows: the apply and
    J^T F strips walk blocks of ceil(3 * 103 / 32) = 10 rows, the last block 3 rows (production:
    about 46 rows at 4096^2); every small test above walks the minimum of 8."""
    S = zoo.EMITTED[(name, False)][0][0]
    W, H = 2 * S + 1, 103
    monkeypatch.setenv("OPT_AMD_GEN_BLOCKS", "8")
    w, ref = reference(name, W, H)
    s = solver(monkeypatch, files, name, W, H, False, STRIP)
    g = s.generated_forms()
    assert g["grid"] == 8 and g["rows"] == H
    for k in ("apply_row_block", "jtf_row_block"):
        assert g[k] == 10 and H % g[k] == 3, g
    assert g["cost_row_block"] >= 8
    check_kernels(s, params(w, False), ref, False, seed=11)


# ------------------------------------------------------------ c. unaligned pairs
def test_pair_windows_at_an_odd_offset_of_the_solver_vector(monkeypatch, files):
    """B at odd W H: V's 3 W H elements come first, so U's windows of p start at an odd element
    (4-byte aligned) and the pair loads take their unaligned branch."""
    W, H = zoo.sizes("B")[5]
    w, ref = reference("B", W, H)
    s = solver(monkeypatch, files, "B", W, H, False, STRIP)
    off, n, ch = s.unknown_layout()
    assert (off, n, ch) == ([0, 3 * W * H], [W * H, W * H], [3, 2]) and off[1] % 2 == 1
    check_kernels(s, params(w, False), ref, False, seed=12)


def test_pair_windows_of_misaligned_user_arrays(monkeypatch, files):
    """B with U and A bound one element into larger tensors (4-byte aligned): the strips against
    the reference, and bitwise the aligned binding of the same data (the same loads, the same
    arithmetic)."""
    W, H = zoo.sizes("B")[4]
    w, ref = reference("B", W, H)
    out = []
    for offset in (0, 1):
        s = solver(monkeypatch, files, "B", W, H, False, STRIP)
        prm = params(w, False, offset)
        assert prm[1].data_ptr() % 8 == 4 * offset and prm[2].data_ptr() % 8 == 4 * offset
        out.append(check_kernels(s, prm, ref, False, seed=13))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ------------------------------------------------------------ d. whole solves
_SOLVES = {}


def oracle_costs(name, W, H, lm):
    key = (name, W, H, lm)
    if key not in _SOLVES:
        m, act, cost_rows = zoo.model(zoo.problem(name, W, H))
        _SOLVES[key] = solve_with_excluded_centres(m, cost_rows, act, 3, 10, lm, use_pre=zoo.ZOO[name]["use_pre"])
    return _SOLVES[key]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("name", ["A", "D"])
def test_solves_match_the_oracle(monkeypatch, files, name, kind, double):
    S = zoo.EMITTED[(name, False)][0][0]
    W, H = S + 1, 17
    w = zoo.problem(name, W, H)
    ref = oracle_costs(name, W, H, kind == "LMGPU")
    out = {}
    for tag, forced in (("gather", GATHER), ("strip", STRIP), ("strip2", STRIP)):
        s = solver(monkeypatch, files, name, W, H, double, forced, kind)
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm = params(w, double)
        costs = s.profiled_solve(prm)
        out[tag] = (np.array(costs), prm[0].cpu().numpy())
        s.close()
    for tag in ("gather", "strip"):
        costs, X = out[tag]
        print(name, kind, tag, "costs", list(costs), "oracle", list(ref))
        assert len(costs) == len(ref)                                   # the same steps accepted
        np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])
        start = w["X"].reshape(-1).astype(X.dtype)
        assert np.array_equal(X[~w["active"]], start[~w["active"]])     # excluded pixels unmoved
        assert not np.array_equal(X[w["active"]], start[w["active"]])
    assert out["strip"][0].tobytes() == out["strip2"][0].tobytes()
    assert out["strip"][1].tobytes() == out["strip2"][1].tobytes()


# ------------------------------------------------------------ e. slabs
class ZooFamily:
    """What run() of tests/test_decomposition_generic_gpu.py needs of an energy."""

    def __init__(self, name, energy):
        from opt_amd import distributed as dd
        self.dd, self.name, self.energy, self.kind = dd, name, energy, "gaussNewtonGPU"
        self.arrays = [(nm, ch) for nm, ch in zoo.ZOO[name]["unknowns"]] + [("A", 2 if name == "B" else 1)]
        if zoo.ZOO[name]["exclude"] is not None:
            self.arrays.append(("M", 1))

    def params(self, w, s=None):
        out = []
        for nm, ch in self.arrays:
            a = np.ascontiguousarray(w[nm]).reshape(-1)
            a = a if nm == "M" else a.astype(np.float32)
            out.append(cuda((a if s is None else self.dd.slice_rows(a, w["W"], ch, s)).copy()))
        return out + ([zoo.PARAM_W] if self.name == "B" else [])


@pytest.mark.parametrize("name,world,H", [("A", 2, 7), ("A", 3, 10), ("B", 2, 5), ("B", 3, 7), ("C", 2, 17), ("C", 3, 25)])
def test_slabs_exactly_one_halo_tall(monkeypatch, files, name, world, H):
    """Row slabs of the generated gathers with halo 3 (A), 2 (B) and 8 (C): H // world rows per
    slab, exactly the halo, the last slab one row more (C at H = 17: 8 + 9). The halo is the
    one derived from the energy's offsets; the solve agrees with the single domain (the bar of
    test_generated_kernels_decomposed_match_single_domain) and with the float64 oracle."""
    from opt_amd import distributed as dd
    from tests.test_decomposition_generic_gpu import run
    halo = zoo.halo_from_offsets(name)
    assert H // world == halo and dd.slab(H, 0, world, halo).rows == halo
    W = zoo.EMITTED[(name, False)][0][0] + 1
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    fam = ZooFamily(name, files[name])
    w = zoo.problem(name, W, H)
    s = OptSolver([W, H], fam.energy, fam.kind)
    assert s.family() == "generic" and s.halo() == halo
    prm = fam.params(w)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    ref = s.profiled_solve(prm)
    Xref = prm[0].cpu().numpy()
    costs, X = run(fam, w, world, 3, 10)
    oracle = oracle_costs(name, W, H, False)
    print(name, world, "slabs", costs[0], "single", ref, "oracle", list(oracle))
    for r in range(world):
        assert costs[r] == costs[0]
    assert len(costs[0]) == len(ref) == len(oracle)
    np.testing.assert_allclose(costs[0], ref, rtol=1e-5)
    assert np.abs(X - Xref).max() <= 1e-5 * np.abs(Xref).max()
    np.testing.assert_allclose(costs[0], oracle, rtol=tols(False)[2])


# ------------------------------------------------------------ f. materialized
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["A", "B"])
def test_materialized_apply_matches_the_reference(monkeypatch, files, name, fused):
    """The dumped J (gen_dump_j) and its SpMVs: rows and nonzeros per pixel as counted from the
    energy text (every scalar residual, every unknown access), J^T J p against the float64 J."""
    W, H = zoo.sizes(name)[4]
    w, ref = reference(name, W, H)
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    s = OptSolver([W, H], files[name], "gaussNewtonGPU", materialized=True, fused_jtj=fused)
    assert s.family() == "generic" and s.generated_forms()["materialized"] == 1
    assert s.jacobian_shape() == zoo.jacobian_counts(name, W, H)
    _, _, _, _, J, act = ref
    n = s.unknown_count()
    p = (np.random.default_rng(21).normal(size=n) * act).astype(np.float32)
    Ap = zeros(n, False)
    Ap += 7.0
    pAp = s.apply_jtj(params(w, False), cuda(p), Ap)
    Ap = Ap.cpu().numpy()
    Ap_ref = (J.T @ (J @ p.astype(np.float64))) * act
    print(name, fused, "Ap", rel_err(Ap, Ap_ref), "pAp", pAp, float(p @ Ap_ref))
    assert rel_err(Ap, Ap_ref) < tols(False)[0]
    assert pAp == pytest.approx(float(p.astype(np.float64) @ Ap_ref), rel=tols(False)[1])
    assert not Ap[act == 0].any()
