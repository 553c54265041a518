"""CPU: the NormalMatrix("explicit") statement in the front end (both parsers, the signature
token, the generated source and its compile, the refusals by name) and the symbolic phase of
the explicitly formed J^T J, on the host from index arrays alone. No device:
Opt_ProblemDefine, the OptAMD_Generic* calls, hiprtc and OptAMD_NormalPattern.

Opt_ProblemPlan asks for a HIP device before it looks at the energy, so the plan's shape
checks are reached here through OptAMD_GenericPlanCheck, the function the plan calls."""
import os

import numpy as np
import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = os.path.join(ROOT, "energies", "pose_graph_2d.t")
EXPLICIT = os.path.join(ROOT, "energies", "normal_matrix", "pose_graph_2d_explicit.t")
COT = os.path.join(ROOT, "energies", "cotangent_mesh_smoothing.t")
STATEMENT = 'NormalMatrix("explicit")'
KERNELS = ("gen_normal_eblk", "gen_normal_assemble", "gen_normal_assemble_long", "gen_normal_spmv")


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in list(os.environ):
        if k.startswith("OPT_AMD_GEN_"):
            monkeypatch.delenv(k)


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def code_lines(text):
    return [ln for ln in text.splitlines() if ln.strip() and not ln.startswith("--")]


# ------------------------------------------------------------------ the statement
def test_statement_and_signature_token(tmp_path):
    pg, explicit = open(PG).read(), open(EXPLICIT).read()
    assert [ln for ln in code_lines(explicit) if ln != STATEMENT] == code_lines(pg)
    assert code_lines(explicit).count(STATEMENT) == 1
    sig = api.generic_signature(PG)
    assert not sig.endswith("B;")
    # the statement turns the block preconditioner on: B; then NX;
    assert api.generic_signature(EXPLICIT) == sig + "B;NX;"
    block = write(tmp_path, "block.t", pg.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    assert api.generic_signature(block) == sig + "B;"
    assert api.generic_describe(EXPLICIT) == api.generic_describe(PG)
    assert api.problem_family(EXPLICIT) == "generic" and api.problem_family(EXPLICIT, "LMGPU") == "generic"
    assert api.generic_plan_check(EXPLICIT) == "" and api.generic_plan_check(PG) == ""
    # the statement before UsePreconditioner(true): still the block form
    swapped = write(tmp_path, "swapped.t", explicit.replace("UsePreconditioner(true)\n" + STATEMENT,
                                                            STATEMENT + "\nUsePreconditioner(true)"))
    assert open(swapped).read() != explicit
    assert api.generic_signature(swapped) == sig + "B;NX;"
    assert api.generic_source(swapped) == api.generic_source(EXPLICIT)
    # "matrix_free" is today's behaviour: signature, routing and source of the file without it
    free = write(tmp_path, "free.t", explicit.replace(STATEMENT, 'NormalMatrix("matrix_free")'))
    assert api.generic_signature(free) == sig
    assert api.problem_family(free) == "generic"
    for double in (False, True):
        for off32 in (False, True):
            assert api.generic_source(free, double, off32) == api.generic_source(PG, double, off32)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("off32", [False, True])
def test_source_has_the_normal_kernels_only_with_the_statement(tmp_path, double, off32):
    pg = open(PG).read()
    block = write(tmp_path, "block.t", pg.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    src, base = api.generic_source(EXPLICIT, double, off32), api.generic_source(block, double, off32)
    for k in KERNELS:
        assert src.count('extern "C" __global__ __launch_bounds__(256) void %s(' % k) == 1
        assert k not in base and k not in api.generic_source(PG, double, off32)
    # the statement only adds kernels to the block variant's: the matrix-free ones stay
    assert src.startswith(base[:base.rindex("}") + 1])
    assert "constexpr int CR = 3, CE = 3" in src and "constexpr int C = 3, CC = C * C, RW = 64 / C" in src
    assert "qb.b[1]" in src and "qb.b[2]" not in src          # two instance lists: slots i and j
    assert "void gen_schur" not in src


@pytest.mark.parametrize("double", [False, True])
def test_explicit_source_compiles_for_gfx950(double):
    api.generic_compile_check(EXPLICIT, double)     # both gather forms (a.gnb[...] present)
    assert "a.gnb[" in api.generic_source(EXPLICIT, double)


def test_a_mesh_energy_with_four_slots(tmp_path):
    """cotangent_mesh_smoothing.t with the statement: one index space, four slots over it, a
    centred term at offset 0. Accepted, four lists, compiles in both precisions and gather forms;
    the file as shipped keeps its hand-free source."""
    text = open(COT).read()
    assert text.count("UsePreconditioner(true)") == 1
    path = write(tmp_path, "cot_explicit.t", text.replace("UsePreconditioner(true)", "UsePreconditioner(true)\n" + STATEMENT))
    assert api.problem_family(path) == "generic"
    assert api.generic_plan_check(path) == ""
    assert api.generic_signature(path) == api.generic_signature(COT) + "B;NX;"
    src = api.generic_source(path)
    assert "qb.b[3]" in src and "qb.b[4]" not in src
    assert "constexpr int CR = 3, CE = 3" in src
    for k in KERNELS:
        assert k not in api.generic_source(COT)
    for double in (False, True):
        api.generic_compile_check(path, double)


# ------------------------------------------------------------------ refusals of the statement
PGT = open(PG).read()
BA_SCHUR = open(os.path.join(ROOT, "energies", "bundle_adjustment_schur.t")).read()
DEFINE_REFUSALS = [
    ("other_form", PGT + 'NormalMatrix("dense")\n', 'form is "explicit" or "matrix_free"'),
    ("number", PGT + "NormalMatrix(1)\n", 'form is "explicit" or "matrix_free"'),
    ("no_argument", PGT + "NormalMatrix()\n", 'form is "explicit" or "matrix_free"'),
    ("second_statement", PGT + STATEMENT + "\n" + 'NormalMatrix("matrix_free")\n', "a second NormalMatrix"),
    ("with_eliminate", BA_SCHUR + STATEMENT + "\n", 'ReducedSystem("explicit")'),
    ("matrix_free_with_eliminate", BA_SCHUR + 'NormalMatrix("matrix_free")\n', "NormalMatrix: the energy has an Eliminate statement"),
]


@pytest.mark.parametrize("name,text,cause", DEFINE_REFUSALS, ids=[r[0] for r in DEFINE_REFUSALS])
def test_front_end_refusals_name_their_cause(tmp_path, capfd, name, text, cause):
    path = write(tmp_path, name + ".t", text)
    capfd.readouterr()
    with pytest.raises(api.OptError, match="Opt_ProblemDefine refused"):
        api.problem_family(path)
    err = capfd.readouterr().err
    print(err)
    assert cause in err


# ------------------------------------------------------------------ shapes the plan refuses
HEAD = """
local N, M, E = Dim("N", 0), Dim("M", 1), Dim("E", 2)
local X = Unknown("X", opt_float3, {N}, 0)
local A = Array("A", opt_float3, {N}, 1)
local D = Array("D", opt_float, {E}, 2)
local G = Graph("G", {E}, "i", {N}, 3, "j", {N}, 4, "k", {N}, 5, "l", {N}, 6, "e", {E}, 7)
NormalMatrix("explicit")
Energy(X(0) - A(0))
"""
EDGE = "Energy(D(G.e) * (X(G.i)(0) - X(G.j)(1)))\n"
PLAN_REFUSALS = [
    ("two_unknown_spaces", HEAD.replace("local A =", 'local Y = Unknown("Y", opt_float2, {M}, 8)\nlocal A =') + EDGE
     + "Energy(Y(0))\n",
     "the unknowns lie over 2 index spaces ({N}, {M}); the block-sparse J^T J has one block group"),
    ("centred_offset", HEAD + EDGE + "Energy(X(1) - X(0))\n",
     "a centred residual over {N} reads X at a non-zero offset"),
    ("computed_array_offset", HEAD.replace("NormalMatrix", 'local Cx = ComputedArray("Cx", {N}, X(1)(0) - X(0)(0))\nNormalMatrix')
     + EDGE + "Energy(Cx(0))\n",
     "ComputedArray 'Cx' depends on X at a non-zero offset"),
]


@pytest.mark.parametrize("name,text,cause", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_plan_refusals_name_their_cause(tmp_path, name, text, cause):
    path = write(tmp_path, name + ".t", text)
    assert api.problem_family(path) == "generic"          # the front end takes the energy
    why = api.generic_plan_check(path)
    print(why)
    assert why.startswith('generic: NormalMatrix("explicit"): ') and cause in why
    # the same energy with the matrix-free form is planned, and emits no explicit kernel either way
    assert api.generic_plan_check(write(tmp_path, name + "_free.t", text.replace(STATEMENT, ""))) == ""
    assert "gen_normal_spmv" not in api.generic_source(path)


def test_accepted_neighbours_of_the_plan_refusals(tmp_path):
    """Four slots over the unknowns' space, centred terms at offset 0 (a ComputedArray of the
    element's own unknowns among them), arrays and a slot over a second space."""
    ok = (HEAD.replace("NormalMatrix", 'local Cx = ComputedArray("Cx", {N}, X(0)(0) * X(0)(1))\nNormalMatrix') + EDGE
          + "Energy(X(G.i)(2) + X(G.j)(0) - 2 * X(G.k)(1) + D(G.e) * X(G.l)(2))\nEnergy(Cx(0))\n")
    path = write(tmp_path, "ok.t", ok)
    assert api.generic_plan_check(path) == ""
    assert api.generic_signature(path).endswith("B;NX;")
    src = api.generic_source(path)
    assert "qb.b[3]" in src and "qb.b[4]" not in src      # four instance lists: i, j, k, l (not e)
    assert "constexpr int CR = 3, CE = 2" in src           # two residuals per edge
    for double in (False, True):
        api.generic_compile_check(path, double)


# ------------------------------------------------------------------ the symbolic phase
def numpy_pattern(n, lists, graph_edges):
    """Positions, pairs per block in enumeration order, restated with dictionaries: per graph,
    per edge, the instances in [list, edge] order; every ordered pair of two different ones."""
    base, at = [], 0
    for g, v in lists:
        base.append(at)
        at += len(v)
    blocks = {(r, r): [] for r in range(n)}
    for g, ne in enumerate(graph_edges):
        for e in range(ne):
            inst = [(base[l] + e, int(v[e])) for l, (gl, v) in enumerate(lists) if gl == g]
            for a, (q1, r1) in enumerate(inst):
                for b, (q2, r2) in enumerate(inst):
                    if a != b:
                        blocks.setdefault((r1, r2), []).append((q1, q2))
    return blocks


def check_pattern(n, lists, graph_edges):
    counts, row_ptr, col_ind, pair_ptr, pairs = api.normal_pattern(n, lists, graph_edges)
    want = numpy_pattern(n, lists, graph_edges)
    keys = sorted(want)
    assert counts == {"instances": sum(len(v) for _, v in lists), "pairs": sum(len(v) for v in want.values()),
                      "blocks": len(keys)}
    assert [int(c) for c in col_ind] == [c for _, c in keys]
    assert [int(x) for x in row_ptr] == [sum(1 for r, _ in keys if r < row) for row in range(n + 1)]
    assert pair_ptr[0] == 0 and pair_ptr[-1] == counts["pairs"]
    for b, key in enumerate(keys):
        assert [tuple(int(x) for x in pq) for pq in pairs[pair_ptr[b]:pair_ptr[b + 1]]] == want[key], key
    return counts, row_ptr, col_ind, pair_ptr, pairs


def test_pattern_of_a_small_graph_with_every_edge_case():
    # 5 vertices; edges 0-1, 0-1 again (a duplicate), 1-0 (the reverse), 2-2 (a self-loop), 3-1;
    # vertex 4 is isolated: its row holds the diagonal block alone
    i = np.array([0, 0, 1, 2, 3], np.int32)
    j = np.array([1, 1, 0, 2, 1], np.int32)
    counts, row_ptr, col_ind, pair_ptr, pairs = check_pattern(5, [(0, i), (0, j)], [5])
    assert counts == {"instances": 10, "pairs": 10, "blocks": 5 + 2 + 2}
    assert list(row_ptr) == [0, 2, 5, 6, 8, 9] and list(col_ind) == [0, 1, 0, 1, 3, 2, 1, 3, 4]
    # block (0, 1): edges 0 and 1 as (i, j), edge 2 as (j, i); positions: list i at 0..4, list j at 5..9
    assert [tuple(p) for p in pairs[pair_ptr[1]:pair_ptr[2]]] == [(0, 5), (1, 6), (7, 2)]
    # the self-loop: both orders of its two instances land on the diagonal block of vertex 2
    assert [tuple(p) for p in pairs[pair_ptr[5]:pair_ptr[6]]] == [(3, 8), (8, 3)]
    assert pair_ptr[8] == pair_ptr[9] == 10                      # vertex 4: its diagonal block, no pair
    assert pair_ptr[0] == pair_ptr[1] == 0                       # vertex 0's diagonal: no self-loop there


def test_pattern_of_four_slot_edges():
    """A 4-slot edge has 4 * 3 = 12 ordered pairs; two graphs share the vertices."""
    rng = np.random.default_rng(8)
    quad = [(0, rng.integers(0, 7, 9).astype(np.int32)) for _ in range(4)]
    counts, *_ = check_pattern(7, quad, [9])
    assert counts["pairs"] == 12 * 9 and counts["instances"] == 36
    two = quad + [(1, rng.integers(0, 7, 5).astype(np.int32)), (1, rng.integers(0, 7, 5).astype(np.int32))]
    counts, *_ = check_pattern(7, two, [9, 5])
    assert counts["pairs"] == 12 * 9 + 2 * 5 and counts["instances"] == 46


def test_pattern_counts_of_the_pose_graph_fixture():
    from tests.test_pose_graph_gpu import arrays
    for N in (40, 200):
        w = arrays(N)
        counts, row_ptr, col_ind, _, _ = check_pattern(N, [(0, w["i"]), (0, w["j"])], [w["E"]])
        assert counts["pairs"] == 2 * w["E"] and counts["instances"] == 2 * w["E"]
        D = np.eye(N, dtype=bool)
        D[w["i"], w["j"]] = D[w["j"], w["i"]] = True
        assert counts["blocks"] == int(D.sum())


def test_pattern_refuses_bad_input_by_name():
    with pytest.raises(api.OptError, match="vertex index outside its space at edge 1"):
        api.normal_pattern(3, [np.array([0, 3], np.int32), np.array([0, 1], np.int32)])


def test_pattern_refuses_more_pairs_than_an_int_indexes():
    """Counted before anything of that size is allocated: 256 lists of one graph (the host entry
    point has no limit on them) are 65 280 ordered pairs per edge, so 32 897 edges are
    2 147 516 160 > 2^31 - 1 pairs."""
    ne, k = 32897, 256
    v = np.zeros(ne, np.int32)
    assert k * (k - 1) * ne > 2 ** 31 - 1 > k * (k - 1) * (ne - 1)
    with pytest.raises(api.OptError, match=r'NormalMatrix\("explicit"\): %d instance pairs over %d edge instances'
                                           % (k * (k - 1) * ne, k * ne)):
        api.normal_pattern(1, [(0, v)] * k, [ne])
