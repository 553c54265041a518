"""CPU: the ReducedSystem("explicit") statement in the front end (both parsers, the signature
token, the generated source and its compile, the refusals by name) and the symbolic phase of
the explicitly formed Schur complement, on the host from index arrays alone. No device:
Opt_ProblemDefine, the OptAMD_Generic* calls, hiprtc and OptAMD_SchurPattern.

Opt_ProblemPlan asks for a HIP device before it looks at the energy, so the plan's shape
checks are reached here through OptAMD_GenericPlanCheck, the function the plan calls.

tests/golden/generated_source_sha256.json holds the sha256 of OptAMD_GenericSource for every
shipped energy without the statement and its UsePreconditioner("block") variant
(tools/gen_dump_matrix.py's substitution), float / double x off32 off / on, recorded on the
commit before the statement existed: those files keep their source byte for byte."""
import glob
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHUR = os.path.join(ROOT, "energies", "bundle_adjustment_schur.t")
EXPLICIT = os.path.join(ROOT, "energies", "bundle_adjustment_schur_explicit.t")
STATEMENT = 'ReducedSystem("explicit")'


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
    schur, explicit = open(SCHUR).read(), open(EXPLICIT).read()
    assert [ln for ln in code_lines(explicit) if ln != STATEMENT] == code_lines(schur)
    assert code_lines(explicit).count(STATEMENT) == 1
    sig = api.generic_signature(SCHUR)
    assert sig.endswith("S1;")
    assert api.generic_signature(EXPLICIT) == sig + "RX;"
    assert api.generic_describe(EXPLICIT) == api.generic_describe(SCHUR)
    assert api.problem_family(EXPLICIT) == "generic" and api.problem_family(EXPLICIT, "LMGPU") == "generic"
    assert api.generic_plan_check(EXPLICIT) == "" and api.generic_plan_check(SCHUR) == ""
    # either order of the two statements
    swapped = write(tmp_path, "swapped.t", explicit.replace("Eliminate(X)\n" + STATEMENT, STATEMENT + "\nEliminate(X)"))
    assert open(swapped).read() != explicit
    assert api.generic_signature(swapped) == sig + "RX;"
    assert api.generic_source(swapped) == api.generic_source(EXPLICIT)
    # "implicit" is today's behaviour: signature, routing and source of the file without it
    implicit = write(tmp_path, "implicit.t", explicit.replace(STATEMENT, 'ReducedSystem("implicit")'))
    assert api.generic_signature(implicit) == sig
    assert api.problem_family(implicit) == "generic"
    for double in (False, True):
        for off32 in (False, True):
            assert api.generic_source(implicit, double, off32) == api.generic_source(SCHUR, double, off32)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("off32", [False, True])
def test_source_has_the_explicit_kernels_only_with_the_statement(double, off32):
    src, base = api.generic_source(EXPLICIT, double, off32), api.generic_source(SCHUR, double, off32)
    for k in ("gen_schur_eblk", "gen_schur_assemble", "gen_schur_assemble_long", "gen_schur_spmv"):
        assert src.count('extern "C" __global__ __launch_bounds__(256) void %s(' % k) == 1
        assert k not in base
    # the statement only adds kernels: the matrix-free ones (right-hand side, back-substitution) stay
    assert src.startswith(base[:base.rindex("}") + 1])
    assert "constexpr int CR = 6, CE = 3" in src


def test_files_without_the_statement_keep_their_source(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_dump_matrix import block_variant
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "generated_source_sha256.json")))
    seen = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "energies", "*.t"))):
        text, name = open(path).read(), os.path.basename(path)[:-2]
        if "ReducedSystem" in text:
            continue
        files = [(name, path)]
        blk = block_variant(text)
        if blk is not None:
            files.append((name + "_block", write(tmp_path, name + "_block.t", blk)))
        for n, f in files:
            for double in (False, True):
                for off32 in (False, True):
                    key = n + (".double" if double else "") + (".off32" if off32 else "")
                    got = hashlib.sha256(api.generic_source(f, double, off32).encode()).hexdigest()
                    assert got == want[key], key
                    seen.add(key)
    assert seen == set(want)


@pytest.mark.parametrize("double", [False, True])
def test_explicit_source_compiles_for_gfx950(double):
    api.generic_compile_check(EXPLICIT, double)     # both gather forms (a.gnb[...] present)
    assert "a.gnb[" in api.generic_source(EXPLICIT, double)


# ------------------------------------------------------------------ refusals of the statement
BA_SCHUR = open(SCHUR).read()
BA = open(os.path.join(ROOT, "energies", "bundle_adjustment.t")).read()
DEFINE_REFUSALS = [
    ("other_form", BA_SCHUR + 'ReducedSystem("dense")\n', 'form is "explicit" or "implicit"'),
    ("number", BA_SCHUR + "ReducedSystem(1)\n", 'form is "explicit" or "implicit"'),
    ("no_argument", BA_SCHUR + "ReducedSystem()\n", 'form is "explicit" or "implicit"'),
    ("second_statement", BA_SCHUR + STATEMENT + "\n" + 'ReducedSystem("implicit")\n', "a second ReducedSystem"),
    ("without_eliminate", BA + STATEMENT + "\n", "ReducedSystem: no Eliminate statement"),
    ("implicit_without_eliminate", BA + 'ReducedSystem("implicit")\n', "ReducedSystem: no Eliminate statement"),
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
local N, M, K, E = Dim("N", 0), Dim("M", 1), Dim("K", 2), Dim("E", 3)
local X = Unknown("X", opt_float3, {N}, 0)
local Y = Unknown("Y", opt_float2, {M}, 1)
local A = Array("A", opt_float3, {N}, 2)
local G = Graph("G", {E}, "i", {N}, 3, "k", {M}, 4, "l", {M}, 5)
Eliminate(X)
ReducedSystem("explicit")
Energy(X(0) - A(0))
"""
PLAN_REFUSALS = [
    ("two_retained_spaces", HEAD.replace('local A =', 'local Z = Unknown("Z", opt_float, {K}, 6)\nlocal A =')
     + "Energy(X(G.i)(0) - Y(G.k)(0))\nEnergy(Y(0))\nEnergy(Z(0))\n",
     "the retained unknowns lie over 2 index spaces ({M}, {K}); the block-sparse S has one block group"),
    ("centred_offset", HEAD + "Energy(X(G.i)(0) - Y(G.k)(0))\nEnergy(Y(1) - Y(0))\n",
     "B is not block-diagonal: a centred residual over {M} reads Y at a non-zero offset"),
    # a pose-pose edge among the retained elements
    ("two_retained_slots", HEAD + "Energy(X(G.i)(0) - Y(G.k)(0))\nEnergy(Y(G.k) - Y(G.l))\nEnergy(Y(0))\n",
     "B is not block-diagonal: a residual of graph 'G' reads {M} through two slots ('k', 'l')"),
]


@pytest.mark.parametrize("name,text,cause", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_plan_refusals_name_their_cause(tmp_path, name, text, cause):
    path = write(tmp_path, name + ".t", text)
    assert api.problem_family(path) == "generic"          # the front end takes the energy
    why = api.generic_plan_check(path)
    print(why)
    assert why.startswith('generic: ReducedSystem("explicit"): ') and cause in why
    # the same energy with the matrix-free form is planned, and emits no explicit kernel either way
    assert api.generic_plan_check(write(tmp_path, name + "_implicit.t", text.replace(STATEMENT, ""))) == ""
    assert "gen_schur_spmv" not in api.generic_source(path)


def test_accepted_neighbours_of_the_plan_refusals(tmp_path):
    """A graph residual that reads only retained unknowns, at one slot, is fine (it adds to B's
    diagonal blocks); so are two graphs' lists over the eliminated space."""
    ok = HEAD + "Energy(X(G.i)(0) - Y(G.k)(0))\nEnergy(0.5 * Y(G.l))\nEnergy(X(G.i)(1) + Y(G.l)(1))\nEnergy(Y(0))\n"
    path = write(tmp_path, "ok.t", ok)
    assert api.generic_plan_check(path) == ""
    assert api.generic_signature(path).endswith("B;S0;RX;")
    src = api.generic_source(path)
    assert "qb.b[1]" in src and "qb.b[2]" not in src      # two instance lists: (i, k) and (i, l)
    for double in (False, True):
        api.generic_compile_check(path, double)


# ------------------------------------------------------------------ the symbolic phase
def numpy_pattern(n_elim, n_ret, lists):
    """Positions, pairs per block in enumeration order, restated with dictionaries."""
    inst = [[] for _ in range(n_elim)]       # per eliminated vertex: (position, retained vertex)
    base = 0
    for ev, rv in lists:
        order = np.argsort(ev, kind="stable")
        for rank, e in enumerate(order):
            inst[ev[e]].append((base + rank, int(rv[e])))
        base += len(ev)
    blocks = {(r, r): [] for r in range(n_ret)}
    for p in range(n_elim):
        for q1, r1 in inst[p]:
            for q2, r2 in inst[p]:
                blocks.setdefault((r1, r2), []).append((q1, q2))
    return blocks


def check_pattern(n_elim, n_ret, lists):
    counts, row_ptr, col_ind, pair_ptr, pairs = api.schur_pattern(n_elim, n_ret, lists)
    want = numpy_pattern(n_elim, n_ret, lists)
    keys = sorted(want)
    assert counts == {"instances": sum(len(ev) for ev, _ in lists), "pairs": sum(len(v) for v in want.values()),
                      "blocks": len(keys)}
    assert [int(c) for c in col_ind] == [c for _, c in keys]
    assert [int(x) for x in row_ptr] == [sum(1 for r, _ in keys if r < row) for row in range(n_ret + 1)]
    assert pair_ptr[0] == 0 and pair_ptr[-1] == counts["pairs"]
    for b, key in enumerate(keys):
        assert [tuple(int(x) for x in pq) for pq in pairs[pair_ptr[b]:pair_ptr[b + 1]]] == want[key], key
    return counts


def test_pattern_of_a_small_graph_with_every_edge_case():
    # point 0: cameras 0, 1 and camera 1 again (a duplicated edge); point 1: seen once, by camera
    # 2; point 2: seen by nobody; camera 3: sees nothing. Edges out of vertex order.
    ev = np.array([1, 0, 0, 0], np.int32)
    rv = np.array([2, 1, 0, 1], np.int32)
    counts = check_pattern(3, 4, [(ev, rv)])
    assert counts == {"instances": 4, "pairs": 3 * 3 + 1, "blocks": 2 * 2 + 1 + 1}
    _, row_ptr, col_ind, pair_ptr, pairs = api.schur_pattern(3, 4, [(ev, rv)])
    assert list(row_ptr) == [0, 2, 4, 5, 6] and list(col_ind) == [0, 1, 0, 1, 2, 3]
    # instance positions: point 0's edges 1, 2, 3 at 0, 1, 2 (cameras 1, 0, 1), point 1's edge at 3
    assert [tuple(p) for p in pairs[pair_ptr[3]:pair_ptr[4]]] == [(0, 0), (0, 2), (2, 0), (2, 2)]     # block (1, 1)
    assert pair_ptr[5] == pair_ptr[6] == 10                                                            # camera 3: B alone
    assert [tuple(p) for p in pairs[pair_ptr[4]:pair_ptr[5]]] == [(3, 3)]


def test_pattern_over_two_lists():
    rng = np.random.default_rng(4)
    lists = [(rng.integers(0, 9, 40).astype(np.int32), rng.integers(0, 6, 40).astype(np.int32)),
             (rng.integers(0, 9, 25).astype(np.int32), rng.integers(0, 6, 25).astype(np.int32))]
    check_pattern(9, 6, lists)


@pytest.mark.parametrize("NC,NP,pairs,blocks", [(5, 131, 600, 17), (70, 9, 5673, 3930)])
def test_pattern_counts_of_the_bundle_fixtures(NC, NP, pairs, blocks):
    """The fixtures of tests/test_schur_gpu.py (built on the host: importing that module needs
    no device). Counts as checked in numpy: sum over points of (observations)^2 pairs, cameras
    sharing a point plus every diagonal block."""
    from tests.test_schur_gpu import bundle
    w = bundle(NC, NP)
    counts = check_pattern(NP, NC, [(w["p"], w["c"])])
    assert counts["pairs"] == pairs == int((np.bincount(w["p"], minlength=NP) ** 2).sum())
    assert counts["blocks"] == blocks and blocks <= NC * NC
    D = np.zeros((NC, NP))
    np.add.at(D, (w["c"], w["p"]), 1)
    assert int((((D @ D.T) > 0) | np.eye(NC, dtype=bool)).sum()) == blocks


def test_pattern_refuses_bad_input_by_name():
    with pytest.raises(api.OptError, match="vertex index outside its space at edge 1"):
        api.schur_pattern(3, 2, [(np.array([0, 3], np.int32), np.array([0, 1], np.int32))])


def test_pattern_refuses_more_pairs_than_an_int_indexes():
    """46 341 observations of one point are 46 341^2 = 2 147 488 281 > 2^31 - 1 pairs: refused,
    with the counts, before anything of that size is allocated."""
    n = 46341
    with pytest.raises(api.OptError, match="%d instance pairs over %d edge instances" % (n * n, n)):
        api.schur_pattern(1, 1, [(np.zeros(n, np.int32), np.zeros(n, np.int32))])
