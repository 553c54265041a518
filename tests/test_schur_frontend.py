"""CPU: the Eliminate(X, ...) statement in the front end (both parsers, the signature, the
generated source, the compile, the refusals). No device: everything here goes through
Opt_ProblemDefine, OptAMD_GenericSource and hiprtc.

The plan-time refusals (useMaterializedJTJ / useFusedJTJ) are in tests/test_schur_gpu.py:
Opt_ProblemPlan asks for a HIP device before it looks at the energy."""
import hashlib
import os

import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = os.path.join(ROOT, "energies", "bundle_adjustment.t")
SCHUR = os.path.join(ROOT, "energies", "bundle_adjustment_schur.t")

# sha256 of OptAMD_GenericSource for bundle_adjustment.t and its UsePreconditioner("block")
# variant on the commit before Eliminate existed: (double, off32) -> digest
PARENT_SOURCE = {
    "scalar": {(False, False): "ee7c785e60b99b1c0dab60eb970b54b101be190c0cdef95d08cbe81679bd06ba",
               (False, True): "70198a680b33ab7df334740b71597eeb8200a75b3e9f5580c36e47915299da1a",
               (True, False): "0306ef5dc48e80e8ee81c5bb9a2b1a6fb5b7ce166c82ebc45f5f1359e8d9810b",
               (True, True): "90b9d45a3a9d0832f179e94ffb61e59c4ab8cea8d2628e3d260360114888788c"},
    "block": {(False, False): "00f96d678c3da7647314fd33065d6ab3eecc7be0f90a0951fa2df5fced49a06e",
              (False, True): "cb4c2f4774fda958f6b0cc1bba19616598c7ce7139d40a88b953325153d506ef",
              (True, False): "470cee6122ed98d4f814f0f198ff7c8e54b711ec12353482e9b2ededc0c1465f",
              (True, True): "1660725f8ce8aa9ffda340d46745a4fd4d5002c88585aba751dfc237167256ac"},
}


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in list(os.environ):
        if k.startswith("OPT_AMD_GEN_"):
            monkeypatch.delenv(k)


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def block_variant(tmp_path):
    text = open(BA).read()
    assert text.count("UsePreconditioner(true)") == 1
    return write(tmp_path, "ba_block.t", text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))


def test_statement_keeps_the_energy_and_marks_the_signature(tmp_path):
    ba, schur = open(BA).read(), open(SCHUR).read()
    code = [ln for ln in schur.splitlines() if ln.strip() and not ln.startswith("--")]
    assert [ln for ln in code if ln != "Eliminate(X)"] == [ln for ln in ba.splitlines() if ln.strip() and not ln.startswith("--")]
    assert code.count("Eliminate(X)") == 1
    assert api.generic_describe(SCHUR) == api.generic_describe(BA)
    blk = api.generic_signature(block_variant(tmp_path))
    assert blk.endswith("B;")
    assert api.generic_signature(SCHUR) == blk + "S1;"          # {NP} is the second index space
    assert api.problem_family(SCHUR) == "generic" and api.problem_family(SCHUR, "LMGPU") == "generic"
    # the statement alone turns the block preconditioner on, wherever UsePreconditioner stands
    for text in (schur.replace("UsePreconditioner(true)\n", ""),
                 schur.replace("UsePreconditioner(true)\nEliminate(X)", "Eliminate(X)\nUsePreconditioner(false)")):
        assert text != schur
        assert api.generic_signature(write(tmp_path, "v.t", text)) == blk + "S1;"


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("off32", [False, True])
def test_source_has_the_schur_kernels_and_other_files_keep_theirs(tmp_path, double, off32):
    src = api.generic_source(SCHUR, double, off32)
    for k in ("gen_schur_rhs", "gen_schur_elim", "gen_schur_apply"):
        assert src.count('extern "C" __global__ __launch_bounds__(256) void %s(' % k) == 1
    assert ("opt_g32(w + " in src) == off32        # eliminated reads come from w, by a literal of the read
    for name, path in (("scalar", BA), ("block", block_variant(tmp_path))):
        other = api.generic_source(path, double, off32)
        assert "gen_schur" not in other and "q0[1]" not in other
        assert hashlib.sha256(other.encode()).hexdigest() == PARENT_SOURCE[name][(double, off32)], name


@pytest.mark.parametrize("double", [False, True])
def test_schur_source_compiles_for_gfx950(double):
    api.generic_compile_check(SCHUR, double)     # both gather forms (a.gnb[...] present)
    assert "a.gnb[" in api.generic_source(SCHUR, double)


HEAD = """
local N, M, E = Dim("N", 0), Dim("M", 1), Dim("E", 2)
local X = Unknown("X", opt_float3, {N}, 0)
local Y = Unknown("Y", opt_float2, {M}, 1)
local A = Array("A", opt_float3, {N}, 2)
local G = Graph("G", {E}, "i", {N}, 3, "j", {N}, 4, "k", {M}, 5)
"""
COUPLE = "Energy(X(G.i)(0) - Y(G.k)(0))\nEnergy(Y(0))\n"
BA_TEXT = open(BA).read()

REFUSALS = [
    ("array_argument", HEAD + "Eliminate(A)\nEnergy(X(0) - A(0))\n" + COUPLE, "argument 1 is not an unknown image"),
    ("number_argument", HEAD + "Eliminate(X, 3)\nEnergy(X(0) - A(0))\n" + COUPLE, "argument 2 is not an unknown image"),
    ("camr_without_camt", BA_TEXT + "Eliminate(CamR)\n", "unknown CamT over {NC} is not named"),
    ("two_spaces", BA_TEXT + "Eliminate(CamT, X)\n", "lie over different index spaces"),
    ("nothing_remains", """
local N = Dim("N", 0)
local X = Unknown("X", opt_float3, {N}, 0)
local A = Array("A", opt_float3, {N}, 1)
Eliminate(X)
Energy(X(0) - A(0))
""", "no unknown-carrying index space would remain beside {N}"),
    ("second_statement", BA_TEXT + "Eliminate(X)\nEliminate(X)\n", "a second Eliminate"),
    ("centred_offset", HEAD + "Eliminate(X)\nEnergy(X(1) - X(0))\n" + COUPLE,
     "a centred residual over {N} reads X at a non-zero offset"),
    # a pose-graph style residual: both ends of an edge lie in the group's space
    ("two_slots", HEAD + "Eliminate(X)\nEnergy(X(0) - A(0))\nEnergy(X(G.i) - X(G.j) + Y(G.k)(0))\nEnergy(Y(0))\n",
     "a residual of graph 'G' reads {N} through two slots ('i', 'j')"),
    ("computed_array_offset", HEAD + 'local B = ComputedArray("B", {N}, X(1)(0) - X(0)(0))\nEliminate(X)\nEnergy(B(0))\n' + COUPLE,
     "ComputedArray 'B' depends on X at an offset"),
    ("nine_channels", """
local N, M, E = Dim("N", 0), Dim("M", 1), Dim("E", 2)
local X1 = Unknown("X1", opt_float3, {N}, 0)
local X2 = Unknown("X2", opt_float3, {N}, 1)
local X3 = Unknown("X3", opt_float3, {N}, 2)
local Y = Unknown("Y", opt_float2, {M}, 3)
local G = Graph("G", {E}, "i", {N}, 4, "k", {M}, 5)
Eliminate(X1, X2, X3)
Energy(X1(G.i)(0) + X2(G.i)(1) + X3(G.i)(2) - Y(G.k)(0))
Energy(X1(0)) Energy(X2(0)) Energy(X3(0)) Energy(Y(0))
""", "index space {N} holds 9 unknown channels (a block has at most 8)"),
]


@pytest.mark.parametrize("name,text,cause", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_their_cause(tmp_path, capfd, name, text, cause):
    path = write(tmp_path, name + ".t", text)
    capfd.readouterr()
    with pytest.raises(api.OptError, match="Opt_ProblemDefine refused"):
        api.problem_family(path)
    err = capfd.readouterr().err
    print(err)
    assert cause in err


def test_accepted_neighbours_of_the_refusals(tmp_path):
    """The refusals above are about the group, not about the energies' other features."""
    ok = HEAD + "Eliminate(X)\nEnergy(X(0) - A(0))\n" + COUPLE
    assert api.problem_family(write(tmp_path, "ok.t", ok)) == "generic"
    assert api.generic_signature(write(tmp_path, "ok.t", ok)).endswith("B;S0;")
    # an offset read of a retained unknown, and two slots over a retained space, are fine
    ok2 = HEAD + "Eliminate(Y)\nEnergy(X(1) - X(0))\nEnergy(X(G.i) - X(G.j) + Y(G.k)(0))\nEnergy(Y(0))\n"
    assert api.generic_signature(write(tmp_path, "ok2.t", ok2)).endswith("B;S1;")
    for double in (False, True):
        api.generic_compile_check(write(tmp_path, "ok2.t", ok2), double)
