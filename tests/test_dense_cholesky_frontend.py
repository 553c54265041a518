"""CPU: the LinearSolver("cholesky") statement in the front end — both parsers, the signature
token DC;, the two generated kernels (gen_dense_fill, gen_dense_store) and their compile for
gfx950, the refusals by message — and the shipped files without the statement, none of which
gains a kernel or the token (their source digests: tests/test_schur_explicit_frontend.py against
tests/golden/generated_source_sha256.json). No device: Opt_ProblemDefine, the OptAMD_Generic* calls, hiprtc."""
import glob
import os

import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = lambda *p: os.path.join(ROOT, "energies", *p)
BA_EXPLICIT, BA_CHOLESKY = E("bundle_adjustment_schur_explicit.t"), E("direct", "bundle_adjustment_schur_cholesky.t")
PG_EXPLICIT, PG_CHOLESKY = E("normal_matrix", "pose_graph_2d_explicit.t"), E("direct", "pose_graph_2d_cholesky.t")
PAIRS = [(BA_EXPLICIT, BA_CHOLESKY, "RX;"), (PG_EXPLICIT, PG_CHOLESKY, "NX;")]
STATEMENT = 'LinearSolver("cholesky")'
KERNELS = ("gen_dense_fill", "gen_dense_store")


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


@pytest.mark.parametrize("explicit,cholesky,token", PAIRS, ids=("bundle", "pose_graph"))
def test_statement_and_signature_token(tmp_path, explicit, cholesky, token):
    base, text = open(explicit).read(), open(cholesky).read()
    assert [ln for ln in code_lines(text) if ln != STATEMENT] == code_lines(base)
    assert code_lines(text).count(STATEMENT) == 1
    sig = api.generic_signature(explicit)
    assert sig.endswith(token)
    assert api.generic_signature(cholesky) == sig + "DC;"
    assert api.generic_describe(cholesky) == api.generic_describe(explicit)
    for kind in ("gaussNewtonGPU", "LMGPU"):
        assert api.problem_family(cholesky, kind) == "generic"
    assert api.generic_plan_check(cholesky) == ""
    # the statement first: the same file
    first = write(tmp_path, "first.t", text.replace(STATEMENT + "\n", "").replace("Energy(", STATEMENT + "\nEnergy(", 1))
    assert api.generic_signature(first) == sig + "DC;"
    assert api.generic_source(first) == api.generic_source(cholesky)
    # "pcg" is the file without the statement: signature, routing and source
    pcg = write(tmp_path, "pcg.t", text.replace(STATEMENT, 'LinearSolver("pcg")'))
    assert api.generic_signature(pcg) == sig
    assert api.problem_family(pcg) == "generic"
    for double in (False, True):
        for off32 in (False, True):
            assert api.generic_source(pcg, double, off32) == api.generic_source(explicit, double, off32)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("off32", [False, True])
@pytest.mark.parametrize("explicit,cholesky,token", PAIRS, ids=("bundle", "pose_graph"))
def test_source_has_the_dense_kernels_only_with_the_statement(explicit, cholesky, token, double, off32):
    src, base = api.generic_source(cholesky, double, off32), api.generic_source(explicit, double, off32)
    for k in KERNELS:
        assert src.count('extern "C" __global__ __launch_bounds__(256) void %s(' % k) == 1
        assert k not in base
    assert src.startswith(base)                     # the statement only adds the two kernels, at the end
    assert "atomic" not in src[len(base):]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("cholesky", [BA_CHOLESKY, PG_CHOLESKY], ids=("bundle", "pose_graph"))
def test_dense_kernels_compile_for_gfx950(cholesky, double):
    api.generic_compile_check(cholesky, double)


def test_no_other_shipped_energy_has_the_kernels():
    files = [f for f in glob.glob(E("**", "*.t"), recursive=True) if STATEMENT not in open(f).read()]
    assert len(files) >= 20
    for f in files:
        src = api.generic_source(f)
        assert not any(k in src for k in KERNELS), f
        assert "DC;" not in api.generic_signature(f), f


BA_X = open(BA_EXPLICIT).read()
PG_X = open(PG_EXPLICIT).read()
BA = open(E("bundle_adjustment.t")).read()
BA_SCHUR = open(E("bundle_adjustment_schur.t")).read()
NEITHER = 'the file has neither ReducedSystem("explicit") nor NormalMatrix("explicit")'
REFUSALS = [
    ("other_kind", BA_X + 'LinearSolver("lu")\n', 'kind is "cholesky" or "pcg"'),
    ("number", PG_X + "LinearSolver(1)\n", 'kind is "cholesky" or "pcg"'),
    ("no_argument", BA_X + "LinearSolver()\n", 'kind is "cholesky" or "pcg"'),
    ("two_arguments", BA_X + 'LinearSolver("cholesky", "pcg")\n', 'kind is "cholesky" or "pcg"'),
    ("second_statement", BA_X + STATEMENT + "\n" + STATEMENT + "\n", "a second LinearSolver"),
    ("second_statement_pcg", PG_X + 'LinearSolver("pcg")\n' + STATEMENT + "\n", "a second LinearSolver"),
    ("plain_energy", BA + STATEMENT + "\n", NEITHER),
    ("implicit_schur", BA_SCHUR + STATEMENT + "\n", NEITHER),
    ("implicit_statement", BA_SCHUR + 'ReducedSystem("implicit")\n' + STATEMENT + "\n", NEITHER),
    ("matrix_free", PG_X.replace('NormalMatrix("explicit")', 'NormalMatrix("matrix_free")') + STATEMENT + "\n", NEITHER),
]


@pytest.mark.parametrize("name,text,cause", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_front_end_refusals_name_their_cause(tmp_path, capfd, name, text, cause):
    path = write(tmp_path, name + ".t", text)
    capfd.readouterr()
    with pytest.raises(api.OptError, match="Opt_ProblemDefine refused"):
        api.problem_family(path)
    err = capfd.readouterr().err
    print(err)
    assert cause in err


def test_pcg_needs_no_explicit_statement(tmp_path):
    """LinearSolver("pcg") is a no-op in any file."""
    path = write(tmp_path, "ba_pcg.t", BA + 'LinearSolver("pcg")\n')
    assert api.generic_signature(path) == api.generic_signature(E("bundle_adjustment.t"))
    assert api.generic_source(path) == api.generic_source(E("bundle_adjustment.t"))
