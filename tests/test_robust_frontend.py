"""CPU: the RobustEnergy statement in the front end — lowering of the two shipped robust
energies, the loss group in OptAMD_GenericDescribe and the signature, the generated source
(the weights kernel, and the gathers loading the weight instead of recomputing it), its
compile for gfx950 in both precisions and both gather forms, every refusal by name, and the
statement beside the explicitly formed S and H. No device: Opt_ProblemDefine, the
OptAMD_Generic* calls and hiprtc."""
import os
import re

import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = os.path.join(ROOT, "energies", "pose_graph_2d.t")
BA = os.path.join(ROOT, "energies", "bundle_adjustment.t")
PG_CAUCHY = os.path.join(ROOT, "energies", "robust", "pose_graph_2d_cauchy.t")
BA_HUBER = os.path.join(ROOT, "energies", "robust", "bundle_adjustment_huber.t")
KERNEL = 'extern "C" __global__ __launch_bounds__(256) void %s('


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in list(os.environ):
        if k.startswith("OPT_AMD_GEN_"):
            monkeypatch.delenv(k)


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def kernel_body(src, name):
    """The text of one generated kernel (to the brace that closes it, in column 0)."""
    at = src.index(KERNEL % name)
    return src[at:src.index("\n}\n", at) + 3]


# ------------------------------------------------------------------ the statement
def test_both_energies_lower_to_the_generated_kernels():
    for path in (PG_CAUCHY, BA_HUBER):
        assert api.problem_family(path) == "generic" and api.problem_family(path, "LMGPU") == "generic"
        assert api.generic_plan_check(path) == ""


def test_describe_shows_the_group():
    pg, plain = api.generic_describe(PG_CAUCHY), api.generic_describe(PG)
    assert pg[-1] == "loss0 graph0 cauchy scale=1.5 residuals=3"
    assert len(pg) == len(plain) + 1 and not any(ln.startswith("loss") for ln in plain)
    # the group's templates are W0 * (the plain file's), the anchor prior is untouched
    assert pg[:3] == plain[:3]
    for k in range(3, 6):
        dom, n, expr = plain[k].split(" ", 2)
        assert pg[k] == "%s %s (W0 * %s)" % (dom, n, expr)
    ba = api.generic_describe(BA_HUBER)
    assert ba[-1] == "loss0 graph0 huber scale=param huber residuals=2"
    assert sum("W0" in ln for ln in ba[:-1]) == 2


def test_signature_ends_in_the_loss_suffix():
    assert api.generic_signature(PG_CAUCHY).endswith("L0:cauchy:3;")
    assert api.generic_signature(BA_HUBER).endswith("B;L0:huber:2;")
    for plain in (PG, BA):
        assert not re.search(r"L\d+:(huber|cauchy):\d+;", api.generic_signature(plain))
    assert api.generic_signature(PG_CAUCHY) != api.generic_signature(PG)


def test_the_robust_files_are_the_plain_ones_with_the_statement():
    def code(path):
        return [ln for ln in open(path).read().splitlines() if ln.strip() and not ln.startswith("--")]
    pg, plain = code(PG_CAUCHY), code(PG)
    assert pg[:-4] == plain[:-3] and pg[-4].startswith('RobustEnergy("cauchy", 1.5,')
    assert "".join(pg[-4:]).replace(" ", "") == 'RobustEnergy("cauchy",1.5,' + ",".join(
        ln[len("Energy("):-1] for ln in plain[-3:]).replace(" ", "") + ")"
    ba, plain = code(BA_HUBER), code(BA)
    assert 'local huber = Param("huber", float, 12)' in ba and 'UsePreconditioner("block")' in ba
    assert ba[-1] == 'RobustEnergy("huber", huber, q(0) / q(2) - m(0), q(1) / q(2) - m(1))'
    assert [ln for ln in ba[:-1] if "huber" not in ln and "UsePreconditioner" not in ln] == \
           [ln for ln in plain[:-2] if "UsePreconditioner" not in ln]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("path", [PG_CAUCHY, BA_HUBER], ids=["pose_graph_cauchy", "bundle_huber"])
def test_source_compiles_for_gfx950(path, double):
    api.generic_compile_check(path, double)          # both gather forms (a.gnb[...] present)
    assert "a.gnb[" in api.generic_source(path, double)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("off32", [False, True])
def test_weights_kernel_once_and_the_gathers_load_the_weight(double, off32):
    for robust, plain in ((PG_CAUCHY, PG), (BA_HUBER, BA)):
        src, base = api.generic_source(robust, double, off32), api.generic_source(plain, double, off32)
        assert src.count(KERNEL % "gen_loss_weights") == 1 and "gen_loss_weights" not in base
        assert "lwq" not in base and "lwe" not in base and "lpos" not in base
        for k in ("gen_apply_graph", "gen_jtf_graph"):
            body, plain_body = kernel_body(src, k), kernel_body(base, k)
            # the weight is loaded at q, in the incidence order, not recomputed: no sqrt or log
            # that the plain file's gather does not have
            for fn in ("sqrt(", "log(", "log1p("):
                assert body.count(fn) == plain_body.count(fn), (k, fn)
            assert "a.lwq[" in body and "a.lwe[" not in body and "a.lpos[" not in body
        w = kernel_body(src, "gen_loss_weights")
        assert "a.lwe[0])[e] = lw;" in w and w.count("a.lpos[") == w.count("a.lwq[") >= 1
        # the cost takes rho from the raw residuals and never reads the cached weights
        c = kernel_body(src, "gen_cost")
        assert "rho0" in c and "a.lwq[" not in c and "a.lwe[" not in c
    # one incidence-order copy per slot that carries the group's unknowns: poses i and j;
    # cameras and points (the observation slot carries none)
    assert kernel_body(api.generic_source(PG_CAUCHY), "gen_loss_weights").count("a.lwq[") == 2
    assert kernel_body(api.generic_source(BA_HUBER), "gen_loss_weights").count("a.lwq[") == 2


# ------------------------------------------------------------------ refusals
PGT = open(PG).read()
ROWS = ("u0(0) * e0 + u0(1) * e1 + u0(2) * e2", "u1(0) * e1 + u1(1) * e2", "u1(2) * e2")
HEADPG = PGT[:PGT.index("Energy(u0(0)")]
TWO_GRAPHS = """
local N, E, F = Dim("N", 0), Dim("E", 1), Dim("F", 2)
local X = Unknown("X", opt_float3, {N}, 0)
local G = Graph("G", {E}, "i", {N}, 1, "j", {N}, 2)
local K = Graph("K", {F}, "a", {N}, 3, "b", {N}, 4)
Energy(X(0))
RobustEnergy("huber", 1.0, X(G.i) - X(G.j), X(K.a)(0) - X(K.b)(0))
"""
DEFINE_REFUSALS = [
    ("unknown_kind", HEADPG + 'RobustEnergy("tukey", 1.5, %s)\n' % ROWS[0], 'kind is "huber" or "cauchy" (got "tukey")'),
    ("kind_not_a_string", HEADPG + "RobustEnergy(1.5, 1.5, %s)\n" % ROWS[0], 'kind is "huber" or "cauchy"'),
    ("zero_scale", HEADPG + 'RobustEnergy("huber", 0, %s)\n' % ROWS[0], "the scale must be positive (got 0)"),
    ("negative_scale", HEADPG + 'RobustEnergy("cauchy", -1.5, %s)\n' % ROWS[0], "the scale must be positive (got -1.5)"),
    ("string_scale", HEADPG + 'RobustEnergy("cauchy", "wide", %s)\n' % ROWS[0],
     "the scale is a positive number or a float Param"),
    ("expression_scale", HEADPG + 'RobustEnergy("cauchy", 2 * w_anchor, %s)\n' % ROWS[0],
     "the scale is a positive number or a float Param"),
    ("int_param_scale", HEADPG + 'local k = Param("k", int, 10)\nRobustEnergy("cauchy", k, %s)\n' % ROWS[0],
     "the scale is a positive number or a float Param"),
    ("no_terms", HEADPG + 'RobustEnergy("huber", 1.5)\n', "RobustEnergy: no terms"),
    ("centred_term", HEADPG + 'RobustEnergy("huber", 1.5, %s, P(0)(0) - P0(0)(0))\n' % ROWS[0],
     "RobustEnergy: term 2 of statement 1 is a centred (non-graph) term"),
    ("two_graphs", TWO_GRAPHS, "RobustEnergy: term 4 of statement 1 reads graph 'K', the terms before it graph 'G'"),
    ("fifth_group", HEADPG + "".join('RobustEnergy("huber", %d.5, %s)\n' % (k, ROWS[k % 3]) for k in range(5)),
     "RobustEnergy: more than 4 loss groups in one energy"),
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


def test_accepted_neighbours_of_the_refusals(tmp_path):
    """Four groups, a float Param scale, and a statement per row are all taken."""
    four = write(tmp_path, "four.t", HEADPG + "".join('RobustEnergy("huber", %d.5, %s)\n' % (k, ROWS[k % 3])
                                                      for k in range(4)))
    assert api.problem_family(four) == "generic"
    assert api.generic_signature(four).endswith("L0:huber:1;L0:huber:1;L0:huber:1;L0:huber:1;")
    assert [ln for ln in api.generic_describe(four) if ln.startswith("loss")] == \
           ["loss%d graph0 huber scale=%d.5 residuals=1" % (k, k) for k in range(4)]
    src = api.generic_source(four)
    assert kernel_body(src, "gen_loss_weights").count("a.lwe[") == 4
    api.generic_compile_check(four)
    prm = write(tmp_path, "param.t", HEADPG + 'RobustEnergy("cauchy", w_anchor, %s)\n' % ", ".join(ROWS))
    assert api.generic_describe(prm)[-1] == "loss0 graph0 cauchy scale=param w_anchor residuals=3"


# ------------------------------------------------------------------ beside the explicit forms
@pytest.mark.parametrize("double", [False, True])
def test_statement_beside_the_explicit_forms(tmp_path, double):
    ba = open(BA_HUBER).read()
    assert ba.count('UsePreconditioner("block")') == 1
    sx = write(tmp_path, "ba_huber_explicit.t",
               ba.replace('UsePreconditioner("block")', 'UsePreconditioner("block")\nEliminate(X)\nReducedSystem("explicit")'))
    assert api.problem_family(sx) == "generic" and api.generic_plan_check(sx) == ""
    assert api.generic_signature(sx).endswith("B;S1;RX;L0:huber:2;")
    src = api.generic_source(sx, double)
    assert "a.lwq[" in kernel_body(src, "gen_schur_eblk") and "sqrt(" not in kernel_body(src, "gen_schur_eblk")
    for k in ("gen_schur_elim", "gen_schur_apply"):
        assert "a.lwq[" in kernel_body(src, k)
    api.generic_compile_check(sx, double)
    pg = open(PG_CAUCHY).read()
    nx = write(tmp_path, "pg_cauchy_explicit.t", pg.replace("UsePreconditioner(true)", 'NormalMatrix("explicit")'))
    assert pg.count("UsePreconditioner(true)") == 1
    assert api.problem_family(nx) == "generic" and api.generic_plan_check(nx) == ""
    assert api.generic_signature(nx).endswith("B;NX;L0:cauchy:3;")
    src = api.generic_source(nx, double)
    # the per-edge pass reads the edge-order copy
    assert "a.lwe[0])[e]" in kernel_body(src, "gen_normal_eblk") and "a.lwq[" not in kernel_body(src, "gen_normal_eblk")
    api.generic_compile_check(nx, double)
