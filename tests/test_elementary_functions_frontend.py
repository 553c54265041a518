"""CPU: the rest of the DSL's elementary functions through the front end (ad.t:840-856):
tan tanh sinh cosh asin acos atan asinh acosh log10 and atan2, by bare name and as ad.<name>,
lowered, printed by name, compiled for gfx950 in both precisions; constant arguments fold on
the host; the energies that existed before keep their signatures; energies/pose_graph_2d.t
lowers as documented, with the scalar and with the block preconditioner.

atan2 is the C library's atan2(y, x) (the reference's own definition
evaluates atan2(x*x + y*y, y) and has the sign of its second partial wrong)."""
import hashlib
import json
import math
import os
import re

import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNARY = ["tan", "tanh", "sinh", "cosh", "asin", "acos", "atan", "asinh", "acosh", "log10"]
FUNCTIONS = UNARY + ["atan2"]


def E(name):
    return os.path.join(ROOT, "energies", name + ".t")


def one_line_energy(f, prefix=""):
    """Energy(f(X(0)) - D(0)) over a 1-D space; atan2 takes two channels of X."""
    if f == "atan2":
        return ('local N = Dim("N", 0)\nlocal X = Unknown("X", opt_float2, {N}, 0)\n'
                'local D = Array("D", opt_float, {N}, 1)\n'
                "Energy(%satan2(X(0, 0), X(0, 1)) - D(0))\n" % prefix)
    return ('local N = Dim("N", 0)\nlocal X = Unknown("X", opt_float, {N}, 0)\n'
            'local D = Array("D", opt_float, {N}, 1)\n'
            "Energy(%s%s(X(0)) - D(0))\n" % (prefix, f))


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@pytest.mark.parametrize("f", FUNCTIONS)
def test_each_function_lowers_and_compiles(tmp_path, f):
    path = _write(tmp_path, f + ".t", one_line_energy(f))
    sig = api.generic_signature(path)
    assert sig
    d = api.generic_describe(path)
    assert len(d) == 1 and d[0].startswith("centred ")
    assert re.search(r"\b%s\(" % f, d[0]), d[0]          # printed by name (atan is not atan2, asin not sin ...)
    assert api.problem_family(path) == "generic"
    for double in (False, True):
        api.generic_compile_check(path, double)
        src = api.generic_source(path, double)
        assert re.search(r"= %s\(t\d+" % f, src), f       # the overloaded device function, on T
    # the ad.<name> spelling is the same function
    assert api.generic_signature(_write(tmp_path, "ad_" + f + ".t", one_line_energy(f, "ad."))) == sig


@pytest.mark.parametrize("f", FUNCTIONS)
def test_derivative_reuses_the_function_where_it_appears(tmp_path, f):
    """tan' = 1 + tan^2 and tanh' = 1 - tanh^2 are built from the node itself: the kernels
    evaluate the function once per read. sinh / cosh differentiate into each other; the rest
    have algebraic derivatives and call no second function."""
    src = api.generic_source(_write(tmp_path, f + ".t", one_line_energy(f)))
    jtf = src[src.index("void gen_jtf("):src.index("void gen_apply(")]
    calls = re.findall(r"= ([a-z0-9]+)\(t\d+", jtf)
    expect = {"sinh": ["cosh", "sinh"], "cosh": ["cosh", "sinh"], "asin": ["asin", "sqrt"], "acos": ["acos", "sqrt"],
              "asinh": ["asinh", "sqrt"], "acosh": ["acosh", "sqrt"]}.get(f, [f])
    assert sorted(calls) == expect, calls


MASKED = ('local W,H = Dim("W",0), Dim("H",1)\nlocal X = Unknown("X", opt_float, {W,H}, 0)\n'
          'local D = Array("D", opt_float, {W,H}, 1)\nlocal Mask = Array("Mask", opt_float, {W,H}, 2)\n'
          "Energy(Select(InBounds(1,0), X(0,0) - X(1,0), 0))\n"
          "Energy(Select(eq(Mask(0,0),0), %s - D(0,0), 0))\n")


@pytest.mark.parametrize("f", FUNCTIONS)
def test_mask_is_factored_onto_jp_only_where_no_partial_can_be_non_finite(tmp_path, f):
    """The strip apply evaluates a masked residual's mask once (m<k>) and applies it to Jp alone
    only when no partial can be NaN / Inf where the mask is off. tan sinh cosh asin acos acosh
    log10 can be (out of domain, overflow, on whatever the masked pixels hold), and the
    partials of atan asinh atan2 hold a division: all keep the Select per partial. tanh is
    finite everywhere and its partial 1 - tanh^2 has no division: it is factored."""
    call = "atan2(X(0,0), D(0,0))" if f == "atan2" else f + "(X(0,0))"
    src = api.generic_source(_write(tmp_path, "m_" + f + ".t", MASKED % call))
    assert "void gen_apply_strip(" in src
    strip = src[src.index("void gen_apply_strip("):]
    strip = strip[:strip.index('extern "C"')]
    assert ("const bool m1 = " in strip) == (f == "tanh"), f


def test_cached_reads_outside_the_image_take_f_of_zero(tmp_path):
    """A cached transcendental of a centred read is f(0) outside the image, the value the
    uncached expression has there (reads outside are 0): cosh 1, acos pi / 2, log10 -inf,
    acosh NaN, tan 0."""
    want = {"cosh": "((T)1.0)", "acos": "((T)%.17g)" % (math.pi / 2), "log10": "(-(T)__builtin_huge_val())",
            "acosh": '((T)__builtin_nan(""))', "tan": "((T)0.0)", "asin": "((T)0.0)"}
    for f, lit in want.items():
        text = ('local W,H = Dim("W",0), Dim("H",1)\nlocal X = Unknown("X", opt_float, {W,H}, 0)\n'
                "Energy(%s(X(0,0)) - %s(X(1,0)))\nEnergy(X(0,0) - X(0,1))\n" % (f, f))
        path = _write(tmp_path, "c_" + f + ".t", text)
        src = api.generic_source(path)
        cost = src[src.index("void gen_cost("):]
        cost = cost[:cost.index('extern "C"')]
        assert re.search(r"\? \(\(const T\*\)a\.img\[\d+\]\)\[li \+ \(1\)\] : " + re.escape(lit) + ";", cost), (f, lit)
        api.generic_compile_check(path)


def test_constants_fold(tmp_path):
    head = 'local N = Dim("N", 0)\nlocal X = Unknown("X", opt_float, {N}, 0)\n'
    lit = api.generic_describe(_write(tmp_path, "lit.t", head + "Energy(X(0) - %r)\n" % (math.pi / 4)))
    for k, expr in enumerate(["math.atan2(1, 1)", "atan(1)", "ad.atan(1)", "atan2(1, 1)", "math.atan(1)",
                              "asin(math.sin(math.pi / 4))", "acos(0) / 2"]):
        d = api.generic_describe(_write(tmp_path, "c%d.t" % k, head + "Energy(X(0) - %s)\n" % expr))
        if expr in ("math.atan2(1, 1)", "atan(1)"):
            assert d == lit, (expr, d, lit)               # the same template as the literal pi / 4
        assert len(d) == 1 and not re.search(r"[a-z0-9]\(", d[0].split(" ", 2)[2].replace("inbox", "")), d
        v = float(re.search(r"- ([0-9.e+-]+)\)", d[0]).group(1))
        assert v == pytest.approx(math.pi / 4, rel=1e-5)  # (printed with 6 digits)
    # every host-number function, against Python's
    body = "\n".join("assert(math.abs(math.%s(%s) - %r) < 1e-15, '%s')" % (f, a, getattr(math, f)(a), f)
                     for f, a in [("tan", 0.5), ("tanh", 0.5), ("sinh", 0.5), ("cosh", 0.5), ("asin", 0.5),
                                  ("acos", 0.5), ("atan", 0.5), ("asinh", 0.5), ("acosh", 1.5), ("log10", 0.5)])
    body += "\nassert(math.abs(math.atan2(-1, -2) - %r) < 1e-15, 'atan2')\n" % math.atan2(-1, -2)
    assert len(api.generic_describe(_write(tmp_path, "m.t", head + body + "Energy(X(0))\n"))) == 1


def test_existing_energies_keep_their_signatures():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "single_space_frontend.json")))
    seen = 0
    for f in sorted(os.listdir(os.path.join(ROOT, "energies"))):
        name = f[:-2]
        if not f.endswith(".t") or name not in golden:
            continue
        seen += 1
        sig = api.generic_signature(E(name))
        assert hashlib.sha256(sig.encode()).hexdigest() == golden[name]["signature_sha256"], name
    assert seen == len(golden) == 12


def block_variant(tmp_path):
    text = open(E("pose_graph_2d")).read()
    assert text.count("UsePreconditioner(true)") == 1
    return _write(tmp_path, "pose_graph_2d_block.t", text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))


def test_pose_graph_lowers_and_compiles(tmp_path):
    """One centred term (the anchor prior, a row per channel of the pose) and three graph
    residuals over {N} / {E}; the angle row is the wrapped one."""
    path = E("pose_graph_2d")
    assert api.problem_family(path) == "generic" and api.problem_family(path, "LMGPU") == "generic"
    d = api.generic_describe(path)
    assert [ln.split(" ")[0] for ln in d] == ["centred{N}"] * 3 + ["graph0{i:{N},j:{N},e:{E}}"] * 3
    assert [ln.split(" ")[1] for ln in d] == ["1", "1", "1", "6", "6", "2"]
    assert all("atan2(sin(" in ln for ln in d[3:]) and not any("atan2" in ln for ln in d[:3])
    blk = block_variant(tmp_path)
    assert api.generic_describe(blk) == d
    assert api.generic_signature(blk) == api.generic_signature(path) + "B;"
    assert api.problem_family(blk) == "generic"
    for double in (False, True):
        api.generic_compile_check(path, double)
        api.generic_compile_check(blk, double)
        src = api.generic_source(blk, double)
        # one block group, the pose's three channels
        assert re.search(r"struct OptGroup0 \{\s*static constexpr int C = 3;", src) and "OptGroup1" not in src
        assert "gen_blk_apply" in src and "gen_blk_apply" not in api.generic_source(path, double)
