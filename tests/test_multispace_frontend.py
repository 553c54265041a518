"""CPU: energies whose unknowns and arrays lie over several index spaces (the reference's
UnknownType groups unknown images by IndexSpace, API/src/o.t:999-1019; a graph slot carries
its own space, o.t:1760): the front end lowers bundle_adjustment.t and row_bias.t, gives
every centred residual and every graph slot its space, compiles the per-space kernels for
gfx950, and refuses — with the construct named — a centred residual that mixes spaces, a
slot access into an image of another space, a second Exclude on one space and more than
four unknown-carrying spaces. Energies over one space lower exactly as before
(tests/golden/single_space_frontend.json: signature and template hashes of the twelve
single-space energies, recorded from the commit before this feature)."""
import hashlib
import json
import os

import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def E(name):
    return os.path.join(ROOT, "energies", name + ".t")


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_bundle_adjustment_lowers_with_its_three_spaces():
    d = api.generic_describe(E("bundle_adjustment"))
    dom = [ln.split(" ")[0] for ln in d]
    # priors: 3 channels each of CamR, CamT (cameras) and X (points); 2 reprojection rows
    assert dom == ["centred{NC}"] * 6 + ["centred{NP}"] * 3 + ["graph0{c:{NC},p:{NP},o:{NO}}"] * 2
    # a reprojection row reads CamR (3), CamT (its own channel and z) and X (3)
    assert [ln.split(" ")[1] for ln in d] == ["1"] * 9 + ["8"] * 2
    sig = api.generic_signature(E("bundle_adjustment"))
    assert "G{2,}{9,10,11,}{0,1,2,};" in sig       # slot spaces: cameras, points, observations
    assert api.problem_family(E("bundle_adjustment")) == "generic"
    assert api.problem_family(E("bundle_adjustment"), "LMGPU") == "generic"


def test_row_bias_lowers_with_image_and_row_spaces():
    d = api.generic_describe(E("row_bias"))
    assert [ln.split(" ")[0] for ln in d] == ["graph0{px:{W,H},row:{H}}", "centred{W,H}", "centred{W,H}", "centred{H}"]
    assert [ln.split(" ")[1] for ln in d] == ["2", "2", "2", "1"]
    sig = api.generic_signature(E("row_bias"))
    assert "X0:(I3[0](0,0,0) == 1);" in sig        # the Exclude belongs to the image's space
    assert api.problem_family(E("row_bias")) == "generic"


@pytest.mark.parametrize("name", ["bundle_adjustment", "row_bias"])
@pytest.mark.parametrize("double", [False, True])
def test_generated_kernels_compile_for_gfx950(name, double):
    api.generic_compile_check(E(name), double)     # 64-bit and 32-bit gather addressing
    for off32 in (False, True):
        src = api.generic_source(E(name), double, off32)
        assert "a.snpix[0]" in src and "a.snpix[1]" in src and "a.fbase[1]" in src
        assert ("opt_g32(a.gnb[0]" in src) == off32
        # several spaces run the gather forms only
        assert "gen_apply_strip" not in src.split("\n", 1)[1] and "gen_apply_tiled" not in src.split("\n", 1)[1]
        assert "gen_dump_j_" not in src
        assert "atomic" not in src[src.index("void gen_jtf_graph"):]    # the gathers scatter nothing


BA_HEAD = """
local NC, NP, NO = Dim("NC", 0), Dim("NP", 1), Dim("NO", 2)
local C = Unknown("C", opt_float3, {NC}, 0)
local X = Unknown("X", opt_float3, {NP}, 1)
local C0 = Array("C0", opt_float3, {NC}, 2)
local M = Array("M", opt_float, {NP}, 3)
local G = Graph("G", {NO}, "c", {NC}, 4, "p", {NP}, 5)
"""

BAD = {
    "mixed_centred": (BA_HEAD + "Energy(C(0) - X(0))\n",
                      "centred residual reads arrays over different index spaces"),
    "slot_space": (BA_HEAD + "Energy(X(G.c) - C(G.c))\n",
                   "graph element is in a different index space from image"),
    "two_excludes": (BA_HEAD + "Exclude(eq(M(0), 1))\nExclude(eq(M(0), 2))\nEnergy(C(G.c) - X(G.p))\n",
                     "more than one Exclude over index space {NP}"),
    "computed_array_space": (BA_HEAD + 'local K = ComputedArray("K", {NP}, C(0) * C(0))\nEnergy(X(0) - K(0))\nEnergy(C(0))\n',
                             "ComputedArray 'K' over {NP} reads 'C' over a different index space {NC}"),
    "exclude_without_unknowns": (BA_HEAD + 'local Q = Array("Q", opt_float, {NO}, 6)\nExclude(eq(Q(0), 1))\n'
                                           "Energy(C(G.c) - X(G.p))\n",
                                 "Exclude over index space {NO}, which holds no unknown"),
    "five_spaces": ("".join(f'local N{k} = Dim("N{k}", {k})\nlocal U{k} = Unknown("U{k}", opt_float, {{N{k}}}, {k})\n'
                            f"Energy(U{k}(0))\n" for k in range(5)),
                    "more than 4 index spaces hold unknowns"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_define_refuses_with_the_construct_named(tmp_path, capfd, case):
    text, message = BAD[case]
    path = _write(tmp_path, case + ".t", text)
    capfd.readouterr()
    with pytest.raises(api.OptError, match="Opt_ProblemDefine refused"):
        api.problem_family(path)
    assert message in capfd.readouterr().err


def test_nine_declared_spaces_are_refused(tmp_path, capfd):
    text = 'local N = Dim("N", 0)\nlocal U = Unknown("U", opt_float, {N}, 0)\nEnergy(U(0))\n' + "".join(
        f'local D{k} = Dim("D{k}", {k})\nlocal A{k} = Array("A{k}", opt_float, {{D{k}}}, {k})\n' for k in range(1, 9))
    capfd.readouterr()
    with pytest.raises(api.OptError):
        api.problem_family(_write(tmp_path, "nine.t", text))
    assert "more than 8 index spaces" in capfd.readouterr().err


def test_a_centred_residual_needs_an_unknown_of_its_space(tmp_path):
    with pytest.raises(api.OptError, match=r"index space \{NP\} reads no unknown"):
        api.generic_describe(_write(tmp_path, "known_only.t", BA_HEAD + "Energy(C(0) - C0(0))\nEnergy(M(0))\n"))


def test_known_arrays_may_lie_over_a_space_without_unknowns(tmp_path):
    text = BA_HEAD + 'local Obs = Array("Obs", opt_float3, {NO}, 6)\nlocal H = Graph("H", {NO}, "c", {NC}, 4, "o", {NO}, 7)\n' \
                     "Energy(C(H.c) - Obs(H.o))\nEnergy(C(0) - C0(0))\nEnergy(X(0))\n"
    path = _write(tmp_path, "obs.t", text)
    assert api.problem_family(path) == "generic"
    assert [ln.split(" ")[0] for ln in api.generic_describe(path)] == \
        ["graph1{c:{NC},o:{NO}}"] * 3 + ["centred{NC}"] * 3 + ["centred{NP}"] * 3


def test_single_space_energies_lower_as_before():
    with open(os.path.join(ROOT, "tests", "golden", "single_space_frontend.json")) as f:
        golden = json.load(f)
    assert len(golden) == 12
    for name, g in sorted(golden.items()):
        sig = api.generic_signature(E(name))
        desc = "\n".join(api.generic_describe(E(name)))
        assert hashlib.sha256(sig.encode()).hexdigest() == g["signature_sha256"], name
        assert hashlib.sha256(desc.encode()).hexdigest() == g["describe_sha256"], name
        # and their kernels declare none of the per-space arguments
        for dbl in (False, True):
            src = api.generic_source(E(name), dbl)
            assert "sdims" not in src and "snpix" not in src and "fbase" not in src, name


def flow_with_calibration(tmp_path):
    """optical_flow.t (SampledImage with derivative images: a per-Step sample cache over the
    image's space) plus one unknown per calibration entry over a space of its own."""
    with open(E("optical_flow")) as f:
        text = f.read()
    text += '\nlocal N = Dim("N", 2)\nlocal B = Unknown("B", opt_float, {N}, 7)\nEnergy(B(0) - 0.5)\n'
    return _write(tmp_path, "flow_calibration.t", text)


@pytest.mark.parametrize("double", [False, True])
def test_sample_cache_runs_over_the_sampled_images_space(tmp_path, double):
    import re

    path = flow_with_calibration(tmp_path)
    assert api.problem_family(path, "LMGPU") == "generic"
    d = api.generic_describe(path)
    assert [ln.split(" ")[0] for ln in d] == ["centred{W,H}"] * 9 + ["centred{N}"]
    api.generic_compile_check(path, double)
    src = api.generic_source(path, double)
    assert "[-1]" not in src
    # every space a kernel names is a declared one: {W,H} = 0, {N} = 1
    assert set(re.findall(r"a\.(?:sdims|snpix|fbase)\[(-?\d+)\]", src)) == {"0", "1"}
    # the sample cache (value and the two gradient images) is filled over the image's space
    pre = src[src.index("void gen_precompute_0("):src.index("void gen_jtf(")]
    assert "lin < a.snpix[0]" in pre and "a.snpix[1]" not in pre and "opt_sample(" in pre
    # and no 2-D coordinate or bounds test is left with the 1-D space's loop
    jtf = src[src.index("void gen_jtf("):src.index("void gen_apply(")]
    one_d = jtf[jtf.index("lin < a.snpix[1]"):]
    assert "opt_sample(" not in one_d and " < H" not in one_d
