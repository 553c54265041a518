"""CPU: UsePreconditioner("block") through the front end — the statement, the routing, the
signature mark, the generated block kernels (compiled for gfx950 with hiprtc, no device) and
the C <= 8 refusal. Energy variants are copies of the shipped files with the statement
replaced (row_bias.t has none: it is added)."""
import os

import pytest

from opt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_KERNELS = ("gen_blk_init", "gen_blk_step2", "gen_blk_half2", "gen_blk_apply")


def energy(name):
    return os.path.join(ROOT, "energies", name + ".t")


def block_variant(tmp_path, name):
    text = open(energy(name)).read()
    if "UsePreconditioner(true)" in text:
        text = text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")')
    else:
        assert "UsePreconditioner" not in text
        text = text.replace("Exclude(", 'UsePreconditioner("block")\nExclude(', 1)
    assert text.count('UsePreconditioner("block")') == 1
    path = tmp_path / (name + "_block.t")
    path.write_text(text)
    return str(path)


def test_block_statement_keeps_the_residuals_and_marks_the_signature(tmp_path):
    shipped, blk = energy("bundle_adjustment"), block_variant(tmp_path, "bundle_adjustment")
    assert api.generic_describe(blk) == api.generic_describe(shipped)
    assert api.generic_signature(blk) == api.generic_signature(shipped) + "B;"


def test_any_other_argument_is_the_scalar_preconditioner(tmp_path):
    text = open(energy("bundle_adjustment")).read().replace("UsePreconditioner(true)", 'UsePreconditioner("jacobi")')
    path = tmp_path / "other.t"
    path.write_text(text)
    assert api.generic_signature(str(path)) == api.generic_signature(energy("bundle_adjustment"))
    assert "gen_blk_init" not in api.generic_source(str(path))


def test_a_family_file_with_block_runs_on_generated_kernels(tmp_path):
    assert api.problem_family(energy("arap_mesh_deformation")) == "arap_mesh_deformation"
    assert api.problem_family(block_variant(tmp_path, "arap_mesh_deformation")) == "generic"
    assert api.problem_family(block_variant(tmp_path, "arap_mesh_deformation"), "LMGPU") == "generic"


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("name", ["bundle_adjustment", "row_bias", "arap_mesh_deformation"])
def test_block_variants_compile_for_gfx950(tmp_path, name, double):
    """generic_compile_check compiles the 64-bit and, for graph energies, the 32-bit gather form."""
    blk = block_variant(tmp_path, name)
    api.generic_compile_check(blk, double)
    for off32 in (False, True):
        src, shipped = api.generic_source(blk, double, off32), api.generic_source(energy(name), double, off32)
        assert "a.gnb[" in src                                   # all three are graph energies
        for k in BLOCK_KERNELS:
            assert k in src and k not in shipped
        assert "T* __restrict__ blk" in src and "blk" not in shipped


def test_more_than_eight_channels_in_one_space_is_refused(tmp_path, capfd):
    path = tmp_path / "nine.t"
    path.write_text('local N = Dim("N", 0)\n'
                    'local A = Unknown("A", opt_float3, {N}, 0)\n'
                    'local B = Unknown("B", opt_float3, {N}, 1)\n'
                    'local C = Unknown("C", opt_float3, {N}, 2)\n'
                    'UsePreconditioner("block")\n'
                    'Energy(A(0) - B(0))\nEnergy(B(0) + C(0))\nEnergy(0.5 * C(0))\n')
    capfd.readouterr()
    with pytest.raises(api.OptError, match="Opt_ProblemDefine refused"):
        api.problem_family(str(path))
    err = capfd.readouterr().err
    assert "{N}" in err and "9" in err and "block" in err
    # the same file with the scalar preconditioner is accepted
    path.write_text(path.read_text().replace('"block"', "true"))
    assert api.problem_family(str(path)) == "generic"
