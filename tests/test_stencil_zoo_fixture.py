"""The stencil zoo's fixtures (tests/stencil_zoo.py) without a GPU: what the generator emits
for the four energies, that the inputs exercise what the GPU tests mean to exercise (every
residual alive and bbox-dropped somewhere, the exclusion within reach of active pixels), and
that the float64 reference would notice a lost term."""
import numpy as np
import pytest

from opt_amd import api
from tests import stencil_zoo as zoo

FP32_BAR = 2e-5   # tests/test_multispace_gpu.py tols(False)[0]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("name", sorted(zoo.ZOO))
def test_generator_emits_the_listed_forms(tmp_path, name, double):
    f = api.generic_forms(zoo.write_energy(tmp_path, name), double)
    (sa, sj, sc), (tx, ty) = zoo.EMITTED[(name, double)]
    assert f["has_tiled"] == 1 and (f["tiles_x"], f["tiles_y"]) == (tx, ty)
    assert f["has_strip"] == (sa is not None) and f["has_jtf_strip"] == (sj is not None)
    assert f["has_cost_strip"] == 1 and f["cost_strip_cols"] == sc
    if sa is not None:
        assert (f["strip_cols"], f["jtf_strip_cols"]) == (sa, sj)


def test_b_in_double_has_no_scatter_strips(tmp_path):
    f = api.generic_forms(zoo.write_energy(tmp_path, "B"), True)
    assert f["has_strip"] == 0 and f["has_jtf_strip"] == 0 and f["has_cost_strip"] == 1


def test_halo_from_offsets_is_the_listed_one():
    for name, z in zoo.ZOO.items():
        assert zoo.halo_from_offsets(name) == z["halo"]


@pytest.mark.parametrize("name", sorted(zoo.ZOO))
def test_every_residual_lives_and_is_dropped_somewhere(name):
    z = zoo.ZOO[name]
    for W, H in zoo.sizes(name):
        w = zoo.problem(name, W, H)
        act = w["active"]
        for t, spec in enumerate(z["terms"]):
            if not zoo.fits(name, W, H, t):
                continue
            centres, _, ok = zoo.image_term(W, H, spec["reads"], spec.get("bounds", False))
            assert act[centres].any(), (name, W, H, t)
            reach = any(o != (0, 0) for o in spec["reads"])
            if spec.get("bounds"):
                assert len(centres) == W * H and not all(m.all() for m in ok.values())
            elif reach:
                assert 0 < len(centres) < W * H, (name, W, H, t)       # alive, and bbox-dropped somewhere
        if z["exclude"] is None or not all(zoo.fits(name, W, H, t) for t in range(len(z["terms"]))):
            continue
        frac = 1.0 - act.mean()
        assert 0.10 <= frac <= 0.20, (name, W, H, frac)
        # an excluded pixel is read by a residual centred on (or reaching) an active one
        a2 = act.reshape(H, W)
        near = False
        for spec in z["terms"]:
            for dx, dy in spec["reads"]:
                if (dx, dy) == (0, 0):
                    continue
                src = a2[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]      # centres
                dst = a2[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]      # what they read
                near = near or bool((src & ~dst).any())
        assert near, (name, W, H)


def test_small_sizes_keep_only_the_fit_terms():
    for name, z in zoo.ZOO.items():
        for t, spec in enumerate(z["terms"]):
            alive = len(zoo.image_term(3, 2, spec["reads"], spec.get("bounds", False))[0]) > 0
            assert alive == (all(o == (0, 0) for o in spec["reads"]) or spec.get("bounds", False)), (name, t)


def reference_apply(w, drop=None):
    m, act, _ = zoo.model(w, drop)
    J = m.jacobian()
    p = np.random.default_rng(5).normal(size=m.n) * act
    return (J.T @ (J @ p)) * act


@pytest.mark.parametrize("name", sorted(zoo.ZOO))
def test_reference_apply_is_nonzero_and_notices_a_lost_term(name):
    sz = zoo.sizes(name)
    for W, H in sz:
        assert np.abs(reference_apply(zoo.problem(name, W, H))).max() > 0.1, (name, W, H)
    W, H = sz[4]
    w = zoo.problem(name, W, H)
    full = reference_apply(w)
    for t in range(len(zoo.ZOO[name]["terms"])):
        d = np.abs(reference_apply(w, drop=t) - full).max() / np.abs(full).max()
        assert d > 100 * FP32_BAR, (name, t, d)


def test_b_with_odd_pixel_count_puts_u_at_an_odd_offset():
    """V (3 channels) comes first: U's first element is 3 W H, odd for the (2S+1, 17) size, so
    the pair loads of U's windows of the solver vector are only 4-byte aligned there (the GPU
    test asserts the same of the plan's unknown_layout)."""
    W, H = zoo.sizes("B")[5]
    assert (3 * W * H) % 2 == 1
    m, act, _ = zoo.model(zoo.problem("B", W, H))
    assert m.off["U"] == 3 * W * H and len(act) == 5 * W * H


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("name", sorted(zoo.ZOO))
def test_generated_source_compiles_for_gfx950(tmp_path, name, double):
    """hiprtc without a device, as a plan compiles it. D in float chains lane shifts of two in
    its J^T F strip; with the shift helper's loops left to the optimizer's unroller that source
    crashed the compiler (a segmentation fault inside hiprtcCompileProgram, so a crash here, not
    an error, is what a regression looks like)."""
    path = zoo.write_energy(tmp_path, name)
    api.generic_compile_check(path, double)
    src = api.generic_source(path, double)
    assert '_Pragma("unroll") for (; d > 0; --d) v = opt_lr(v);' in src


def test_shifted_exclude_is_evaluated_by_the_whole_wave(tmp_path):
    """B's Exclude reads M at (-1, 0): in gen_jtf_strip the output's test takes its value from
    the lane to the left, which is switched off inside the branch on the output lanes (a DPP
    shift then reads 0), so the test stands before that branch."""
    src = api.generic_source(zoo.write_energy(tmp_path, "B"), False)
    k = src[src.index("void gen_jtf_strip("):src.index("void gen_cost_strip(")]
    assert k.index("act_o = act;") < k.index("if (xout && yo >= y0 && yo < y1)")
    tail = k[k.index("if (xout && yo >= y0 && yo < y1)"):]
    assert "opt_sh(" not in tail[:tail.index("a.flags")]
