"""GPU: the launch schedule of one Step of the generic driver (stencil_plan.h: linear_init,
pcg_loop / pcg_loop_fused and their stages), per plan kind: how many launches of each timed
name one Step enqueues. With kernel timing on the plan launches eagerly and every bracket
counts once (OptAMD_KernelStat), and the loop enqueues every iteration whatever the
device-side exit decides, so the counts depend on the plan kind, lIterations and
residual_reset_period alone, not on the data.

L = lIterations = 7 and P = residual_reset_period = 3: LM's R = L // P = 2 residual-reset
iterations (i = 2 and i = 5) replace step2 by half1 / an untimed apply of delta / half2.
A is the plan's apply_kernel_name(). cost, precompute, update and halo_exchange are left
out: an LM revert changes them."""
import os

import pytest

from opt_amd import OptSolver, workloads
from tests import test_arap_gpu as arap
from tests import test_pose_graph_gpu as pg
from tests import test_schur_gpu as ba
from tests import test_sfs_gpu as sfs
from tests.iw_helpers import ROOT

pytestmark = pytest.mark.gpu
L, P = 7, 3
R = L // P
POISSON = os.path.join(ROOT, "energies", "poisson_image_editing.t")
EXPLICIT = os.path.join(ROOT, "energies", "bundle_adjustment_schur_explicit.t")
NORMAL = os.path.join(ROOT, "energies", "normal_matrix", "pose_graph_2d_explicit.t")
GN, LM = "gaussNewtonGPU", "LMGPU"
# every name some case counts: a case expects 0 of the ones it does not list
NAMES = ["jtf", "gn_init", "lm_init", "step2", "step3", "step23", "blk_init", "blk_step2", "blk_half2",
         "schur_rhs", "schur_elim", "schur_apply", "schur_back", "schur_eblk", "schur_assemble", "schur_spmv",
         "schur_symbolic", "normal_symbolic", "normal_eblk", "normal_assemble", "normal_spmv", "saveJToCRS", "gen_apply"]


def poisson(kind, tmp_path=None, **kw):
    import torch
    w = workloads.poisson_image_editing(96, 80, seed=4)
    return OptSolver([96, 80], POISSON, kind, **kw), [torch.from_numpy(w[k].copy()).cuda() for k in ("X", "T", "M")]


def shading(kind, tmp_path=None):
    W, H = 97, 61
    return OptSolver([W, H], sfs.ENERGY, kind), sfs.params(sfs.synthetic(W, H, seed=2 * W + H))


def mesh(kind, tmp_path=None):
    w = arap.perturbed(7, 5, seed=12)
    return arap.solver(w, kind), arap.params(w)


def bundle(path, block=False):
    """block: bundle_adjustment.t with UsePreconditioner("block") in place of its scalar one"""
    def make(kind, tmp_path):
        w = ba.bundle(5, 131)
        energy = path
        if block:
            energy = tmp_path / "ba_block.t"
            energy.write_text(open(path).read().replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
        return ba.solver(w, kind, path=str(energy)), ba.bundle_params(w, False)[0]
    return make


def poses(kind, tmp_path=None):
    w = pg.arrays(40)
    return pg.solver(w, kind, energy=NORMAL), pg.params(w, False)[0]


def common(lm):
    return {"jtf": 1, "lm_init" if lm else "gn_init": 1, "step3": L}


def classic(lm):
    """apply / step2 / step3; LM's reset iterations have no step2 and their apply of delta is untimed"""
    return {**common(lm), "A": L, "step2": L - R if lm else L}


def fused(lm):
    """apply + step23; LM's reset iterations are the classic halves and step3"""
    return {"jtf": 1, "lm_init" if lm else "gn_init": 1, "A": L, "step23": L - R if lm else L,
            "step3": R if lm else 0}


def block(lm):
    return {**common(lm), "A": L, "blk_init": 1, "blk_step2": L - R if lm else L, "blk_half2": R if lm else 0}


def schur(lm):
    """every apply, the reset's included, is schur_elim + schur_apply (the one of the reduced
    right-hand side rides in schur_rhs's bracket)"""
    n = L + R if lm else L
    d = block(lm)
    del d["A"]
    return {**d, "schur_rhs": 1, "schur_elim": n, "schur_apply": n, "schur_back": 1}


def schur_explicit(lm, first=True):
    """S assembled once per Step, every apply one block SpMV; the pattern of S once per wiring"""
    d = schur(lm)
    d.update({"schur_elim": 0, "schur_apply": 0, "schur_eblk": 1, "schur_assemble": 1,
              "schur_spmv": L + R if lm else L, "schur_symbolic": 1 if first else 0})
    return d


def normal_explicit(lm, first=True):
    """H assembled once per Step, every apply (the reset's included) one block SpMV; the pattern
    of H once per wiring"""
    d = block(lm)
    del d["A"]
    return {**d, "normal_eblk": 1, "normal_assemble": 1, "normal_spmv": L + R if lm else L,
            "normal_symbolic": 1 if first else 0, "gen_apply": 0}


def materialized(lm):
    """J assembled once per Step; the loop's applies are the SpMV pair (A = its second), the
    family's own apply only the reset's untimed one"""
    return {**classic(lm), "saveJToCRS": 1, "plain": 0}


CASES = {
    "poisson-GN": (poisson, GN, {}, classic),
    "poisson-LM": (poisson, LM, {}, classic),
    "sfs-LM-fused": (shading, LM, {"OPT_AMD_FUSE23": "1"}, fused),
    "sfs-LM-classic": (shading, LM, {"OPT_AMD_FUSE23": "0"}, classic),
    # ARAP's step3_fused runs under step3's bracket, apply_prepared under the apply's
    "arap-GN-fuse3": (mesh, GN, {}, classic),
    "arap-GN-plain": (mesh, GN, {"OPT_AMD_FUSE_STEP3": "0"}, classic),
    "block-GN": (bundle(ba.BA, block=True), GN, {}, block),
    "block-LM": (bundle(ba.BA, block=True), LM, {}, block),
    "schur-GN": (bundle(ba.SCHUR), GN, {}, schur),
    "schur-LM": (bundle(ba.SCHUR), LM, {}, schur),
    "explicit-GN": (bundle(EXPLICIT), GN, {}, schur_explicit),
    "explicit-LM": (bundle(EXPLICIT), LM, {}, schur_explicit),
    "normal-GN": (poses, GN, {}, normal_explicit),
    "normal-LM": (poses, LM, {}, normal_explicit),
    "materialized-LM": (lambda kind, tmp_path: poisson(kind, materialized=True), LM, {}, materialized),
}


def counts(s, names):
    return {n: s.kernel_stat(n)[0] for n in names}


def step_counts(s, names):
    before = counts(s, names)
    s.step()
    after = counts(s, names)
    return {n: after[n] - before[n] for n in names}


@pytest.mark.parametrize("case", list(CASES))
def test_launches_of_one_step(monkeypatch, tmp_path, case):
    make, kind, env, expected = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, prm = make(kind, tmp_path)
    s.set_solver_params({"nIterations": 3, "lIterations": L, "residual_reset_period": P})
    s.set_kernel_timing(1)
    A = s.apply_kernel_name()
    plain = poisson(kind)[0].apply_kernel_name() if expected is materialized else A
    names = NAMES + [n for n in (A, plain) if n not in NAMES]
    s.init(prm)
    steps = [step_counts(s, names)]
    if expected in (schur_explicit, normal_explicit):
        steps.append(step_counts(s, names))   # the same graphs: no second symbolic phase
    for k, got in enumerate(steps):
        want = expected(kind == LM) if k == 0 else expected(kind == LM, first=False)
        want = {A if n == "A" else plain if n == "plain" else n: c for n, c in want.items()}
        want = {n: want.get(n, 0) for n in names}
        print(case, "step", k, {n: c for n, c in got.items() if c or want[n]})
        assert got == want
    s.close()
