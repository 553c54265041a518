"""GPU: the block-Jacobi preconditioner (UsePreconditioner("block")) on the generated kernels,
against float64 numpy on the AD oracle's J (oracle.examples_ad.Model; the models are built
here, after the pattern of tests/test_multispace_gpu.py).

M_e is the diagonal block of J^T J over all unknown channels of element e of an index space
(+ diag CtC_e in LM); PCG uses z = M_e^-1 r. Checked: the groups, z for a caller's r (GN and
LM forms, the pivot-rule fallback, excluded elements), whole GN / LM solves against numpy
loops in the order of stencil_plan.h, C = 1 against the scalar preconditioner, a centred
energy with off-diagonal entries, bitwise reproducibility, the materialized apply, and the
row-slab refusal.

Tolerances (tests/test_generic_gpu.py): per-unknown vectors within 2e-5 (fp32) / 1e-9 (fp64)
of the largest magnitude, scalars 1e-5 / 1e-9 relative, solves 1e-4 / 1e-8."""
import os

import numpy as np
import pytest

from opt_amd import OptSolver, api
from oracle import examples_ad as ad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(5, 131), (70, 9)]
SC_BASE, SC_SLOTS = 8, 7          # stencil_plan.h: rz_i sits at kScBase + kSlots * i


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def zeros(n, double):
    import torch
    return torch.zeros(n, device="cuda", dtype=torch.float64 if double else torch.float32)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def tols(double):
    return (1e-9, 1e-9, 1e-8) if double else (2e-5, 1e-5, 1e-4)


def eps_of(double):
    return float(np.finfo(np.float64 if double else np.float32).eps)


def rot(ang):
    a, b, g = ang[:, 0], ang[:, 1], ang[:, 2]
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    return np.stack([cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                     sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca,
                     -sb, cb * sa, cb * ca], -1).reshape(-1, 3, 3)


# ------------------------------------------------------------------ energy variants
@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """Energy files written for this module: shipped files with the statement replaced."""
    d = tmp_path_factory.mktemp("block_energies")
    out = {}
    ba = open(os.path.join(ROOT, "energies", "bundle_adjustment.t")).read()
    assert "UsePreconditioner(true)" in ba
    rb = open(os.path.join(ROOT, "energies", "row_bias.t")).read()
    assert "UsePreconditioner" not in rb
    for name, text in (("ba_block", ba.replace("UsePreconditioner(true)", 'UsePreconditioner("block")')),
                       ("ba_scalar", ba),
                       ("rb_block", rb.replace("Exclude(", 'UsePreconditioner("block")\nExclude(', 1)),
                       ("rb_true", rb.replace("Exclude(", "UsePreconditioner(true)\nExclude(", 1)),
                       ("rb_shipped", rb),
                       ("coupled", COUPLED)):
        p = d / (name + ".t")
        p.write_text(text)
        out[name] = str(p)
    return out


# ------------------------------------------------------------------ numpy restatements
def cholesky_passes(M, eps):
    """The pivot rule: every Cholesky pivot d_j = M_jj - sum_k L_jk^2 must exceed
    eps * C * max_i M_ii."""
    C = len(M)
    tol = eps * C * M.diagonal().max()
    L = np.zeros_like(M)
    for j in range(C):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not d > tol:
            return False
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return True


def block_inverse(JtJ, groups, scal, eps, add=None, active=None):
    """Dense M^-1 (n x n) and the fallback elements [(group, element)]. scal: the scalar
    preconditioner's values (the fallback's diagonal); add: CtC (LM); active: per unknown."""
    n = JtJ.shape[0]
    Minv = np.zeros((n, n))
    fallback = []
    for g, idx in enumerate(groups):
        for e, ix in enumerate(idx):
            if active is not None and not active[ix[0]]:
                continue
            M = JtJ[np.ix_(ix, ix)].copy()
            if add is not None:
                M += np.diag(add[ix])
            if cholesky_passes(M, eps):
                Minv[np.ix_(ix, ix)] = np.linalg.inv(M)
            else:
                Minv[ix, ix] = scal[ix]
                fallback.append((g, e))
    return Minv, fallback


def guarded_invert(d):
    return 1.0 / (1.0 + np.sqrt(d)) ** 2


class Problem:
    """A model with the reference's Exclude rule: cost over `cost_rows`, r / J^T J p / the
    update masked by `act` (per unknown), J with every row."""

    def __init__(self, model, groups, act=None, cost_rows=None):
        self.m, self.groups = model, groups
        self.act = np.ones(model.n) if act is None else np.asarray(act, np.float64)
        self.cost_rows = cost_rows

    def cost(self, F=None):
        F = self.m.residuals() if F is None else F
        F = F if self.cost_rows is None else F[self.cost_rows]
        return 0.5 * float(F @ F)

    def linearise(self):
        J = self.m.jacobian()
        F = self.m.residuals()
        JtJ = (J.T @ J).toarray()
        return J, F, JtJ, -(J.T @ F) * self.act, self.m.diag_access.copy()


def gn_solve_reference(P, steps, L, eps, block=True):
    """GN with PCG in the order of stencil_plan.h (alpha = rz / pAp, r, z, beta, p).
    Returns (costs after init and each step, rz history of the first step)."""
    x0 = P.m.get()
    costs, rz_first = [P.cost()], None
    for _ in range(steps):
        J, F, JtJ, r, diag = P.linearise()
        scal = P.act * guarded_invert(diag)
        Minv = block_inverse(JtJ, P.groups, scal, eps, active=P.act)[0] if block else np.diag(scal)
        delta = np.zeros(P.m.n)
        z = Minv @ r
        p = z.copy()
        rz = float(r @ z)
        hist = [rz]
        for _i in range(L):
            Ap = (JtJ @ p) * P.act
            alpha = rz / float(p @ Ap)
            delta += alpha * p
            r = r - alpha * Ap
            z = Minv @ r
            rz_new = float(z @ r)
            p = z + (rz_new / rz) * p
            rz = rz_new
            hist.append(rz)
        rz_first = rz_first or hist
        P.m.set(P.m.get() + delta * P.act)
        costs.append(P.cost())
    P.m.set(x0)
    return costs, rz_first


def lm_ctc(diag, radius, min_d=float(np.float32(1e-6)), max_d=float(np.float32(1e32))):
    """lm_init_kernel's first step: SSq = guarded_invert(diag), CtC = clamp(diag / radius,
    min_lm / (SSq radius), max_lm / (SSq radius)); the scalar preconditioner 1 / (CtC + diag)."""
    ssq = guarded_invert(diag)
    clampm = (1.0 / ssq) / radius
    c = np.clip(diag / radius, min_d * clampm, max_d * clampm)
    return ssq, c, 1.0 / (c + diag)


def lm_solve_reference(P, steps, L, eps):
    """LM as stencil_plan.h runs it (step + lm_finish_step) with the block M; returns the
    costs after init and after each step, and the accept (True) / reject sequence."""
    x0 = P.m.get()
    radius, decrease = 1e4, 2.0
    min_rel, fn_tol, q_tol, reset = 1e-3, float(np.float32(1e-6)), float(np.float32(1e-4)), 10
    prev = P.cost()
    costs, accepted, ssq = [prev], [], None
    for _ in range(steps):
        J, F, JtJ, r, diag = P.linearise()
        if ssq is None:
            ssq = guarded_invert(diag)
        clampm = (1.0 / ssq) / radius
        c = np.clip(diag / radius, float(np.float32(1e-6)) * clampm, float(np.float32(1e32)) * clampm) * P.act
        scal = P.act / np.where(P.act > 0, c + diag, 1.0)
        Minv = block_inverse(JtJ, P.groups, scal, eps, add=c, active=P.act)[0]
        A = lambda v: (JtJ @ v + c * v) * P.act
        b = r.copy()
        delta = np.zeros(P.m.n)
        z = Minv @ r
        p = z.copy()
        rz, Q0 = float(r @ z), 0.0
        for i in range(L):
            Ap = A(p)
            alpha = rz / float(p @ Ap)
            delta += alpha * p
            r = b - A(delta) if (i + 1) % reset == 0 else r - alpha * Ap
            z = Minv @ r
            rz_new = float(z @ r)
            q = 0.5 * float(delta @ (r + b))
            if (i + 1) * (q - Q0) / q < q_tol:
                break
            Q0 = q
            p = z + (rz_new / rz) * p
            rz = rz_new
        mc = F + J @ delta
        mc = mc if P.cost_rows is None else mc[P.cost_rows]
        model_cost = 0.5 * float(mc @ mc)
        saved = P.m.get()
        P.m.set(saved + delta * P.act)
        new = P.cost()
        cost_change, rel = prev - new, (prev - new) / (prev - model_cost)
        if cost_change >= 0 and rel > min_rel:
            if cost_change <= prev * fn_tol:
                break
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3), 1e16)
            decrease, prev = 2.0, new
            accepted.append(True)
        else:
            P.m.set(saved)
            radius, decrease = radius / decrease, 2.0 * decrease
            accepted.append(False)
        costs.append(prev)
    P.m.set(x0)
    return costs, accepted


# ------------------------------------------------------------------ bundle adjustment
_BUNDLE = {}


def bundle(NC, NP):
    """Inputs (rounded to fp32): camera 0 sees every point, the last camera none, point
    NP - 1 is seen once."""
    if (NC, NP) in _BUNDLE:
        return _BUNDLE[(NC, NP)]
    rng = np.random.default_rng(1000 * NC + NP)
    X = rng.uniform(-1, 1, (NP, 3))
    R = rng.normal(0, 0.15, (NC, 3))
    T = np.array([0, 0, 5.0]) + rng.normal(0, 0.3, (NC, 3))
    cam, pt = [np.zeros(NP, np.int64)], [np.arange(NP)]
    for c in range(1, NC - 1):
        k = max(3, NP // 3)
        cam.append(np.full(k, c))
        pt.append(rng.choice(NP - 1, k, replace=False))
    cam, pt = np.concatenate(cam), np.concatenate(pt)
    order = rng.permutation(len(cam))
    cam, pt = cam[order].astype(np.int32), pt[order].astype(np.int32)
    NO = len(cam)
    q = np.einsum("nij,nj->ni", rot(R)[cam], X[pt]) + T[cam]
    obs_slot = rng.permutation(NO).astype(np.int32)
    Obs = np.zeros((NO, 2))
    Obs[obs_slot] = q[:, :2] / q[:, 2:3] + rng.normal(0, 1e-3, (NO, 2))
    w = dict(NC=NC, NP=NP, NO=NO, c=cam, p=pt, o=obs_slot, Obs=f32(Obs), w_cam=0.1, w_pt=0.1,
             CamR=f32(R + rng.normal(0, 0.02, R.shape)), CamT=f32(T + rng.normal(0, 0.05, T.shape)),
             X=f32(X + rng.normal(0, 0.05, X.shape)))
    _BUNDLE[(NC, NP)] = w
    return w


def bundle_model(w):
    import torch
    m = ad.Model([("CamR", w["CamR"]), ("CamT", w["CamT"]), ("X", w["X"])],
                 {"CamR0": w["CamR"], "CamT0": w["CamT"], "X0": w["X"], "Obs": w["Obs"]})
    wc, wp = float(np.float32(w["w_cam"])), float(np.float32(w["w_pt"]))
    ic, ip = np.arange(w["NC"]), np.arange(w["NP"])
    m.term(lambda r, r0: wc * (r - r0), [("u", "CamR", ic), ("c", "CamR0", ic)], 3)
    m.term(lambda t, t0: wc * (t - t0), [("u", "CamT", ic), ("c", "CamT0", ic)], 3)
    m.term(lambda x, x0: wp * (x - x0), [("u", "X", ip), ("c", "X0", ip)], 3)

    def reproject(r, t, x, ob):
        q = ad._rotate3d(r, x) + t
        return torch.stack([q[0] / q[2] - ob[0], q[1] / q[2] - ob[1]])

    m.term(reproject, [("u", "CamR", w["c"]), ("u", "CamT", w["c"]), ("u", "X", w["p"]), ("c", "Obs", w["o"])], 2)
    return m


def bundle_groups(w):
    """Unknown indices of every element's block: cameras CamR | CamT (C = 6), points (C = 3)."""
    NC, NP = w["NC"], w["NP"]
    e, c3 = np.arange(NC)[:, None], np.arange(3)[None, :]
    cams = np.concatenate([3 * e + c3, 3 * NC + 3 * e + c3], 1)
    pts = 6 * NC + 3 * np.arange(NP)[:, None] + c3
    return [cams, pts]


def bundle_params(w, double):
    T = np.float64 if double else np.float32
    unk = [cuda(w[k].astype(T)) for k in ("CamR", "CamT", "X")]
    prm = [w["w_cam"], w["w_pt"]] + unk + [cuda(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
    return prm, unk


def bundle_solver(w, path, kind="gaussNewtonGPU", double=False, **kw):
    return OptSolver([w["NC"], w["NP"], w["NO"]], path, kind, double_precision=double, **kw)


_LIN = {}


def bundle_linearised(key, w):
    """(J^T J dense, diag) of the bundle model at its start, once per problem."""
    if key not in _LIN:
        P = Problem(bundle_model(w), bundle_groups(w))
        _, _, JtJ, _, diag = P.linearise()
        _LIN[key] = (JtJ, diag)
    return _LIN[key]


def check_z(s, prm, Minv, double, seed, note=""):
    """apply_preconditioner for a random r against Minv r; returns (r, z)."""
    n = s.unknown_count()
    r = np.random.default_rng(seed).normal(size=n).astype(np.float64 if double else np.float32)
    z = zeros(n, double)
    s.apply_preconditioner(prm, cuda(r), z)
    z = z.cpu().numpy()
    ref = Minv @ r.astype(np.float64)
    print(note, "z", rel_err(z, ref), "bound", tols(double)[0])
    assert rel_err(z, ref) < tols(double)[0]
    return r, z


@pytest.mark.parametrize("NC,NP", SIZES)
def test_groups_of_the_bundle_energy(variants, NC, NP):
    w = bundle(NC, NP)
    s = bundle_solver(w, variants["ba_block"])
    assert s.family() == "generic"
    assert s.preconditioner_blocks() == ([0, 0, 1], [0, 3, 0], 2)
    assert bundle_solver(w, variants["ba_scalar"]).preconditioner_blocks() == ([], [], 0)
    assert s.lib.OptAMD_PlanPreconditionerBlocks(None, 4, None, None) == -1


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_gn_form_applies_the_inverse_blocks(variants, NC, NP, double):
    w = bundle(NC, NP)
    JtJ, diag = bundle_linearised(("ba", NC, NP), w)
    Minv, fallback = block_inverse(JtJ, bundle_groups(w), guarded_invert(diag), eps_of(double))
    assert not fallback
    s = bundle_solver(w, variants["ba_block"], double=double)
    prm, _ = bundle_params(w, double)
    check_z(s, prm, Minv, double, seed=NC)


def test_scalar_plan_applies_pre(variants):
    w = bundle(5, 131)
    _, diag = bundle_linearised(("ba", 5, 131), w)
    s = bundle_solver(w, variants["ba_scalar"], double=True)
    prm, _ = bundle_params(w, True)
    check_z(s, prm, np.diag(guarded_invert(diag)), True, seed=3)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("zeroed,n_singular", [("w_pt", 40), ("w_cam", 1)])
def test_singular_blocks_fall_back_to_the_scalar_preconditioner(variants, zeroed, n_singular, double):
    w = dict(bundle(5, 131))
    w[zeroed] = 0.0
    JtJ, diag = bundle_linearised(("ba", 5, 131, zeroed), w)
    scal = guarded_invert(diag)
    groups = bundle_groups(w)
    # (the float64 reference of the issue: 40 point blocks / the last camera's block)
    _, fb64 = block_inverse(JtJ, groups, scal, eps_of(True))
    assert len(fb64) == n_singular
    assert all(g == 1 for g, _ in fb64) if zeroed == "w_pt" else fb64 == [(0, 4)]
    Minv, fallback = block_inverse(JtJ, groups, scal, eps_of(double))
    print("fallback elements", len(fallback))
    s = bundle_solver(w, variants["ba_block"], double=double)
    prm, _ = bundle_params(w, double)
    r, z = check_z(s, prm, Minv, double, seed=11, note=zeroed)
    fb = np.concatenate([groups[g][e] for g, e in fallback])
    ref = scal[fb] * r[fb].astype(np.float64)
    print("fallback z", np.abs(z[fb] - ref).max() / np.abs(ref).max())
    assert np.abs(z[fb] - ref).max() <= tols(double)[0] * np.abs(ref).max()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_lm_form_adds_the_clamped_diagonal(variants, NC, NP, double):
    w = bundle(NC, NP)
    JtJ, diag = bundle_linearised(("ba", NC, NP), w)
    _, c, scal = lm_ctc(diag, 1e4)
    Minv, fallback = block_inverse(JtJ, bundle_groups(w), scal, eps_of(double), add=c)
    assert not fallback
    s = bundle_solver(w, variants["ba_block"], "LMGPU", double)
    prm, _ = bundle_params(w, double)
    check_z(s, prm, Minv, double, seed=NP)


_GN = {}


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_gn_solve_matches_numpy_pcg(variants, NC, NP, double):
    w = bundle(NC, NP)
    if (NC, NP) not in _GN:
        P = Problem(bundle_model(w), bundle_groups(w))
        _GN[(NC, NP)] = (gn_solve_reference(P, 3, 10, eps_of(True)), gn_solve_reference(P, 1, 10, eps_of(True), block=False))
    (ref_costs, ref_rz), (_, scalar_rz) = _GN[(NC, NP)]
    s = bundle_solver(w, variants["ba_block"], double=double)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, _ = bundle_params(w, double)
    s.init(prm)
    costs = [s.cost()]
    assert s.step()
    costs.append(s.cost())
    sc = s.scalars()
    rz = [sc[SC_BASE + SC_SLOTS * i] for i in range(11)]
    while s.step():
        costs.append(s.cost())
    print("costs", costs, "numpy", ref_costs)
    for i in range(11):
        print(f"rz[{i}] block {rz[i]:.6e} numpy {ref_rz[i]:.6e} rel {abs(rz[i] - ref_rz[i]) / ref_rz[i]:.2e}"
              f"   scalar preconditioner (numpy) {scalar_rz[i]:.6e}")
    assert len(costs) == 4
    np.testing.assert_allclose(costs, ref_costs, rtol=tols(double)[2])
    np.testing.assert_allclose(rz, ref_rz, rtol=tols(double)[1])


_LM = {}


@pytest.mark.parametrize("double", [True, False])
def test_lm_solve_matches_numpy_restatement(variants, double):
    w = bundle(5, 131)
    if "ba" not in _LM:
        _LM["ba"] = lm_solve_reference(Problem(bundle_model(w), bundle_groups(w)), 3, 10, eps_of(True))
    ref_costs, accepted = _LM["ba"]
    s = bundle_solver(w, variants["ba_block"], "LMGPU", double)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, _ = bundle_params(w, double)
    costs = s.profiled_solve(prm)
    print("costs", costs, "numpy", ref_costs, "accepted", accepted)
    assert len(costs) == len(ref_costs)
    got = [b < a for a, b in zip(costs, costs[1:])]
    assert got == accepted
    np.testing.assert_allclose(costs, ref_costs, rtol=tols(double)[2])


def test_block_lm_solves_are_bitwise_reproducible(variants):
    w = bundle(5, 131)
    out = []
    for _ in range(2):
        s = bundle_solver(w, variants["ba_block"], "LMGPU")
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = bundle_params(w, False)
        costs = s.profiled_solve(prm)
        out.append((np.array(costs), [u.cpu().numpy() for u in unk]))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    for a, b in zip(out[0][1], out[1][1]):
        assert a.tobytes() == b.tobytes()
    assert out[0][0][-1] < out[0][0][0]


# ---------------------------------------------------------------------------- row bias
def row_bias(W, H):
    rng = np.random.default_rng(100 * W + H)
    n = W * H
    yy, xx = np.mgrid[0:H, 0:W]
    truth = np.sin(0.3 * xx) + 0.1 * yy
    bias = rng.normal(0, 0.3, H)
    px = np.flatnonzero(rng.random(n) >= 0.10).astype(np.int32)   # an edge per pixel except 10 %
    px = px[rng.permutation(len(px))]
    return dict(W=W, H=H, E=len(px), px=px, row=(px // W).astype(np.int32), w_s=0.5, w_b=0.05,
                D=f32(truth + bias[:, None] + rng.normal(0, 0.02, (H, W))), Mask=f32(rng.random((H, W)) < 0.15),
                I=f32(truth + rng.normal(0, 0.05, (H, W))), B=f32(rng.normal(0, 0.05, H)))


def row_bias_params(w, double):
    T = np.float64 if double else np.float32
    unk = [cuda(w["I"].astype(T)), cuda(w["B"].astype(T))]
    return [w["w_s"], w["w_b"]] + unk + [cuda(w[k]) for k in ("D", "Mask", "px", "row")], unk


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("W,H", [(9, 7), (70, 5)])
def test_one_channel_blocks_equal_the_scalar_lm_preconditioner(variants, W, H, double):
    """Both groups have C = 1: M_e = B_e + CtC_e = d + c, today's 1 / (c + d). The scalar plan
    compared is the file with UsePreconditioner(true): the shipped row_bias.t has no statement,
    so its PCG runs unpreconditioned (z = r) and is another iteration altogether; its costs
    are printed beside the others."""
    w = row_bias(W, H)
    costs = {}
    for name in ("rb_block", "rb_true", "rb_shipped"):
        s = OptSolver([W, H, w["E"]], variants[name], "LMGPU", double_precision=double)
        assert s.family() == "generic"
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, _ = row_bias_params(w, double)
        costs[name] = s.profiled_solve(prm)
        if name == "rb_block":
            assert s.preconditioner_blocks() == ([0, 1], [0, 0], 2)
            n = s.unknown_count()
            z = zeros(n, double)
            prm2, _ = row_bias_params(w, double)
            s.apply_preconditioner(prm2, cuda(np.ones(n, np.float64 if double else np.float32)), z)
            z = z.cpu().numpy()
            masked = np.concatenate([w["Mask"].reshape(-1) == 1, np.zeros(H, bool)])
            assert masked.any() and not z[masked].any() and np.all(z[~masked] > 0)
    print(costs)
    assert len(costs["rb_block"]) == len(costs["rb_true"])
    np.testing.assert_allclose(costs["rb_block"], costs["rb_true"], rtol=tols(double)[1])


# ------------------------------------------ a centred energy with off-diagonal block entries
COUPLED = """
local W, H = Dim("W", 0), Dim("H", 1)
local P = Unknown("P", opt_float2, {W, H}, 0)
local S = Unknown("S", opt_float, {W, H}, 1)
local A = Array("A", opt_float2, {W, H}, 2)
local M = Array("M", opt_float, {W, H}, 3)
UsePreconditioner("block")
Exclude(eq(M(0, 0), 1))
Energy(P(0, 0)(0) * S(0, 0) + P(0, 0)(1) - A(0, 0)(0))
Energy(Select(InBounds(1, 0), 0.2 * (S(0, 0) * P(1, 0)(0) - P(0, 0)(1) * S(1, 0)), 0))
Energy(Select(InBounds(0, 1), P(0, 0)(0) * P(0, 1)(1) - S(0, 1) - A(0, 0)(1), 0))
Energy(0.3 * (S(0, 0) - 1))
"""
_COUPLED = {}


def coupled(W, H):
    if (W, H) in _COUPLED:
        return _COUPLED[(W, H)]
    rng = np.random.default_rng(7 * W + H)
    n = W * H
    # A is consistent with a "true" (P, S) up to noise; the start is that truth, perturbed
    Pt, St = rng.normal(0.8, 0.2, (n, 2)), rng.normal(1.0, 0.1, (n, 1))
    down = np.minimum(np.arange(n) + W, n - 1)
    A = np.stack([Pt[:, 0] * St[:, 0] + Pt[:, 1], Pt[:, 0] * Pt[down, 1] - St[down, 0]], 1)
    w = dict(W=W, H=H, P=f32(Pt + rng.normal(0, 0.03, Pt.shape)), S=f32(St + rng.normal(0, 0.03, St.shape)),
             A=f32(A + rng.normal(0, 0.01, A.shape)), M=f32(rng.random(n) < 0.2))
    _COUPLED[(W, H)] = w
    return w


def coupled_problem(w):
    W, H = w["W"], w["H"]
    n = W * H
    m = ad.Model([("P", w["P"]), ("S", w["S"])], {"A": w["A"]})
    yy, xx = np.mgrid[0:H, 0:W]
    i = (xx + W * yy).reshape(-1)
    masked = w["M"] == 1
    keep = [~masked[i]]
    m.term(lambda p, s, a: (p[0] * s[0] + p[1] - a[0]).reshape(1), [("u", "P", i), ("u", "S", i), ("c", "A", i)], 1)
    ok = (xx + 1 < W).reshape(-1)
    m.term(lambda s, p, pr, sr: (0.2 * (s[0] * pr[0] - p[1] * sr[0])).reshape(1),
           [("u", "S", i[ok]), ("u", "P", i[ok]), ("u", "P", i[ok] + 1), ("u", "S", i[ok] + 1)], 1)
    keep.append(~masked[i[ok]])
    ok = (yy + 1 < H).reshape(-1)
    m.term(lambda p, pd, sd, a: (p[0] * pd[1] - sd[0] - a[1]).reshape(1),
           [("u", "P", i[ok]), ("u", "P", i[ok] + W), ("u", "S", i[ok] + W), ("c", "A", i[ok])], 1)
    keep.append(~masked[i[ok]])
    m.term(lambda s: 0.3 * (s - 1.0), [("u", "S", i)], 1)
    keep.append(~masked[i])
    e = np.arange(n)[:, None]
    groups = [np.concatenate([2 * e, 2 * e + 1, 2 * n + e], 1)]
    act = np.concatenate([np.repeat(~masked, 2), ~masked]).astype(np.float64)
    return Problem(m, groups, act, np.concatenate(keep))


def coupled_params(w, double):
    T = np.float64 if double else np.float32
    unk = [cuda(w["P"].astype(T)), cuda(w["S"].astype(T))]
    return unk + [cuda(w["A"]), cuda(w["M"])], unk


_CREF = {}


def coupled_reference(W, H):
    if (W, H) not in _CREF:
        P = coupled_problem(coupled(W, H))
        _, _, JtJ, _, diag = P.linearise()
        Minv, fallback = block_inverse(JtJ, P.groups, P.act * guarded_invert(diag), eps_of(True), active=P.act)
        _CREF[(W, H)] = (Minv, fallback, gn_solve_reference(P, 3, 10, eps_of(True))[0], P.act)
    return _CREF[(W, H)]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("W,H", [(5, 4), (67, 3)])
def test_centred_energy_with_off_diagonal_entries(variants, W, H, double):
    w = coupled(W, H)
    Minv, fallback, ref_costs, act = coupled_reference(W, H)
    assert not fallback and (act == 0).any()
    off = Minv - np.diag(Minv.diagonal())
    assert np.abs(off).max() > 1e-3 * np.abs(Minv).max()            # the blocks are not diagonal
    s = OptSolver([W, H], variants["coupled"], double_precision=double)
    assert s.family() == "generic" and s.preconditioner_blocks() == ([0, 0], [0, 2], 1)
    prm, _ = coupled_params(w, double)
    _, z = check_z(s, prm, Minv, double, seed=W)
    assert not z[act == 0].any()
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, _ = coupled_params(w, double)
    costs = s.profiled_solve(prm)
    print("costs", costs, "numpy", ref_costs)
    assert len(costs) == 4
    np.testing.assert_allclose(costs, ref_costs, rtol=tols(double)[2])


@pytest.mark.parametrize("double", [False, True])
def test_materialized_apply_gives_the_matrix_free_costs(variants, double):
    w = coupled(67, 3)
    costs = []
    for kw in ({}, {"materialized": True}):
        s = OptSolver([67, 3], variants["coupled"], double_precision=double, **kw)
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, _ = coupled_params(w, double)
        costs.append(s.profiled_solve(prm))
    assert costs[1] and s.materialized_nonzeros() is not None
    print(costs)
    np.testing.assert_allclose(costs[1], costs[0], rtol=tols(double)[2])


def test_row_slabs_are_refused_by_name(variants, capfd):
    s = OptSolver([67, 3], variants["coupled"])
    capfd.readouterr()
    group = s.lib.OptAMD_LocalGroupCreate(2)
    with pytest.raises(api.OptError, match="OptAMD_PlanSetDecomposition failed"):
        s.set_decomposition(s.lib.OptAMD_LocalGroupRank(group, 0), 0, 2)
    s.lib.OptAMD_LocalGroupDestroy(group)
    assert "block preconditioner" in capfd.readouterr().err
