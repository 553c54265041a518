"""GPU: energies over several index spaces on the generated kernels, against the float64
AD oracle (oracle.examples_ad.Model / solve; the models are built here).

bundle_adjustment.t: cameras {NC}, points {NP}, observations {NO}; row_bias.t: an image
{W,H} with a per-row unknown {H} and an Exclude on the image's space. Per kernel (cost,
J^T F with the preconditioner, J^T J p) against the oracle's J; whole GN / LM solves; bitwise
determinism; backend_cpu == backend_cuda; the unknown layout; the host-side slot range check;
the refusals (row slabs, materialized J^T J, Jacobian assembly).

Tolerances (tests/test_generic_gpu.py): fp32 per-unknown outputs within 2e-5 of the largest
magnitude, scalars within 1e-5 relative, solves within 1e-4; fp64 1e-9 / 1e-8.

The reference evaluates cost and model cost only at centres that are not excluded
(computeCost, solverGPUGaussNewton.t:974) while J^T F and J^T J p gather every residual
instance that contains an active unknown (createjtfcentered, o.t:2870-2913), so row_bias's
oracle model keeps the centred rows of excluded pixels
for J and drops them from the cost. examples_ad.solve has no such rule (its `active` masks
only the preconditioner), so for row_bias this file deviates from "the oracle used
unchanged": it keeps examples_ad.Model and the C loop behind examples_ad.solve, and drives
that loop through solve_with_excluded_centres below, which states the rule explicitly."""
import os

import numpy as np
import pytest

from opt_amd import OptSolver, api
from oracle import examples_ad as ad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = os.path.join(ROOT, "energies", "bundle_adjustment.t")
RB = os.path.join(ROOT, "energies", "row_bias.t")
SIZES = [(5, 131), (70, 9)]


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


def rot(ang):
    """L.Rotate3D's matrix (lib.t:84-97) for an (n, 3) array of angles -> (n, 3, 3)."""
    a, b, g = ang[:, 0], ang[:, 1], ang[:, 2]
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    return np.stack([cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                     sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca,
                     -sb, cb * sa, cb * ca], -1).reshape(-1, 3, 3)


# ------------------------------------------------------------------ bundle adjustment
_BUNDLE = {}


def bundle(NC, NP):
    """Inputs (all rounded to fp32) of the bundle problem; built once per size."""
    if (NC, NP) in _BUNDLE:
        return _BUNDLE[(NC, NP)]
    rng = np.random.default_rng(1000 * NC + NP)
    X = rng.uniform(-1, 1, (NP, 3))
    R = rng.normal(0, 0.15, (NC, 3))
    T = np.array([0, 0, 5.0]) + rng.normal(0, 0.3, (NC, 3))
    cam, pt = [np.zeros(NP, np.int64)], [np.arange(NP)]          # camera 0 sees every point
    for c in range(1, NC - 1):                                   # the last camera sees none
        k = max(3, NP // 3)
        cam.append(np.full(k, c))
        pt.append(rng.choice(NP - 1, k, replace=False))          # point NP-1: seen once
    cam, pt = np.concatenate(cam), np.concatenate(pt)
    order = rng.permutation(len(cam))
    cam, pt = cam[order].astype(np.int32), pt[order].astype(np.int32)
    NO = len(cam)
    q = np.einsum("nij,nj->ni", rot(R)[cam], X[pt]) + T[cam]
    obs_slot = rng.permutation(NO).astype(np.int32)               # Obs in an order of its own
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


def bundle_params(w, double, host=False):
    T = np.float64 if double else np.float32
    put = (lambda a: np.ascontiguousarray(a)) if host else cuda
    unk = [put(w[k].astype(T)) for k in ("CamR", "CamT", "X")]
    prm = [w["w_cam"], w["w_pt"]] + unk + [put(w[k]) for k in ("CamR", "CamT", "X", "Obs", "c", "p", "o")]
    return prm, unk


def bundle_solver(w, kind="gaussNewtonGPU", double=False, **kw):
    return OptSolver([w["NC"], w["NP"], w["NO"]], BA, kind, double_precision=double, **kw)


_REF = {}


def kernel_reference(key, model, active=None, use_pre=True, cost_rows=None):
    """(cost, r, pre, r.pre.r, J) of the oracle model, computed once per problem. Without
    UsePreconditioner(true) the reference forces the preconditioner of a unit diagonal
    (PCGInit1, solverGPUGaussNewton.t:541-547)."""
    if key not in _REF:
        J = model.jacobian()
        F = model.residuals()
        Fc = F if cost_rows is None else F[cost_rows]
        act = np.ones(model.n) if active is None else np.asarray(active, np.float64)
        r = -(J.T @ F) * act
        pre = act / (1.0 + np.sqrt(model.diag_access if use_pre else np.ones(model.n))) ** 2
        _REF[key] = (0.5 * float(Fc @ Fc), r, pre, float(r @ (pre * r)), J, act)
    return _REF[key]


def check_kernels(s, prm, ref, double, seed):
    cost, r_ref, pre_ref, rz_ref, J, act = ref
    vec, sca, _ = tols(double)
    n = s.unknown_count()
    assert n == len(r_ref)
    c = s.eval_cost(prm)
    print("cost", c, cost)
    r, pre = zeros(n, double), zeros(n, double)
    rz = s.eval_jtf(prm, r, pre)
    r, pre = r.cpu().numpy(), pre.cpu().numpy()
    print("r", rel_err(r, r_ref), "pre", rel_err(pre, pre_ref), "rz", rz, rz_ref)
    p = np.random.default_rng(seed).normal(size=n).astype(np.float64 if double else np.float32)
    Ap = zeros(n, double)
    pAp = s.apply_jtj(prm, cuda(p), Ap)
    Ap = Ap.cpu().numpy()
    Ap_ref = (J.T @ (J @ p.astype(np.float64))) * act
    pAp_ref = float(p.astype(np.float64) @ Ap_ref)
    print("Ap", rel_err(Ap, Ap_ref), "pAp", pAp, pAp_ref)
    assert c == pytest.approx(cost, rel=sca)
    assert rel_err(r, r_ref) < vec and rel_err(pre, pre_ref) < vec
    assert rz == pytest.approx(rz_ref, rel=sca)
    assert rel_err(Ap, Ap_ref) < vec
    assert pAp == pytest.approx(pAp_ref, rel=sca)
    return r, pre, Ap


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_bundle_kernels_match_oracle(NC, NP, double):
    w = bundle(NC, NP)
    s = bundle_solver(w, double=double)
    assert s.family() == "generic"
    prm, _ = bundle_params(w, double)
    check_kernels(s, prm, kernel_reference(("ba", NC, NP), bundle_model(w)), double, seed=NC)


_SOLVE = {}


def oracle_costs(key, build, lm):
    if key not in _SOLVE:
        _SOLVE[key] = ad.solve(build(), 3, 10, lm=lm)
    return _SOLVE[key]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("NC,NP", SIZES)
def test_bundle_solve_matches_oracle(NC, NP, kind, double):
    w = bundle(NC, NP)
    s = bundle_solver(w, kind, double)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, _ = bundle_params(w, double)
    costs = s.profiled_solve(prm)
    ref = oracle_costs(("ba", NC, NP, kind), lambda: bundle_model(w), kind == "LMGPU")
    print("costs", costs, "oracle", list(ref))
    assert len(costs) == len(ref)                                  # the same steps accepted
    np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])
    assert costs[-1] < 0.2 * costs[0]


def test_bundle_solves_are_bitwise_reproducible():
    w = bundle(5, 131)
    out = []
    for _ in range(2):
        s = bundle_solver(w, "LMGPU")
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = bundle_params(w, False)
        costs = s.profiled_solve(prm)
        out.append((np.array(costs), [u.cpu().numpy() for u in unk]))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    for a, b in zip(out[0][1], out[1][1]):
        assert a.tobytes() == b.tobytes()


def test_backend_cpu_with_host_arrays_equals_backend_cuda():
    w = bundle(5, 131)
    res = {}
    for backend in ("backend_cuda", "backend_cpu"):
        s = bundle_solver(w, backend=backend)
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = bundle_params(w, False, host=backend == "backend_cpu")
        cost = s.solve(prm)
        res[backend] = (cost, [np.asarray(u.cpu().numpy() if hasattr(u, "cpu") else u) for u in unk])
    assert res["backend_cpu"][0] == res["backend_cuda"][0]
    for a, b in zip(res["backend_cpu"][1], res["backend_cuda"][1]):
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(res["backend_cpu"][1][2], w["X"])     # the host arrays were written back


@pytest.mark.parametrize("NC,NP", SIZES)
def test_unknown_layout_lists_blocks_of_different_lengths(NC, NP):
    w = bundle(NC, NP)
    s = bundle_solver(w)
    assert s.unknown_layout() == ([0, 3 * NC, 6 * NC], [NC, NC, NP], [3, 3, 3])
    assert s.unknown_count() == 6 * NC + 3 * NP


@pytest.mark.parametrize("slot,size", [("c", "NC"), ("p", "NP"), ("o", "NO")])
def test_slot_index_outside_its_own_space_stops_the_solve(slot, size):
    """Each slot is checked against ITS space on the host before any kernel reads it: an
    index equal to that space's size (valid for a larger space of the same energy)."""
    w = dict(bundle(5, 131))
    bad = w[slot].copy()
    bad[7] = w[size]
    w[slot] = bad
    s = bundle_solver(w)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = bundle_params(w, False)
    before = [u.clone() for u in unk]
    with pytest.raises(api.OptError, match=f"slot '{slot}': vertex index {w[size]} outside"):
        s.init(prm)
    assert s.lib.Opt_ProblemStep(s.state, s.plan, s._pk.ptr) == 0
    with pytest.raises(api.OptError, match="outside"):
        s.step()
    for a, b in zip(before, unk):
        assert bool((a == b).all())


def test_refusals_name_their_cause(capfd):
    w = bundle(5, 131)
    s = bundle_solver(w)
    capfd.readouterr()
    group = s.lib.OptAMD_LocalGroupCreate(2)
    with pytest.raises(api.OptError, match="OptAMD_PlanSetDecomposition failed"):
        s.set_decomposition(s.lib.OptAMD_LocalGroupRank(group, 0), 0, 1)
    s.lib.OptAMD_LocalGroupDestroy(group)
    assert "no row-slab decomposition for an energy over several index spaces" in capfd.readouterr().err
    assert s.jacobian_shape()[1] == -1
    for kw in ({"materialized": True}, {"materialized": True, "fused_jtj": True}):
        with pytest.raises(api.OptError, match="Opt_ProblemPlan failed"):
            bundle_solver(w, **kw)
        assert "useMaterializedJTJ / useFusedJTJ) for an energy over several index spaces" in capfd.readouterr().err
    import torch
    prm, _ = bundle_params(w, False)
    rp = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(api.OptError, match="OptAMD_EvalJacobian failed"):
        s.eval_jacobian(prm, rp, rp, torch.zeros(16, device="cuda"))
    assert "OptAMD_EvalJacobian) for an energy over several index spaces" in capfd.readouterr().err


# ---------------------------------------------------------------------------- row bias
def solve_with_excluded_centres(model, cost_rows, active, n_iter, l_iter, lm, use_pre=False):
    """The C oracle's GN / LM loop (oracle_solve_f64, as examples_ad.solve drives it) with
    the reference's Exclude rule, which examples_ad.solve does not have: cost and model cost
    sum only the rows `cost_rows`; r = -J^T F and J^T J p keep every row and vanish on the
    excluded unknowns, as the kernels write them. use_pre: UsePreconditioner(true), the
    diagonal preconditioner on the active unknowns. Returns the costs after init and after
    each step."""
    import ctypes
    lib = ad._c.load()
    lib.oracle_solve_f64.restype = ctypes.c_int
    lib.oracle_solve_f64.argtypes = [ctypes.POINTER(ad._Problem), ctypes.c_int, ctypes.POINTER(ad._Params), ad._D]
    n = model.n
    act = np.ascontiguousarray(active, np.uint8)
    mask = act.astype(np.float64)
    st = {}

    def arr(ptr):
        return np.ctypeslib.as_array(ptr, shape=(n,))

    def cost(_):
        F = model.residuals()[cost_rows]
        return 0.5 * float(F @ F)

    def jtf(_, r, diag):
        st["J"] = model.jacobian()
        arr(r)[:] = -(st["J"].T @ model.residuals()) * mask
        arr(diag)[:] = model.diag_access

    def apply(_, p, Ap):
        pv = arr(p) * mask
        out = (st["J"].T @ (st["J"] @ pv)) * mask
        arr(Ap)[:] = out
        return float(pv @ out)

    def model_cost(_, d):
        m = (model.residuals() + st["J"] @ (arr(d) * mask))[cost_rows]
        return 0.5 * float(m @ m)

    def update(_, d):
        model.set(model.get() + arr(d) * mask)

    def save(_):
        st["prev"] = model.get()

    def revert(_):
        model.set(st["prev"])

    cbs = [ad._COST(cost), ad._JTF(jtf), ad._APPLY(apply), ad._MODEL(model_cost), ad._UPD(update),
           ad._VOID(save), ad._VOID(revert)]
    P = ad._Problem(n, act.ctypes.data, int(use_pre), None, *cbs, None, None)
    sp = ad.default_params(n_iter, l_iter)
    costs = np.zeros(n_iter + 1)
    k = lib.oracle_solve_f64(ctypes.byref(P), int(lm), ctypes.byref(sp), costs.ctypes.data_as(ad._D))
    return costs[: k + 1]


_ROWS = {}


def row_bias(W, H):
    if (W, H) in _ROWS:
        return _ROWS[(W, H)]
    rng = np.random.default_rng(100 * W + H)
    n = W * H
    yy, xx = np.mgrid[0:H, 0:W]
    truth = np.sin(0.3 * xx) + 0.1 * yy
    bias = rng.normal(0, 0.3, H)
    px = np.flatnonzero(rng.random(n) >= 0.10).astype(np.int32)   # an edge per pixel except 10 %
    px = px[rng.permutation(len(px))]
    w = dict(W=W, H=H, E=len(px), px=px, row=(px // W).astype(np.int32), w_s=0.5, w_b=0.05,
             D=f32(truth + bias[:, None] + rng.normal(0, 0.02, (H, W))), Mask=f32(rng.random((H, W)) < 0.15),
             I=f32(truth + rng.normal(0, 0.05, (H, W))), B=f32(rng.normal(0, 0.05, H)))
    _ROWS[(W, H)] = w
    return w


def row_bias_model(w):
    W, H = w["W"], w["H"]
    n = W * H
    m = ad.Model([("I", w["I"].reshape(n, 1)), ("B", w["B"].reshape(H, 1))], {"D": w["D"].reshape(n, 1)})
    ws, wb = float(np.float32(w["w_s"])), float(np.float32(w["w_b"]))
    masked = w["Mask"].reshape(-1) == 1
    keep = []
    m.term(lambda i, b, d: i + b - d, [("u", "I", w["px"]), ("u", "B", w["row"]), ("c", "D", w["px"])], 1)
    keep.append(np.ones(len(w["px"]), bool))
    yy, xx = np.mgrid[0:H, 0:W]
    for dx, dy in ((1, 0), (0, 1)):
        ok = (xx + dx < W) & (yy + dy < H)
        i0, i1 = (xx + W * yy)[ok], ((xx + dx) + W * (yy + dy))[ok]
        m.term(lambda a, b: ws * (a - b), [("u", "I", i0), ("u", "I", i1)], 1)
        keep.append(~masked[i0])
    m.term(lambda b: wb * b, [("u", "B", np.arange(H))], 1)
    keep.append(np.ones(H, bool))
    m.cost_rows = np.concatenate(keep)
    m.active = np.concatenate([~masked, np.ones(H, bool)]).astype(np.uint8)   # every B is active
    return m, m.active


def row_bias_params(w, double):
    T = np.float64 if double else np.float32
    unk = [cuda(w["I"].astype(T)), cuda(w["B"].astype(T))]
    return [w["w_s"], w["w_b"]] + unk + [cuda(w[k]) for k in ("D", "Mask", "px", "row")], unk


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("W,H", [(37, 29), (1, 9)])
def test_row_bias_kernels_match_oracle(W, H, double):
    w = row_bias(W, H)
    s = OptSolver([W, H, w["E"]], RB, double_precision=double)
    assert s.family() == "generic" and s.unknown_layout() == ([0, W * H], [W * H, H], [1, 1])
    prm, _ = row_bias_params(w, double)
    m, active = row_bias_model(w)
    r, pre, Ap = check_kernels(s, prm, kernel_reference(("rb", W, H), m, active, use_pre=False, cost_rows=m.cost_rows),
                              double, seed=W)
    off = active == 0
    assert off[: W * H].any() and not off[W * H:].any()
    for v in (r, pre, Ap):                         # zero on the masked elements, and only there
        assert not v[off].any() and np.all(v[~off] != 0)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("W,H", [(37, 29), (1, 9)])
def test_row_bias_solve_matches_oracle(W, H, kind, double):
    w = row_bias(W, H)
    s = OptSolver([W, H, w["E"]], RB, kind, double_precision=double)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = row_bias_params(w, double)
    start = unk[0].cpu().numpy().copy()
    costs = s.profiled_solve(prm)
    if ("rb", W, H, kind) not in _SOLVE:
        m, active = row_bias_model(w)
        _SOLVE[("rb", W, H, kind)] = solve_with_excluded_centres(m, m.cost_rows, active, 3, 10, kind == "LMGPU")
    ref = _SOLVE[("rb", W, H, kind)]
    print("costs", costs, "oracle", list(ref))
    assert len(costs) == len(ref)
    np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])
    end = unk[0].cpu().numpy()
    masked = w["Mask"] == 1
    assert end[masked].tobytes() == start[masked].tobytes()       # excluded pixels: untouched, bitwise
    assert np.any(end[~masked] != start[~masked])
    assert np.all(unk[1].cpu().numpy() != w["B"])                  # every B moved


# ------------------------------------- a SampledImage energy with a second unknown space
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("W,H,N", [(64, 48, 70), (130, 7, 3)])
def test_sampled_image_energy_with_a_second_space_matches_oracle(tmp_path, W, H, N, double):
    """optical_flow.t plus an unknown B over {N} with the residual B - 0.5: the per-Step sample
    cache (value and gradient images) is filled over the image's space. The flow block
    equals the optical-flow oracle (the bars of tests/test_generic_gpu.py); the B block is
    analytic: B = 0 gives cost N / 8, r = 0.5, J^T J p = p."""
    from oracle import oracle
    from tests.test_multispace_frontend import flow_with_calibration
    from tests.test_optical_flow_gpu import params as of_params, perturbed as of_perturbed

    w = of_perturbed(W, H, seed=W * H)
    s = OptSolver([W, H, N], flow_with_calibration(tmp_path), "LMGPU", double_precision=double)
    assert s.family() == "generic" and s.unknown_layout() == ([0, 2 * W * H], [W * H, N], [2, 1])
    prm = of_params(w, double) + [zeros(N, double)]
    tol = 1e-12 if double else 2e-5
    assert s.eval_cost(prm) == pytest.approx(oracle.of_cost(w, double=double) + N / 8, rel=max(tol, 1e-6))
    n, nf = 2 * W * H + N, 2 * W * H
    r, pre = zeros(n, double), zeros(n, double)
    s.eval_jtf(prm, r, pre)
    r = r.cpu().numpy()
    r_ref, _ = oracle.of_jtf(w, double=double)
    assert rel_err(r[:nf], r_ref) < tol * 10
    assert np.all(r[nf:] == 0.5) and np.all(pre.cpu().numpy() == 0.25)
    p = np.random.default_rng(2).normal(size=n)
    Ap = zeros(n, double)
    pT = p.astype(np.float64 if double else np.float32)
    pAp = s.apply_jtj(prm, cuda(pT), Ap)
    Ap = Ap.cpu().numpy()
    Ap_ref, pAp_ref = oracle.of_apply(w, p[:nf], double=double)
    assert rel_err(Ap[:nf], Ap_ref) < tol * 10
    assert np.array_equal(Ap[nf:], pT[nf:])
    assert pAp == pytest.approx(pAp_ref + float(pT[nf:].astype(np.float64) @ pT[nf:]), rel=max(tol, 1e-6))
