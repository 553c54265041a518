"""GPU: energies/pose_graph_2d.t on the generated kernels, against the float64 AD oracle
(oracle.examples_ad.Model / solve; the model is built here).

Poses on a closed loop with noise, odometry constraints plus loop closures, random SPD
information matrices with off-diagonal entries. Headings are stored on different turns
(+-2 pi) so that theta_j - theta_i - z2 lies near +-2 pi on many constraints while the wrapped
error stays within +-0.5: without the atan2(sin d, cos d) wrap those residuals would be ~6.
No wrapped error comes within 0.1 of the cut at +-pi, so fp32 cannot flip the branch.

Per kernel (cost, J^T F with the preconditioner, J^T J p); whole GN / LM solves; bitwise
determinism; backend_cpu == backend_cuda; the block preconditioner; inputs through the g2o
reader. Tolerances (tests/test_generic_gpu.py, test_multispace_gpu.py: tols): fp32 per-unknown
outputs within 2e-5 of the largest magnitude, scalars 1e-5 relative, solves 1e-4; fp64 1e-9 /
1e-9 / 1e-8."""
import os

import numpy as np
import pytest

from opt_amd import OptSolver
from opt_amd.harness import formats, problems
from oracle import examples_ad as ad
from tests.test_multispace_gpu import check_kernels, cuda, f32, kernel_reference, tols

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = os.path.join(ROOT, "energies", "pose_graph_2d.t")
SIZES = [40, 200]
W_ANCHOR = 10.0


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


_GRAPH = {}


def pose_graph(N):
    """The g2o-level description (float64 values that are exact in fp32): start poses V, edges
    (ij, z, info), the anchored pose; built once per size."""
    if N in _GRAPH:
        return _GRAPH[N]
    rng = np.random.default_rng(N)
    phi = 2 * np.pi * np.arange(N) / N
    R = 0.5 * N / (2 * np.pi)                                     # ~0.5 between neighbours
    truth = np.stack([R * np.cos(phi), R * np.sin(phi), phi + np.pi / 2], 1)   # headings pi/2 .. 5 pi/2
    i = np.concatenate([np.arange(N - 1), [N - 1], rng.integers(0, N, N // 4)])
    j = np.concatenate([np.arange(1, N), [0], np.zeros(N // 4, np.int64)])
    far = np.arange(N, len(i))
    j[far] = (i[far] + rng.integers(2, N - 2, len(far))) % N      # loop closures: any other pose
    order = rng.permutation(len(i))
    i, j = i[order], j[order]
    E = len(i)
    c, s = np.cos(truth[i, 2]), np.sin(truth[i, 2])
    dt = truth[j, :2] - truth[i, :2]
    z = np.stack([c * dt[:, 0] + s * dt[:, 1], -s * dt[:, 0] + c * dt[:, 1], wrap(truth[j, 2] - truth[i, 2])], 1)
    z += rng.normal(0, 1, (E, 3)) * [0.02, 0.02, 0.01]
    z[::3, 2] += 2 * np.pi * rng.choice([-1, 1], len(z[::3]))     # measured angles on another turn
    B = rng.normal(0, 1, (E, 3, 3))
    info = 4.0 * (np.einsum("eab,ecb->eac", B, B) + 2.0 * np.eye(3))
    V = truth + rng.normal(0, 1, (N, 3)) * [0.1, 0.1, 0.08]
    V[:, 2] += 2 * np.pi * rng.integers(-1, 2, N)                 # headings on different turns
    V, z, info = f32(V).astype(np.float64), f32(z).astype(np.float64), f32(info).astype(np.float64)
    info = 0.5 * (info + info.transpose(0, 2, 1))
    d = V[j, 2] - V[i, 2] - z[:, 2]
    assert np.abs(wrap(d)).max() < 0.5                            # far from the cut at +-pi
    assert (np.abs(d) > 5.5).sum() >= E // 4 and (d > 5.5).any() and (d < -5.5).any()
    _GRAPH[N] = (V, (np.stack([i, j], 1).astype(np.int32), z, info), np.array([N // 3], np.int32))
    return _GRAPH[N]


def arrays(N):
    """The energy's arrays, built directly (not through opt_amd.harness.problems)."""
    V, (ij, z, info), fixed = pose_graph(N)
    U = np.stack([np.linalg.cholesky(m).T for m in info])
    A = np.zeros(N, np.float32)
    A[fixed] = 1
    return dict(N=N, E=len(ij), w_anchor=W_ANCHOR, P=f32(V), P0=f32(V), A=A, Z=f32(z), U0=f32(U[:, 0, :]),
                U1=f32(np.stack([U[:, 1, 1], U[:, 1, 2], U[:, 2, 2]], 1)),
                i=ij[:, 0].copy(), j=ij[:, 1].copy(), e=np.arange(len(ij), dtype=np.int32))


def model(w):
    import torch
    m = ad.Model([("P", w["P"])], {k: w[k].reshape(len(w[k]), -1) for k in ("P0", "A", "Z", "U0", "U1")})
    wa = float(np.float32(w["w_anchor"]))
    ids = np.arange(w["N"])
    m.term(lambda p, p0, a: wa * a[0] * (p - p0), [("u", "P", ids), ("c", "P0", ids), ("c", "A", ids)], 3)

    def constraint(pi, pj, z, u0, u1):
        c, s = torch.cos(pi[2]), torch.sin(pi[2])
        dx, dy = pj[0] - pi[0], pj[1] - pi[1]
        e0 = c * dx + s * dy - z[0]
        e1 = -s * dx + c * dy - z[1]
        d = pj[2] - pi[2] - z[2]
        e2 = torch.atan2(torch.sin(d), torch.cos(d))
        return torch.stack([u0[0] * e0 + u0[1] * e1 + u0[2] * e2, u1[0] * e1 + u1[1] * e2, u1[2] * e2])

    m.term(constraint, [("u", "P", w["i"]), ("u", "P", w["j"]), ("c", "Z", w["e"]), ("c", "U0", w["e"]),
                        ("c", "U1", w["e"])], 3)
    return m


def params(w, double, host=False):
    put = (lambda a: np.ascontiguousarray(a)) if host else cuda
    prm = problems.pose_graph_2d_params(w, put, double)
    return prm, prm[1]


def solver(w, kind="gaussNewtonGPU", double=False, energy=PG, **kw):
    return OptSolver([w["N"], w["E"]], energy, kind, double_precision=double, **kw)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_kernels_match_oracle(N, double):
    w = arrays(N)
    s = solver(w, double=double)
    assert s.family() == "generic" and s.unknown_layout() == ([0], [N], [3])
    prm, _ = params(w, double)
    ref = kernel_reference(("pg", N), model(w))
    # the wrap is in force: the unwrapped angle rows alone would put the cost far above this
    d = (w["P"][w["j"], 2] - w["P"][w["i"], 2] - w["Z"][:, 2]).astype(np.float64)
    assert 0.5 * float(np.sum((w["U1"][:, 2] * d) ** 2)) > 20 * ref[0]
    check_kernels(s, prm, ref, double, seed=N)


_SOLVE = {}


def oracle_costs(N, kind):
    if (N, kind) not in _SOLVE:
        _SOLVE[(N, kind)] = ad.solve(model(arrays(N)), 3, 10, lm=kind == "LMGPU")
    return _SOLVE[(N, kind)]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("N", SIZES)
def test_solve_matches_oracle(N, kind, double):
    w = arrays(N)
    s = solver(w, kind, double)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, _ = params(w, double)
    costs = s.profiled_solve(prm)
    ref = oracle_costs(N, kind)
    print("costs", costs, "oracle", list(ref))
    assert len(costs) == len(ref)                                  # the same steps accepted
    np.testing.assert_allclose(costs, ref, rtol=tols(double)[2])
    assert costs[-1] < 0.2 * costs[0]


def test_solves_are_bitwise_reproducible():
    w = arrays(200)
    out = []
    for _ in range(2):
        s = solver(w, "LMGPU")
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = params(w, False)
        costs = s.profiled_solve(prm)
        out.append((np.array(costs), unk.cpu().numpy()))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert not np.array_equal(out[0][1], w["P"])


def test_backend_cpu_with_host_arrays_equals_backend_cuda():
    w = arrays(200)
    res = {}
    for backend in ("backend_cuda", "backend_cpu"):
        s = solver(w, backend=backend)
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        prm, unk = params(w, False, host=backend == "backend_cpu")
        cost = s.solve(prm)
        res[backend] = (cost, np.asarray(unk.cpu().numpy() if hasattr(unk, "cpu") else unk))
    assert res["backend_cpu"][0] == res["backend_cuda"][0]
    assert res["backend_cpu"][1].tobytes() == res["backend_cuda"][1].tobytes()
    assert not np.array_equal(res["backend_cpu"][1], w["P"])      # the host array was written back


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("N", SIZES)
def test_block_preconditioner_variant(tmp_path, N, kind):
    """UsePreconditioner("block") substituted for the statement: one 3 x 3 block per pose; it
    ends no higher than 1.05 x the scalar plan's final cost at the same iteration counts."""
    text = open(PG).read()
    assert text.count("UsePreconditioner(true)") == 1
    blk = tmp_path / "pose_graph_2d_block.t"
    blk.write_text(text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")'))
    w = arrays(N)
    final = {}
    for name, energy in (("scalar", PG), ("block", str(blk))):
        s = solver(w, kind, energy=energy)
        assert s.family() == "generic"
        assert s.preconditioner_blocks() == (([0], [0], 1) if name == "block" else ([], [], 0))
        s.set_solver_params({"nIterations": 3, "lIterations": 10})
        costs = s.profiled_solve(params(w, False)[0])
        print(name, costs)
        assert np.isfinite(costs).all() and costs[-1] < costs[0]
        final[name] = costs[-1]
    assert final["block"] <= 1.05 * final["scalar"]


def test_inputs_through_the_g2o_reader(tmp_path):
    """write_g2o -> read_g2o -> problems.pose_graph_2d gives the arrays built directly above,
    and so the same cost, bit for bit."""
    N = 40
    V, edges, fixed = pose_graph(N)
    path = str(tmp_path / "loop.g2o")
    formats.write_g2o(path, V, edges, fixed, ids=[3 * k + 100 for k in range(N)])
    v2, e2, f2 = formats.read_g2o(path)
    w2, dims = problems.pose_graph_2d(v2, e2, f2, w_anchor=W_ANCHOR)
    w = arrays(N)
    assert dims == [w["N"], w["E"]]
    for k in ("P", "P0", "A", "Z", "U0", "U1", "i", "j", "e"):
        assert np.array_equal(w2[k], w[k]) and w2[k].dtype == w[k].dtype, k
    c = solver(w).eval_cost(params(w, False)[0])
    c2 = OptSolver(dims, PG).eval_cost(problems.pose_graph_2d_params(w2, cuda))
    assert c2 == c and c == pytest.approx(kernel_reference(("pg", N), model(w))[0], rel=tols(False)[1])
