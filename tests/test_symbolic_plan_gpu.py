"""GPU: plans whose symbolic phase runs on the device (the default) against plans made under
OPT_AMD_SYMBOLIC=host: the same pattern, the same assembled matrix and the same solve, bit for
bit, on the workloads of tests/test_schur_explicit_gpu.py and tests/test_normal_matrix_gpu.py
(the bundle of 5 cameras and 131 points; pose graphs of 22 and 200 poses; the star whose hub row
takes the SpMV's long-row form and whose 140 parallel edges take the assembly's long-block form:
a wrong long-row or long-block list changes the values). OptSolver.symbolic_info() says which
path a plan took and why."""
import numpy as np
import pytest

from tests import test_normal_matrix_gpu as nm
from tests import test_schur_explicit_gpu as sx
from tests.test_pose_graph_gpu import PG, arrays, params
from tests.test_pose_graph_gpu import solver as pg_solver
from tests.test_schur_gpu import bundle, bundle_params, cuda
from tests.test_schur_gpu import solver as ba_solver

pytestmark = pytest.mark.gpu
KINDS = ["gaussNewtonGPU", "LMGPU"]
POSE_GRAPHS = {"pg22": lambda: arrays(22), "pg200": lambda: arrays(200), "star": nm.star_and_parallel}


def set_path(monkeypatch, path, max_bytes=None):
    """OPT_AMD_SYMBOLIC is read when the plan is made: set it before the solver."""
    for name, value in (("OPT_AMD_SYMBOLIC", path), ("OPT_AMD_SYMBOLIC_MAX_BYTES", max_bytes)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def counts_of(info):
    words = dict(kv.split("=") for kv in info.split())
    assert set(words) == {"path", "reason", "pairs", "blocks", "instances", "transient_bytes"}
    return {k: int(words[k]) for k in ("pairs", "blocks", "instances")}, int(words["transient_bytes"])


def host_arrays(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


def bundle_run(kind, double):
    w = bundle(5, 131)
    s = ba_solver(w, kind, double, path=sx.EXPLICIT)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = bundle_params(w, double)
    assert s.symbolic_info() == ""                                   # no symbolic phase yet
    matrix = host_arrays(s.reduced_matrix(prm))
    info = s.symbolic_info()
    costs = np.array(s.profiled_solve(prm))
    return info, matrix, costs, host_arrays(unk)


def pose_run(name, kind, double):
    w = POSE_GRAPHS[name]()
    s = pg_solver(w, kind, double, energy=nm.EXPLICIT)
    s.set_solver_params({"nIterations": 3, "lIterations": 10})
    prm, unk = params(w, double)
    assert s.symbolic_info() == ""
    matrix = host_arrays(s.normal_matrix(prm))
    info = s.symbolic_info()
    costs = np.array(s.profiled_solve(prm))
    return info, matrix, costs, [unk.cpu().numpy().copy()]


def assert_same_run(a, b):
    (info_a, mat_a, cost_a, unk_a), (info_b, mat_b, cost_b, unk_b) = a, b
    assert counts_of(info_a)[0] == counts_of(info_b)[0]
    for x, y in zip(mat_a + unk_a, mat_b + unk_b):                   # rowPtr, colInd, values; the unknowns
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert len(cost_a) >= 2 and cost_a.tobytes() == cost_b.tobytes()
    assert cost_a[-1] < cost_a[0]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_bundle_plans_agree_bitwise(monkeypatch, kind, double):
    set_path(monkeypatch, "host")
    host = bundle_run(kind, double)
    set_path(monkeypatch, None)
    dev = bundle_run(kind, double)
    assert host[0].startswith("path=host reason=env ") and counts_of(host[0])[1] == 0
    assert dev[0].startswith("path=device reason=default ") and counts_of(dev[0])[1] > 0
    assert counts_of(dev[0])[0]["pairs"] == 600 and counts_of(dev[0])[0]["blocks"] == 17
    assert_same_run(host, dev)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(POSE_GRAPHS))
def test_pose_graph_plans_agree_bitwise(monkeypatch, name, kind, double):
    set_path(monkeypatch, "host")
    host = pose_run(name, kind, double)
    set_path(monkeypatch, None)
    dev = pose_run(name, kind, double)
    assert host[0].startswith("path=host reason=env ")
    assert dev[0].startswith("path=device reason=default ")
    assert_same_run(host, dev)


def test_the_path_can_be_asked_for_by_name(monkeypatch):
    set_path(monkeypatch, "device")
    assert bundle_run("gaussNewtonGPU", False)[0].startswith("path=device reason=env ")


@pytest.mark.parametrize("form", ["bundle", "pg22"])
def test_a_footprint_above_the_cap_takes_the_host_path(monkeypatch, form):
    run = (lambda: bundle_run("LMGPU", False)) if form == "bundle" else (lambda: pose_run(form, "LMGPU", False))
    set_path(monkeypatch, "host")
    host = run()
    set_path(monkeypatch, None, max_bytes="1")
    capped = run()
    assert capped[0].startswith("path=host reason=memory ") and counts_of(capped[0])[1] > 1
    assert_same_run(host, capped)


def test_plans_with_neither_statement():
    w = bundle(5, 131)
    s = ba_solver(w, path=sx.IMPLICIT)
    s.init(bundle_params(w, False)[0])
    assert s.symbolic_info() == -1
    w = arrays(22)
    s = pg_solver(w, energy=PG)
    s.init(params(w, False)[0])
    assert s.symbolic_info() == -1
    assert s.lib.OptAMD_PlanSymbolicInfo(None, None, 0) == -1


# ------------------------------------------------------------------ re-wiring between Steps
def bundle_rewiring(in_place):
    w = bundle(5, 131)
    w2 = sx.rewired(w)
    s = ba_solver(w, path=sx.EXPLICIT)
    s.set_solver_params({"nIterations": 4, "lIterations": 10})
    s.set_kernel_timing(1)
    prm, unk = bundle_params(w, False)
    s.init(prm)
    assert s.step()
    assert s.kernel_stat("schur_symbolic")[0] == 1
    before = s.symbolic_info()
    state = host_arrays(unk)
    if in_place:                                                   # the same device arrays, rewritten
        for k, name in zip((9, 10, 11), ("c", "p", "o")):
            prm[k].copy_(cuda(w2[name]))
    else:                                                          # other arrays bound
        prm, unk = bundle_params(dict(w2, CamR=state[0], CamT=state[1], X=state[2]), False)
        for k, name in zip((5, 6, 7), ("CamR", "CamT", "X")):      # the priors stay where they were
            prm[k] = cuda(w[name])
    assert s.step(prm)
    assert s.kernel_stat("schur_symbolic")[0] == 2
    info = s.symbolic_info()
    assert counts_of(info)[0] != counts_of(before)[0]
    return info, host_arrays(s.reduced_matrix(prm)), np.array([s.cost()]), host_arrays(unk)


def pose_rewiring(in_place):
    w = arrays(40)
    w2 = nm.rewired(w)
    s = pg_solver(w, energy=nm.EXPLICIT)
    s.set_solver_params({"nIterations": 4, "lIterations": 10})
    s.set_kernel_timing(1)
    prm, unk = params(w, False)
    s.init(prm)
    assert s.step()
    assert s.kernel_stat("normal_symbolic")[0] == 1
    state = unk.cpu().numpy().copy()
    if in_place:
        for k, name in zip((4, 5, 6, 7, 8), ("Z", "U0", "U1", "i", "j")):
            prm[k].copy_(cuda(w2[name]))
    else:
        prm, unk = params(dict(w2, P=state), False)
        prm[2] = cuda(w["P0"])                                     # the prior stays where it was
    assert s.step(prm)
    assert s.kernel_stat("normal_symbolic")[0] == 2
    info = s.symbolic_info()
    return info, host_arrays(s.normal_matrix(prm)), np.array([s.cost()]), [unk.cpu().numpy().copy()]


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("rewiring", [bundle_rewiring, pose_rewiring])
def test_rewired_plans_stay_bitwise_equal(monkeypatch, rewiring, in_place):
    set_path(monkeypatch, "host")
    host = rewiring(in_place)
    set_path(monkeypatch, None)
    dev = rewiring(in_place)
    assert host[0].startswith("path=host reason=env ") and dev[0].startswith("path=device reason=default ")
    assert counts_of(host[0])[0] == counts_of(dev[0])[0]
    for x, y in zip(host[1] + host[3], dev[1] + dev[3]):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert host[2].tobytes() == dev[2].tobytes()
