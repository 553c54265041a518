"""GPU: tan tanh sinh cosh asin acos atan asinh acosh log10 atan2 on the generated kernels,
against the float64 AD oracle (oracle.examples_ad.Model; the models are built here).

Per function: the one-line energy Energy(f(X(0)) - D(0)) below, at and above one wave.
Every kernel form (gather, LDS tiles, register strips) of a 2-D energy whose residuals read
neighbours through tan / atan, so that the per-Step transcendental cache engages, with a
masked acos residual whose masked pixels lie outside acos's domain (the mask must not be
factored onto Jp there). The graph record cache on and off for tan / atan of slot reads.

Tolerances (tests/test_generic_gpu.py, tests/test_multispace_gpu.py: tols): fp32 per-unknown
outputs within 2e-5 of the largest magnitude, scalars within 1e-5 relative; fp64 1e-9 / 1e-9.
Inputs are rounded to fp32 first and stay strictly inside each function's domain, away from
where its derivative blows up, so the float64 model itself is well conditioned."""
import numpy as np
import pytest

from opt_amd import OptSolver, api
from oracle import examples_ad as ad
from tests.test_elementary_functions_frontend import FUNCTIONS, one_line_energy
from tests.test_multispace_gpu import check_kernels, cuda, f32, kernel_reference, rel_err, tols

pytestmark = pytest.mark.gpu

# the interval each function's argument is drawn from
DOMAIN = {"tan": (-1.2, 1.2), "asin": (-0.9, 0.9), "acos": (-0.9, 0.9), "acosh": (1.2, 4.0), "log10": (0.2, 5.0),
          "sinh": (-2.0, 2.0), "cosh": (-2.0, 2.0), "tanh": (-2.0, 2.0), "atan": (-3.0, 3.0), "asinh": (-3.0, 3.0)}
NP_NAME = {"asin": "arcsin", "acos": "arccos", "atan": "arctan", "asinh": "arcsinh", "acosh": "arccosh"}


def _torch_fn(f):
    import torch
    return getattr(torch, f)


def atan2_inputs(N, rng):
    """(N, 2) points (a, b) = r (sin phi, cos phi) with r in [0.5, 2]: a^2 + b^2 >= 0.25, the
    four quadrants in turn, and every fifth point within 0.05 of the cut at +-pi, on
    alternating sides (the first point too, so N = 1 sits at the cut)."""
    k = np.arange(N)
    phi = (k % 4) * (np.pi / 2) - np.pi + rng.uniform(0.1, np.pi / 2 - 0.1, N)
    cut = k % 5 == 0
    phi[cut] = np.where((k[cut] // 5) % 2 == 0, np.pi - 0.05, -np.pi + 0.05) * rng.uniform(0.99, 1.0, cut.sum())
    r = rng.uniform(0.5, 2.0, N)
    X = f32(np.stack([r * np.sin(phi), r * np.cos(phi)], 1))
    assert np.all(np.sum(X.astype(np.float64) ** 2, 1) >= 0.25)
    if N >= 64:
        a, b = X[:, 0], X[:, 1]
        assert all(np.any((np.sign(a) == sa) & (np.sign(b) == sb)) for sa in (-1, 1) for sb in (-1, 1))
        assert np.any((b < 0) & (a > 0) & (a < 0.15)) and np.any((b < 0) & (a < 0) & (a > -0.15))
    return X


_INPUTS = {}


def inputs(f, N):
    """X (N, channels) and D (N,), rounded to fp32. D keeps every residual between 0.3 and 1 in
    magnitude, so that the cost does not hinge on a cancellation."""
    if (f, N) not in _INPUTS:
        rng = np.random.default_rng(1000 * FUNCTIONS.index(f) + N)
        if f == "atan2":
            X = atan2_inputs(N, rng)
            val = np.arctan2(X[:, 0].astype(np.float64), X[:, 1].astype(np.float64))
        else:
            lo, hi = DOMAIN[f]
            X = f32(rng.uniform(lo, hi, (N, 1)))
            X = np.clip(X, np.float32(lo), np.float32(hi))
            val = getattr(np, NP_NAME.get(f, f))(X[:, 0].astype(np.float64))
        D = f32(val - rng.choice([-1.0, 1.0], N) * rng.uniform(0.3, 1.0, N))
        _INPUTS[(f, N)] = (X, D)
    return _INPUTS[(f, N)]


def function_model(f, X, D):
    N = len(X)
    m = ad.Model([("X", X)], {"D": D.reshape(N, 1)})
    fn = _torch_fn(f)
    ids = np.arange(N)
    if f == "atan2":
        m.term(lambda x, d: (fn(x[0], x[1]) - d[0]).reshape(1), [("u", "X", ids), ("c", "D", ids)], 1)
    else:
        m.term(lambda x, d: fn(x) - d, [("u", "X", ids), ("c", "D", ids)], 1)
    return m


@pytest.fixture(scope="module")
def energy_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("elementary")
    out = {}
    for f in FUNCTIONS:
        p = d / (f + ".t")
        p.write_text(one_line_energy(f))
        out[f] = str(p)
    for name, text in (("forms", forms_energy(False)), ("forms_masked", forms_energy(True)), ("graph", GRAPH)):
        p = d / (name + ".t")
        p.write_text(text)
        out[name] = str(p)
    return out


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("N", [1, 64, 65, 300])
@pytest.mark.parametrize("f", FUNCTIONS)
def test_function_kernels_match_oracle(energy_files, f, N, double):
    """Cost, -J^T F with the preconditioner and J^T J p of Energy(f(X(0)) - D(0)). The energy has
    no UsePreconditioner statement: the preconditioner is the one of a unit diagonal."""
    X, D = inputs(f, N)
    s = OptSolver([N], energy_files[f], double_precision=double)
    assert s.family() == "generic" and s.unknown_count() == X.size
    prm = [cuda(X.astype(np.float64 if double else np.float32)), cuda(D)]
    ref = kernel_reference(("ef", f, N), function_model(f, X, D), use_pre=False)
    check_kernels(s, prm, ref, double, seed=N)


# ------------------------------------------------------------------ every kernel form
def forms_energy(masked):
    text = ('local W,H = Dim("W",0), Dim("H",1)\n'
            'local X = Unknown("X", opt_float, {W,H}, 0)\n'
            'local D = Array("D", opt_float, {W,H}, 1)\n'
            'local Mask = Array("Mask", opt_float, {W,H}, 2)\n'
            "UsePreconditioner(true)\n"
            "Energy(Select(InBounds(1,0), tan(X(0,0)) - tan(X(1,0)), 0))\n"
            "Energy(Select(InBounds(0,1), atan(X(0,0)) - atan(X(0,1)), 0))\n")
    if masked:
        text += "Energy(Select(eq(Mask(0,0),0), acos(X(0,0)) - D(0,0), 0))\n"
    return text


_FORMS = {}


def forms_inputs(W, H, masked):
    if (W, H, masked) not in _FORMS:
        rng = np.random.default_rng(100 * W + H)
        X = f32(rng.uniform(-0.9, 0.9, (H, W)))
        D = f32(rng.uniform(-1.0, 1.0, (H, W)))
        Mask = f32(rng.random((H, W)) < 0.25) if masked else np.zeros((H, W), np.float32)
        X[Mask == 1] = 5.0                       # outside acos's domain: acos and its partial are NaN there
        _FORMS[(W, H, masked)] = (X, D, Mask)
    return _FORMS[(W, H, masked)]


def forms_model(W, H, X, D, Mask, masked):
    import torch
    n = W * H
    m = ad.Model([("X", X.reshape(n, 1))], {"D": D.reshape(n, 1)})
    yy, xx = np.mgrid[0:H, 0:W]
    for (dx, dy), fn in (((1, 0), torch.tan), ((0, 1), torch.atan)):
        ok = (xx + dx < W) & (yy + dy < H)
        i0, i1 = (xx + W * yy)[ok], ((xx + dx) + W * (yy + dy))[ok]
        m.term(lambda a, b, fn=fn: fn(a) - fn(b), [("u", "X", i0), ("u", "X", i1)], 1)
    if masked:
        on = np.flatnonzero(Mask.reshape(-1) == 0)     # a masked row is 0 and has no partials
        m.term(lambda x, d: torch.acos(x) - d, [("u", "X", on), ("c", "D", on)], 1)
    return m


# (apply, J^T F, cost): every form of each at least once
FORMS = [("gather", "gather", "gather"), ("tiled", "gather", "strip"), ("strip", "strip", "gather"),
         ("strip", "strip", "strip")]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("W,H", [(5, 3), (70, 9)])
def test_every_kernel_form_matches_oracle(monkeypatch, energy_files, W, H, masked, double):
    """The centred transcendental cache holds tan / atan (/ acos) of X per pixel; the gather,
    tiled and strip forms read it (or the strips' row windows) and agree with the model and
    with each other. Masked: X = 5 under the mask, where acos and its partial are NaN; the
    Select must discard them in every form, so the outputs are finite and the model's."""
    path = energy_files["forms_masked" if masked else "forms"]
    src = api.generic_source(path, double)
    for k in ("gen_apply_tiled", "gen_apply_strip", "gen_jtf_strip", "gen_cost_strip", "gen_precompute_0"):
        assert k in src                                   # the forms exist, so the knobs select them
    X, D, Mask = forms_inputs(W, H, masked)
    assert not masked or (Mask == 1).sum() >= 2
    ref = kernel_reference(("forms", W, H, masked), forms_model(W, H, X, D, Mask, masked))
    out = []
    for apply, jtf, cost in FORMS:
        monkeypatch.setenv("OPT_AMD_GEN_APPLY", apply)
        monkeypatch.setenv("OPT_AMD_GEN_JTF", jtf)
        monkeypatch.setenv("OPT_AMD_GEN_COST", cost)
        s = OptSolver([W, H], path, double_precision=double)
        assert s.family() == "generic"
        prm = [cuda(X.astype(np.float64 if double else np.float32)), cuda(D), cuda(Mask)]
        r, pre, Ap = check_kernels(s, prm, ref, double, seed=W)
        assert all(np.isfinite(v).all() for v in (r, pre, Ap))
        out.append((r, pre, Ap))
    vec = tols(double)[0]
    for o in out[1:]:
        for a, b in zip(o, out[0]):
            assert rel_err(a, b) < vec


# ------------------------------------------------------------------ graph record cache
GRAPH = ('local N, E = Dim("N", 0), Dim("E", 1)\n'
         'local X = Unknown("X", opt_float, {N}, 0)\n'
         'local D = Array("D", opt_float, {N}, 1)\n'
         'local G = Graph("G", {E}, "a", {N}, 2, "b", {N}, 3)\n'
         "UsePreconditioner(true)\n"
         "Energy(0.5 * (X(0) - D(0)))\n"
         "Energy(tan(X(G.a)) - atan(X(G.b)))\n")


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("N", [7, 300])
def test_graph_record_cache_on_and_off(monkeypatch, energy_files, N, double):
    """tan / atan of slot reads come from the per-vertex record (one precompute per Step) or,
    with OPT_AMD_GEN_GRAPH_CACHE=0, are evaluated at every edge: both match the model and
    agree with each other."""
    import torch
    rng = np.random.default_rng(N)
    X, D = f32(rng.uniform(-1.2, 1.2, (N, 1))), f32(rng.uniform(-1, 1, (N, 1)))
    a = np.concatenate([np.arange(N), rng.integers(0, N, 2 * N)]).astype(np.int32)
    b = ((a + 1 + rng.integers(0, N - 1, len(a))) % N).astype(np.int32)          # b != a
    order = rng.permutation(len(a))
    a, b = a[order], b[order]
    m = ad.Model([("X", X)], {"D": D})
    m.term(lambda x, d: 0.5 * (x - d), [("u", "X", np.arange(N)), ("c", "D", np.arange(N))], 1)
    m.term(lambda xa, xb: torch.tan(xa) - torch.atan(xb), [("u", "X", a), ("u", "X", b)], 1)
    ref = kernel_reference(("graph", N), m)
    out = {}
    for c in ("1", "0"):
        monkeypatch.setenv("OPT_AMD_GEN_GRAPH_CACHE", c)
        assert ("gen_precompute_0" in api.generic_source(energy_files["graph"], double)) == (c == "1")
        s = OptSolver([N, len(a)], energy_files["graph"], double_precision=double)
        assert s.family() == "generic"
        prm = [cuda(X.astype(np.float64 if double else np.float32)), cuda(D), cuda(a), cuda(b)]
        out[c] = check_kernels(s, prm, ref, double, seed=N)
    for u, v in zip(out["0"], out["1"]):
        assert rel_err(u, v) < tols(double)[0]
