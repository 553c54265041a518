"""A test energy whose Jacobian is an arbitrary sparse matrix, for the materialized path
(csr.h): per-vertex fit rows and three rows per graph edge over three freely chosen
vertices, so the sparsity of J, J^T and J^T J is whatever the edge list says — rows of
every length, empty neighbourhoods, SELL slices of different widths, repeated columns.

Layout (generateDumpJ): rows 2v + ch are the fit rows of vertex v, rows 2N + 3e + {0,1,2}
the rows of edge e; unknown (v, ch) is column 2v + ch.

Everything here is CPU only: the energy text, the graph variants, the inputs, and the
analytic J in float64 as a dense matrix, written from the energy's partials and the
inputs — never from what the device dumps."""
import functools
import os

import numpy as np

ENERGY_TEXT = """local N, E = Dim("N", 0), Dim("E", 1)
local w_fit = Param("w_fit", float, 0)
local w_reg = Param("w_reg", float, 1)
local X  = Unknown("X", opt_float2, {N}, 2)
local T  = Array("T", opt_float2, {N}, 3)
local Wt = Array("Wt", float, {N}, 4)
local M  = Array("M", float, {N}, 5)
local G  = Graph("G", {E}, "a", {N}, 6, "b", {N}, 7, "c", {N}, 8)
UsePreconditioner(true)
Exclude(greater(M(0), 0.5))
Energy(w_fit * (X(0) - T(0)))
Energy(w_reg * (Wt(G.a) * X(G.a) - 2 * Wt(G.b) * X(G.b) + Wt(G.c) * X(G.c)))
local xa, xb = X(G.a), X(G.b)
Energy(w_reg * (xa(0) * xb(1) - Wt(G.c) * X(G.c)(0)))
"""

N_VERT = 197       # 394 unknowns: 7 SELL slices, the last one partial (10 rows)
N_WIRED = 190      # vertices N_WIRED .. N_VERT-1 appear in no edge
E_MODERATE = 260
E_HUB = 150
HUB_EDGES = 40     # edges whose slot a is vertex 0
VARIANTS = ("moderate", "hub", "dups", "tiny")


def write_energy(tmp_path):
    p = os.path.join(str(tmp_path), "sparse_graph.t")
    with open(p, "w") as f:
        f.write(ENERGY_TEXT)
    return p


def _triples(rng, E, lo=0):
    """E triples of distinct vertices in [lo, N_WIRED)."""
    out = np.empty((E, 3), np.int32)
    for e in range(E):
        out[e] = lo + rng.choice(N_WIRED - lo, size=3, replace=False)
    return out


def _graph(N, abc):
    abc = np.ascontiguousarray(abc, np.int32)
    g = {"N": int(N), "E": int(abc.shape[0]), "a": abc[:, 0].copy(), "b": abc[:, 1].copy(), "c": abc[:, 2].copy()}
    check_in_range(g)
    return g


def check_in_range(g):
    """Every index array of a fixture lies in [0, N): asserted before anything is bound."""
    for k in "abc":
        v = g[k]
        assert v.dtype == np.int32 and v.shape == (g["E"],)
        assert v.min() >= 0 and v.max() < g["N"], (k, int(v.min()), int(v.max()))


def random_wiring(seed, E=E_MODERATE):
    return _graph(N_VERT, _triples(np.random.default_rng(seed), E))


def hub_wiring(E=E_HUB, seed=5):
    """Vertex 0 in slot a of HUB_EDGES edges (their b, c distinct and not 0): columns
    (0, 0) and (0, 1) of J have one entry per such edge row, so two J^T J rows pass
    kMaxAtaRow = 64 and the whole pattern build takes the general path."""
    rng = np.random.default_rng(seed)
    abc = _triples(rng, E, lo=1)
    hub = rng.choice(E, size=HUB_EDGES, replace=False)
    abc[hub, 0] = 0
    return _graph(N_VERT, abc)


@functools.lru_cache(maxsize=None)
def variant(name):
    if name == "moderate":
        return random_wiring(11)
    if name == "hub":
        return hub_wiring()
    if name == "dups":   # repeated columns inside J rows: b == a on four edges, a == b == c on one
        g = random_wiring(11)
        abc = np.stack([g["a"], g["b"], g["c"]], 1)
        for e in (3, 64, 130, 259):
            abc[e, 1] = abc[e, 0]
        abc[200, :] = abc[200, 0]
        return _graph(N_VERT, abc)
    if name == "tiny":   # 10 unknowns: one partial slice; vertex 4 in no edge
        return _graph(5, np.array([[0, 1, 2], [3, 2, 0]], np.int32))
    raise KeyError(name)


def inputs(g, double, seed=3):
    """The arrays the plan binds, as numpy in the plan's own types (X, T in the plan's
    real type; Wt, M float; scalars rounded to fp32 first), M > 0.5 on about 10 % of the
    vertices."""
    N = g["N"]
    rng = np.random.default_rng(seed)
    dt = np.float64 if double else np.float32
    w = {"w_fit": float(np.float32(0.75)), "w_reg": float(np.float32(1.3)),
         "X": rng.uniform(0.5, 1.5, (N, 2)).astype(dt) * rng.choice([-1.0, 1.0], (N, 2)).astype(dt),
         "T": rng.normal(size=(N, 2)).astype(dt),
         "Wt": rng.uniform(0.5, 1.5, N).astype(np.float32),
         "M": (rng.uniform(size=N) < 0.1).astype(np.float32)}
    if N <= 8:
        w["M"][:] = 0
        w["M"][1] = 1
    return w


def active(g, w):
    """Per unknown: True where the vertex is solved for (M <= 0.5)."""
    return np.repeat(w["M"] <= 0.5, 2)


def direction(g, w, double, seed=1):
    """A random p in the plan's type, zero on the excluded unknowns."""
    p = np.random.default_rng(seed).normal(size=2 * g["N"]) * active(g, w)
    return p.astype(np.float64 if double else np.float32)


def entries(g, w):
    """Every stored entry of J as (row, col, value) float64 arrays, repeated (row, col)
    pairs kept apart. Partials of the energy: fit rows w_fit; reg rows w_reg Wt(a),
    -2 w_reg Wt(b), w_reg Wt(c); third row w_reg X(b)(1) at (a, 0), w_reg X(a)(0) at
    (b, 1), -w_reg Wt(c) at (c, 0). The inputs are those of inputs(): already rounded to
    the plan's types, promoted here."""
    N, E = g["N"], g["E"]
    a, b, c = (g[k].astype(np.int64) for k in "abc")
    wf, wr = np.float64(np.float32(w["w_fit"])), np.float64(np.float32(w["w_reg"]))
    X, Wt = w["X"].astype(np.float64), w["Wt"].astype(np.float64)
    rows, cols, vals = [np.arange(2 * N)], [np.arange(2 * N)], [np.full(2 * N, wf)]
    e = np.arange(E)
    for ch in (0, 1):
        for v, val in ((a, wr * Wt[a]), (b, -2.0 * wr * Wt[b]), (c, wr * Wt[c])):
            rows.append(2 * N + 3 * e + ch)
            cols.append(2 * v + ch)
            vals.append(val)
    for col, val in ((2 * a, wr * X[b, 1]), (2 * b + 1, wr * X[a, 0]), (2 * c, -wr * Wt[c])):
        rows.append(2 * N + 3 * e + 2)
        cols.append(col)
        vals.append(val)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def shape(g):
    """(rows, columns, stored nonzeros) of J."""
    return 2 * g["N"] + 3 * g["E"], 2 * g["N"], 2 * g["N"] + 9 * g["E"]


def analytic(g, w, double):
    """Dense float64 (J, |J| with repeated columns' magnitudes added, one-ulp matrix): the
    last is the sum over an entry's stored parts of the spacing of the plan's type at that
    part, the unit of the assembly test's bound."""
    rows, cols, _ = shape(g)
    r, c, v = entries(g, w)
    dt = np.float64 if double else np.float32
    J, Jabs, ulp = np.zeros((rows, cols)), np.zeros((rows, cols)), np.zeros((rows, cols))
    np.add.at(J, (r, c), v)
    np.add.at(Jabs, (r, c), np.abs(v))
    np.add.at(ulp, (r, c), np.spacing(np.abs(v).astype(dt)).astype(np.float64))
    return J, Jabs, ulp


def structure(g):
    """Integer count matrix of J's stored entries (repeated columns counted), from the
    index arrays alone."""
    rows, cols, _ = shape(g)
    r, c, _ = entries(g, {"w_fit": 1.0, "w_reg": 1.0, "X": np.ones((g["N"], 2)), "Wt": np.ones(g["N"])})
    S = np.zeros((rows, cols), np.int64)
    np.add.at(S, (r, c), 1)
    return S


def row_ptr(g):
    N, E = g["N"], g["E"]
    return np.concatenate([np.arange(2 * N), 2 * N + 3 * np.arange(3 * E + 1)]).astype(np.int32)


def pattern_stats(g):
    """From the structure alone: stored lengths of the J^T rows, lengths of the structural
    J^T J rows (stored zeros counted), SELL-64 slice widths of both, the pair-list depth
    of every J^T J slot group (the trip count of ata_from_pairs), nnz of both."""
    S = structure(g)
    lenT = S.sum(0)
    prod = S.T @ S                      # products summed into every J^T J entry
    lenA = (prod > 0).sum(1)

    def widths(lens):
        return [int(lens[s:s + 64].max()) for s in range(0, len(lens), 64)]

    depths = []
    for s in range(0, S.shape[1], 64):
        lists = [prod[i][prod[i] > 0] for i in range(s, min(s + 64, S.shape[1]))]
        for j in range(max(len(l) for l in lists)):
            depths.append(int(max(l[j] for l in lists if len(l) > j)))
    return {"lenT": lenT, "lenA": lenA, "widthsT": widths(lenT), "widthsA": widths(lenA), "depths": depths,
            "nnzJ": int(S.sum()), "nnzJTJ": int((prod > 0).sum())}


def reference_apply(g, w, p, double):
    """(ref, tol, pAp reference, pAp tolerance) of the masked apply against the dense
    float64 J: ref = act * (J^T (J p)); componentwise
        tol_i = (m_i + 8) eps (|J|^T |J| |p|)_i,   m_i = 3 len(J^T row i) + 3
    (m_i: the products and additions that reach row i, fused or not — a J row has at most
    3 entries, so a J^T J row at most 3 len entries of at most len products each; + 8:
    the roundings of the J entries themselves), and
        |pAp - p.ref| <= sum |p_i| tol_i + 8 eps sum |p_i ref_i|."""
    J, Jabs, _ = analytic(g, w, double)
    act = active(g, w)
    p = p.astype(np.float64)
    ref = act * (J.T @ (J @ p))
    eps = float(np.finfo(np.float64 if double else np.float32).eps)
    m = 3 * structure(g).sum(0) + 3
    tol = (m + 8) * eps * (Jabs.T @ (Jabs @ np.abs(p)))
    return ref, tol, float(p @ ref), float(np.abs(p) @ tol + 8 * eps * np.abs(p * ref).sum())
