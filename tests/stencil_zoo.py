"""A zoo of 2-D energies whose stencils are wide, one-sided or read knowns further out than
any unknown, with a float64 forward-mode AD reference (oracle.examples_ad.Model) for each.

The shipped energies are all radius 1 and symmetric; the kernel generator's geometry (lane
offset, outputs per wave, first / last centre row, one accumulator row per output offset,
per-array row windows, the output row's Exclude shifted by the lowest offset, the slab halo,
the tile shape) is computed for any stencil, and these four exercise it:

  A  one channel, one-sided: a known read beyond every unknown (A(3,0)), an unknown that is
     never read at the centre row (rows 1..3), a nonlinear diagonal pair with 3-lane shifts
  B  opt_float3 + opt_float2 unknowns (pair windows at an odd element offset when W*H is
     odd), a uint8 mask read at an offset by Exclude and by a Select, a Param
  C  reach 5 / 6 in x and 4 in y, no mask, no preconditioner
  D  an explicit InBounds inside a Select beside bbox-tested terms

The reference does not come from the generated source. Its instance rule restates the DSL's
(DESIGN.md 3.6 "Classification"; the reference's bboxforexpression): a residual is
instantiated at every pixel where ALL its reads (unknowns, knowns, masks; the centre
included) lie inside the image; a residual that uses InBounds decides for itself, exists at
every pixel, and its out-of-range reads are 0. Exclusion (tests/test_generic_gpu.py
volume_J): the cost sums instances centred on active pixels; J^T F, diag and J^T J take every
instance; rows of excluded unknowns are 0.
"""
import numpy as np

from oracle import examples_ad as ad

ENERGIES = {
    "A": """
local W, H = Dim("W", 0), Dim("H", 1)
local X = Unknown("X", opt_float, {W, H}, 0)
local A = Array("A", opt_float, {W, H}, 1)
local M = Array("M", opt_float, {W, H}, 2)
UsePreconditioner(true)
Exclude(Not(eq(M(0,0),0)))
Energy(X(0,0) - A(0,0))
Energy(0.7*(X(2,0) - X(0,0)) * A(3,0))
Energy(0.5*(X(0,1) - 2*X(0,2) + X(0,3)))
Energy(sin(X(-3,-1)) * X(1,2))
""",
    "B": """
local W, H = Dim("W", 0), Dim("H", 1)
local V = Unknown("V", opt_float3, {W, H}, 0)
local U = Unknown("U", opt_float2, {W, H}, 1)
local A = Array("A", opt_float2, {W, H}, 2)
local M = Array("M", uint8, {W, H}, 3)
local w = Param("w", float, 4)
UsePreconditioner(true)
Exclude(eq(M(-1,0),1))
Energy(U(0,0) - A(0,0))
Energy(0.5*(V(0,0) - Vector(A(0,0)(0), A(0,0)(1), 1.0)))
Energy(w*(U(0,-2) - U(1,0)))
Energy(Select(eq(M(2,1),0), V(0,0)(0)*U(-2,0)(1) - V(1,1)(2) + A(0,-1)(0), 0))
Energy(0.3*(V(0,0) - V(-1,2)))
""",
    "C": """
local W, H = Dim("W", 0), Dim("H", 1)
local X = Unknown("X", opt_float, {W, H}, 0)
local A = Array("A", opt_float, {W, H}, 1)
Energy(X(0,0) - A(0,0))
Energy(X(-5,0) - X(6,0))
Energy(X(0,-4) * X(0,4))
""",
    "D": """
local W, H = Dim("W", 0), Dim("H", 1)
local X = Unknown("X", opt_float, {W, H}, 0)
local A = Array("A", opt_float, {W, H}, 1)
local M = Array("M", opt_float, {W, H}, 2)
Exclude(Not(eq(M(0,0),0)))
Energy(X(0,0) - A(0,0))
Energy(Select(InBounds(2,-1) * eq(M(2,-1),0), 0.8*(X(0,0) - X(2,-1)) - A(1,0), 0))
Energy(0.4 * X(-2,3) * cos(X(0,0)))
""",
}

# Per energy, from its text above. terms: per Energy statement the (dx, dy) of EVERY read
# (unknown, known, mask), whether it uses InBounds, its scalar residuals and how many of its
# reads are unknown accesses per scalar residual (the nonzeros of a row of J).
# unknowns: (name, channels) in declaration order. exclude: the offset Exclude reads M at.
# halo: the largest vertical span of one term's reads (centre included), the exclusion's
# reach, at least 1 (the rows a slab needs of its neighbours).
ZOO = {
    "A": dict(unknowns=[("X", 1)], use_pre=True, exclude=(0, 0), halo=3,
              terms=[dict(reads=[(0, 0)], k=1, nnz=1),
                     dict(reads=[(2, 0), (0, 0), (3, 0)], k=1, nnz=2),
                     dict(reads=[(0, 1), (0, 2), (0, 3)], k=1, nnz=3),
                     dict(reads=[(-3, -1), (1, 2)], k=1, nnz=2)]),
    "B": dict(unknowns=[("V", 3), ("U", 2)], use_pre=True, exclude=(-1, 0), halo=2,
              terms=[dict(reads=[(0, 0)], k=2, nnz=1),
                     dict(reads=[(0, 0)], k=3, nnz=1),
                     dict(reads=[(0, -2), (1, 0)], k=2, nnz=2),
                     dict(reads=[(2, 1), (0, 0), (-2, 0), (1, 1), (0, -1)], k=1, nnz=3),
                     dict(reads=[(0, 0), (-1, 2)], k=3, nnz=2)]),
    "C": dict(unknowns=[("X", 1)], use_pre=False, exclude=None, halo=8,
              terms=[dict(reads=[(0, 0)], k=1, nnz=1),
                     dict(reads=[(-5, 0), (6, 0)], k=1, nnz=2),
                     dict(reads=[(0, -4), (0, 4)], k=1, nnz=2)]),
    "D": dict(unknowns=[("X", 1)], use_pre=False, exclude=(0, 0), halo=3,
              terms=[dict(reads=[(0, 0)], k=1, nnz=1),
                     dict(reads=[(0, 0), (2, -1), (1, 0)], k=1, nnz=2, bounds=True),
                     dict(reads=[(-2, 3), (0, 0)], k=1, nnz=2)]),
}
PARAM_W = 0.75   # B's Param, exact in fp32


def write_energy(tmp_dir, name):
    path = tmp_dir / f"zoo_{name}.t"
    path.write_text(ENERGIES[name])
    return str(path)


def halo_from_offsets(name):
    """The slab halo derived from the energy's offsets (ZOO's `reads`), not from the plan."""
    z = ZOO[name]
    h = 1
    for t in z["terms"]:
        ys = [dy for _, dy in t["reads"]] + [0]
        h = max(h, max(ys) - min(ys))
    if z["exclude"] is not None:
        h = max(h, abs(z["exclude"][1]))
    return h


def image_term(W, H, offsets, bounds=False):
    """The DSL's instance rule for a centred residual that reads at `offsets` (every read of
    the residual; the centre always counts). Without InBounds an instance exists where all
    reads lie inside the image; with it (bounds) at every pixel, and a read outside the image
    is 0. Returns (centres, idx, ok): the instances' centre pixels, per offset the pixel each
    instance reads (0 where outside) and whether that read is inside."""
    y, x = np.mgrid[0:H, 0:W]
    inside = {}
    for dx, dy in list(offsets) + [(0, 0)]:
        inside[(dx, dy)] = (x + dx >= 0) & (x + dx < W) & (y + dy >= 0) & (y + dy < H)
    keep = np.ones((H, W), bool) if bounds else np.logical_and.reduce(list(inside.values()))
    centres = (y * W + x)[keep]
    idx = {o: np.where(m, (y + o[1]) * W + (x + o[0]), 0)[keep] for o, m in inside.items()}
    ok = {o: m[keep] for o, m in inside.items()}
    return centres, idx, ok


def fits(name, W, H, t):
    """Whether the image is larger than term t's reach (bbox-tested terms only)."""
    xs = [dx for dx, _ in ZOO[name]["terms"][t]["reads"]] + [0]
    ys = [dy for _, dy in ZOO[name]["terms"][t]["reads"]] + [0]
    return W > max(xs) - min(xs) and H > max(ys) - min(ys)


_PROBLEMS = {}


def problem(name, W, H):
    """Inputs of energy `name` at W x H, built once: O(1) normals rounded to fp32 (kept as
    float64), a mask that excludes 15 % of the pixels (to the nearest pixel), the active map."""
    key = (name, W, H)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rng = np.random.default_rng(7919 * W + 31 * H + ord(name))
    n = W * H
    z = ZOO[name]
    r32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    w = dict(name=name, W=W, H=H)
    for nm, ch in z["unknowns"]:
        w[nm] = r32(rng.normal(size=(n, ch)))
    w["A"] = r32(rng.normal(size=(n, 2 if name == "B" else 1)))
    active = np.ones(n, bool)
    if z["exclude"] is not None:
        ex = z["exclude"][0]                       # Exclude tests M at (ex, 0): ex = 0 or -1
        y, x = np.mgrid[0:H, 0:W]
        can = np.flatnonzero((x + ex >= 0).reshape(-1))   # pixels whose test reads inside the image
        k = min(len(can), int(round(0.15 * n)))
        out = rng.choice(can, k, replace=False)
        M = np.zeros(n)
        M[out + ex] = 1.0
        active[out] = False
        w["M"] = M.astype(np.uint8 if name == "B" else np.float32)
    w["active"] = active
    _PROBLEMS[key] = w
    return w


def model(w, drop=None):
    """The float64 model of problem w: one term per Energy statement with at least one
    instance (drop: leave statement `drop` out). Returns (Model, active per unknown element,
    cost_rows: which rows of J / F are centred on an active pixel)."""
    import torch
    name, W, H = w["name"], w["W"], w["H"]
    z = ZOO[name]
    consts = {"A": w["A"]}
    if "M" in w:
        consts["M"] = w["M"].astype(np.float64)
    m = ad.Model([(nm, w[nm]) for nm, _ in z["unknowns"]], consts)
    cost_rows = []

    def add(t, fn, reads):
        """reads: (kind, array, offset) in fn's argument order"""
        if t == drop:
            return
        spec = z["terms"][t]
        offs = [o for _, _, o in reads]
        assert sorted(set(offs)) == sorted(set(spec["reads"])), (name, t)
        centres, idx, ok = image_term(W, H, offs, spec.get("bounds", False))
        if len(centres) == 0:
            return
        args = [(kind, arr, idx[o]) for kind, arr, o in reads]
        if spec.get("bounds"):
            # out-of-range reads are 0: each read's inside flag rides along as a constant
            for j, (_, _, o) in enumerate(reads):
                m.c[f"ok{t}_{j}"] = ok[o].astype(np.float64).reshape(-1, 1)
                args.append(("c", f"ok{t}_{j}", np.arange(len(centres))))
            nr = len(reads)
            inner = fn
            fn = lambda *a: inner(*[a[j] * a[nr + j] for j in range(nr)], *a[nr:])  # noqa: E731
        m.term(fn, args, spec["k"])
        cost_rows.append(np.repeat(w["active"][centres], spec["k"]))

    zero = lambda v: torch.zeros_like(v)  # noqa: E731
    if name == "A":
        add(0, lambda x, a: x - a, [("u", "X", (0, 0)), ("c", "A", (0, 0))])
        add(1, lambda x2, x0, a3: 0.7 * (x2 - x0) * a3, [("u", "X", (2, 0)), ("u", "X", (0, 0)), ("c", "A", (3, 0))])
        add(2, lambda x1, x2, x3: 0.5 * (x1 - 2 * x2 + x3), [("u", "X", (0, 1)), ("u", "X", (0, 2)), ("u", "X", (0, 3))])
        add(3, lambda xa, xb: torch.sin(xa) * xb, [("u", "X", (-3, -1)), ("u", "X", (1, 2))])
    elif name == "B":
        wv = PARAM_W
        add(0, lambda u, a: u - a, [("u", "U", (0, 0)), ("c", "A", (0, 0))])
        add(1, lambda v, a: 0.5 * (v - torch.stack([a[0], a[1], torch.ones_like(a[0])])),
            [("u", "V", (0, 0)), ("c", "A", (0, 0))])
        add(2, lambda ua, ub: wv * (ua - ub), [("u", "U", (0, -2)), ("u", "U", (1, 0))])
        add(3, lambda mk, v0, u, v1, a: torch.where(mk[0] == 0, v0[0] * u[1] - v1[2] + a[0], zero(a[0])).reshape(1),
            [("c", "M", (2, 1)), ("u", "V", (0, 0)), ("u", "U", (-2, 0)), ("u", "V", (1, 1)), ("c", "A", (0, -1))])
        add(4, lambda v0, v1: 0.3 * (v0 - v1), [("u", "V", (0, 0)), ("u", "V", (-1, 2))])
    elif name == "C":
        add(0, lambda x, a: x - a, [("u", "X", (0, 0)), ("c", "A", (0, 0))])
        add(1, lambda xa, xb: xa - xb, [("u", "X", (-5, 0)), ("u", "X", (6, 0))])
        add(2, lambda xa, xb: xa * xb, [("u", "X", (0, -4)), ("u", "X", (0, 4))])
    elif name == "D":
        add(0, lambda x, a: x - a, [("u", "X", (0, 0)), ("c", "A", (0, 0))])
        # InBounds(2,-1) is the inside flag of the read at (2,-1): fn's argument 3 + 1
        add(1, lambda x0, x1, a, mk, ok0, ok1, oka, okm: torch.where((okm * ok1 > 0) & (mk == 0),
                                                                     0.8 * (x0 - x1) - a, zero(a)),
            [("u", "X", (0, 0)), ("u", "X", (2, -1)), ("c", "A", (1, 0)), ("c", "M", (2, -1))])
        add(2, lambda xa, x0: 0.4 * xa * torch.cos(x0), [("u", "X", (-2, 3)), ("u", "X", (0, 0))])
    act = np.concatenate([np.repeat(w["active"], ch) for _, ch in z["unknowns"]])
    return m, act, np.concatenate(cost_rows)


def jacobian_counts(name, W, H):
    """(rows, nnz) of the materialized J as the plan sizes it: per pixel, every scalar residual
    of the energy text and every unknown access of each (instances outside the bbox keep
    their rows, with zero entries)."""
    rows = sum(t["k"] for t in ZOO[name]["terms"])
    nnz = sum(t["k"] * t["nnz"] for t in ZOO[name]["terms"])
    return rows * W * H, nnz * W * H


# What the generator emits for each energy beside the gathers: (apply, J^T F, cost) strip
# columns (None: not emitted) and the tile, per precision. From the offsets above: a scatter
# strip gives 64 - (lane reach of the reads) - (maxx - minx of the unknown offsets) outputs
# per wave, the cost strip 64 - (lane reach); B in fp64 passes the scatter strips' register
# cap (48 window + accumulator registers per lane in double), so it has neither.
EMITTED = {
    ("A", False): ((53, 53, 58), (11, 12)), ("A", True): ((53, 53, 58), (11, 12)),
    ("B", False): ((57, 57, 60), (13, 12)), ("B", True): ((None, None, 60), (13, 12)),
    ("C", False): ((42, 42, 53), (5, 8)), ("C", True): ((42, 42, 53), (5, 8)),
    ("D", False): ((56, 56, 60), (12, 12)), ("D", True): ((56, 56, 60), (12, 12)),
}


def sizes(name):
    """The test sizes of an energy: one pixel; smaller than every reach; one column short of a
    strip, a strip, one more (with 7 / 8 / 9 rows: a row block short, full, one more); two
    strips and a column with three row blocks, the last of one row; a tile and a column by
    two tiles and a row. S: the fp32 apply strip's columns (B in fp64 emits none)."""
    (S, _, _), (TX, TY) = EMITTED[(name, False)]
    return [(1, 1), (3, 2), (S - 1, 7), (S, 8), (S + 1, 9), (2 * S + 1, 17), (TX + 1, 2 * TY + 1)]
