"""CPU: the fixtures of tests/test_materialized_graph_gpu.py reach the branches they are
there for. Everything is asserted from the analytic structure of J (the index arrays), so
an edit of a seed or an edge count cannot quietly drop a branch of csr.hip from the GPU
tests: the one-thread-per-row pattern path against the general one (kMaxAtaRow = 64),
prod_map's register rows (<= 16) against its long rows, sell_spmv's unroll by 4 and its
tail, ata_from_pairs' unroll by 2 and its tail, a partial last slice, near-empty rows."""
import numpy as np
import pytest

from opt_amd import api
from tests import materialized_graph_helpers as mg


def test_energy_runs_on_the_generated_kernels(tmp_path):
    path = mg.write_energy(tmp_path)
    assert api.problem_family(path) == "generic"
    d = api.generic_describe(path)
    # 2 fit rows with 1 unknown each, then 3 edge rows with 3 unknowns each
    assert [ln.split()[:2] for ln in d] == [["centred", "1"]] * 2 + [["graph0", "3"]] * 3, d


@pytest.mark.parametrize("name", mg.VARIANTS)
def test_variants_are_in_range_and_sized(name):
    g = mg.variant(name)
    mg.check_in_range(g)
    st = mg.pattern_stats(g)
    rows, cols, nnz = mg.shape(g)
    assert st["nnzJ"] == nnz and len(mg.row_ptr(g)) == rows + 1 and mg.row_ptr(g)[-1] == nnz
    if name == "tiny":
        assert cols == 10 and st["widthsT"] == [5]   # a single partial slice
        return
    assert g["N"] == mg.N_VERT and cols == 394 and len(st["widthsT"]) == 7 and cols % 64 != 0
    used = np.unique(np.concatenate([g["a"], g["b"], g["c"]]))
    assert used.max() < mg.N_WIRED   # vertices 190..196 in no edge: J^T rows of length 1
    same = (g["a"] == g["b"]) | (g["b"] == g["c"]) | (g["a"] == g["c"])
    if name == "dups":
        assert np.count_nonzero(g["a"] == g["b"]) >= 4
        assert np.count_nonzero((g["a"] == g["b"]) & (g["b"] == g["c"])) == 1
        assert mg.structure(g).max() == 3   # one column three times in a row
    else:
        assert not same.any() and mg.structure(g).max() == 1


def _slices_vary(widths):
    full = widths[:-1]   # the last slice is the partial one
    return any(a != b for a, b in zip(full, full[1:])) and any(w % 4 for w in full) and any(w >= 4 for w in full)


@pytest.mark.parametrize("name", ["moderate", "hub", "dups"])
def test_variants_reach_every_branch(name):
    st = mg.pattern_stats(mg.variant(name))
    lenA, lenT = st["lenA"], st["lenT"]
    if name == "hub":
        assert np.count_nonzero(lenA > 64) >= 2          # ata_pattern_general, prod_map's long rows
    else:
        assert lenA.max() <= 64                          # ata_rows, the fast pattern path
        assert np.count_nonzero(lenA <= 16) >= 20        # prod_map<16>: rows in registers
        assert np.count_nonzero((lenA > 16) & (lenA <= 64)) >= 20   # and its long-row branch
    assert np.count_nonzero(lenT == 1) >= 5              # near-empty J^T rows
    # sell_spmv: consecutive slices of different width, the unrolled loop and a tail
    assert _slices_vary(st["widthsT"]), st["widthsT"]
    assert _slices_vary(st["widthsA"]), st["widthsA"]
    # ata_from_pairs: pair lists of odd and of even depth, beyond one trip of the unroll by 2
    d = np.array(st["depths"])
    assert np.any((d % 2 == 1) & (d >= 3)) and np.any((d % 2 == 0) & (d >= 2))


WIRINGS = [("moderate", lambda: mg.variant("moderate")), ("second", lambda: mg.random_wiring(12)),
           ("hub260", lambda: mg.hub_wiring(E=mg.E_MODERATE)), ("moderate", lambda: mg.variant("moderate"))]


def test_rewired_graphs_differ_by_far_more_than_the_bound():
    """The sequence the GPU test binds to one plan: same N and E throughout (one plan),
    a different nnz(J^T J) at every change, the general pattern path in the middle — and
    reference applies so far apart that a pattern kept from the wiring before cannot pass."""
    gs = [mk() for _, mk in WIRINGS]
    assert len({(g["N"], g["E"]) for g in gs}) == 1
    st = [mg.pattern_stats(g) for g in gs]
    assert all(a["nnzJTJ"] != b["nnzJTJ"] for a, b in zip(st, st[1:]))
    assert st[1]["lenA"].max() <= 64 < st[2]["lenA"].max()
    for double in (False, True):
        w = mg.inputs(gs[0], double)
        p = mg.direction(gs[0], w, double)
        out = [mg.reference_apply(g, w, p, double) for g in gs]
        for (r0, t0, q0, qt0), (r1, t1, q1, qt1) in zip(out, out[1:]):
            act = t1 > 0
            assert np.count_nonzero(np.abs(r1 - r0)[act] > 1e3 * t1[act]) >= 100
            assert abs(q1 - q0) > 10 * qt1   # a sum over similar random graphs: the rows carry the weight
