"""GPU: the device builder of the explicit forms' symbolic phase (opt_amd/csrc/schur_pattern_dev.hip,
OptAMD_SchurPatternDevice / OptAMD_NormalPatternDevice) against the host builder
(schur_pattern.h, OptAMD_SchurPattern / OptAMD_NormalPattern): the three counts and rowPtr,
colInd, pairPtr and pairs must be equal element for element, the refusals word for word.

The public functions return no long-block or long-row list; those are compared through the plans
(tests/test_symbolic_plan_gpu.py: the star's long row, the parallel edges' long blocks)."""
import numpy as np
import pytest

from opt_amd import api

pytestmark = pytest.mark.gpu
LONG_PAIRS, LONG_ROW = 128, 64        # gen::kSchurLongPairs, gen::kNormalLongRow (codegen.h)
i32 = lambda *v: np.array(v, np.int32)


def same(host, dev):
    assert dev[0] == host[0], (dev[0], host[0])
    for name, a, b in zip(("rowPtr", "colInd", "pairPtr", "pairs"), host[1:], dev[1:]):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a, b), name
    return host


def schur(nE, nR, lists):
    return same(api.schur_pattern(nE, nR, lists), api.schur_pattern(nE, nR, lists, device=True))


def normal(n, lists, graph_edges=None):
    return same(api.normal_pattern(n, lists, graph_edges), api.normal_pattern(n, lists, graph_edges, device=True))


# ------------------------------------------------------------------ small shapes, both modes
def test_empty_list_and_one_retained_element():
    counts = schur(3, 1, [(i32(), i32())])[0]
    assert counts == {"instances": 0, "pairs": 0, "blocks": 1}
    assert schur(2, 1, [(i32(0, 1, 1), i32(0, 0, 0))])[0] == {"instances": 3, "pairs": 5, "blocks": 1}
    assert schur(2, 4, [(i32(), i32()), (i32(1, 0), i32(3, 3))])[0]["blocks"] == 4
    assert normal(1, [i32(), i32()])[0] == {"instances": 0, "pairs": 0, "blocks": 1}
    assert normal(1, [i32(0, 0), i32(0, 0)])[0] == {"instances": 4, "pairs": 4, "blocks": 1}
    assert normal(3, [(0, i32()), (1, i32(2)), (1, i32(2))], [0, 1])[0]["blocks"] == 3


def test_where_the_inserted_diagonal_lands():
    """Rows with no pair at all (only the inserted diagonal), rows whose pairs lie only right of
    the diagonal (inserted first), only left (last), on both sides without it (in the middle), and
    the last row without a diagonal (pairPtr falls back to the pair count)."""
    # Schur: retained row r gets a block (r, c) only together with (r, r), so the diagonal is
    # missing only on rows without any pair: rows 1, 3 and the last
    counts, row_ptr, col_ind, pair_ptr, _ = schur(2, 6, [(i32(0, 0, 1), i32(0, 2, 4))])
    assert list(np.diff(row_ptr)) == [2, 1, 2, 1, 1, 1] and pair_ptr[-1] == pair_ptr[-2] == counts["pairs"]
    # J^T J: an edge (a, b) gives (a, b) and (b, a) and no diagonal
    ii, jj = i32(0, 3, 3, 2, 5), i32(4, 1, 5, 0, 1)
    counts, row_ptr, col_ind, pair_ptr, _ = normal(7, [ii, jj])
    rows = [list(col_ind[row_ptr[r]:row_ptr[r + 1]]) for r in range(7)]
    assert rows == [[0, 2, 4], [1, 3, 5], [0, 2], [1, 3, 5], [0, 4], [1, 3, 5], [6]]
    assert pair_ptr[-1] == pair_ptr[-2] == counts["pairs"] == 10
    # the last row without a diagonal but with pairs left of it
    counts, row_ptr, col_ind, pair_ptr, _ = normal(3, [i32(2, 2), i32(0, 1)])
    assert list(col_ind[row_ptr[2]:]) == [0, 1, 2] and pair_ptr[-2] == pair_ptr[-1] == 4


def test_duplicates_and_a_point_seen_once():
    ev, rv = i32(1, 0, 1, 1, 2, 0, 1), i32(2, 0, 2, 1, 3, 0, 2)       # (1, 2) three times, point 2 once
    counts = schur(4, 5, [(ev, rv)])[0]
    assert counts["pairs"] == 4 + 16 + 1
    counts = normal(4, [i32(0, 0, 1, 0), i32(1, 1, 2, 1)])[0]         # the edge (0, 1) three times
    assert counts == {"instances": 8, "pairs": 8, "blocks": 8}


@pytest.mark.parametrize("k", [2, 3])
def test_several_lists_over_two_graphs(k):
    rng = np.random.default_rng(40 + k)
    ne = [37, 22]
    lists = [(rng.integers(0, 9, ne[l % 2]).astype(np.int32), rng.integers(0, 13, ne[l % 2]).astype(np.int32))
             for l in range(k)]
    assert schur(9, 13, lists)[0]["instances"] == sum(len(a) for a, _ in lists)
    graphs = [0, 1, 1][:k]
    nl = [(g, rng.integers(0, 13, ne[g]).astype(np.int32)) for g in graphs]
    assert normal(13, nl, ne)[0]["instances"] == sum(ne[g] for g in graphs)


def random_schur(seed, pairs):
    """One list whose points' observation counts, squared, sum to `pairs` exactly."""
    rng = np.random.default_rng(seed)
    k, left = [], pairs
    while left:
        c = int(min(rng.integers(1, 60), np.floor(np.sqrt(left))))
        k.append(c)
        left -= c * c
    nE = len(k) + 3                                                   # three points nobody sees
    ev = rng.permutation(np.repeat(rng.permutation(nE)[:len(k)], k)).astype(np.int32)
    return nE, ev, rng.integers(0, 300, len(ev)).astype(np.int32)


@pytest.mark.parametrize("pairs", [255, 256, 257, 65537])
def test_random_schur_inputs_around_one_workgroup_of_pairs(pairs):
    nE, ev, rv = random_schur(pairs, pairs)
    assert schur(nE, 300, [(ev, rv)])[0]["pairs"] == pairs


# k (k - 1) is even for every k: an odd pair total cannot occur in this mode, so the even totals
# on both sides of 255, 257 and 65 537 stand for them
@pytest.mark.parametrize("pairs", [254, 256, 258, 65536, 65538])
def test_random_distinct_inputs_around_one_workgroup_of_pairs(pairs):
    """Graph 0 with three slots (6 pairs per edge), graph 1 with two (2 per edge)."""
    rng = np.random.default_rng(pairs)
    a = int(rng.integers(1, pairs // 12))
    ne = [a, (pairs - 6 * a) // 2]
    lists = [(g, rng.integers(0, 97, ne[g]).astype(np.int32)) for g in (0, 1, 0, 1, 0)]
    assert normal(97, lists, ne)[0]["pairs"] == pairs


# ------------------------------------------------------------------ Schur mode only
def test_one_vertex_with_300_instances():
    """90 000 pairs of one eliminated vertex, spread over many workgroups, and blocks above the
    one-wave assembly's bound."""
    rng = np.random.default_rng(5)
    ev = np.concatenate([np.full(300, 2), rng.integers(0, 6, 50)]).astype(np.int32)
    rv = np.concatenate([rng.integers(0, 7, 300), rng.integers(0, 9, 50)]).astype(np.int32)
    order = rng.permutation(350)
    counts, _, _, pair_ptr, _ = schur(6, 9, [(ev[order], rv[order])])
    assert counts["pairs"] >= 90000 and (np.diff(pair_ptr) > LONG_PAIRS).sum() >= 49


def test_refuses_more_pairs_than_an_int_indexes():
    """tests/test_schur_explicit_frontend.py's refusal, with the host's message character for character."""
    n = 46341
    lists = [(np.zeros(n, np.int32), np.zeros(n, np.int32))]
    msgs = []
    for device in (False, True):
        with pytest.raises(api.OptError) as e:
            api.schur_pattern(1, 1, lists, device=device)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "%d instance pairs over %d edge instances" % (n * n, n) in msgs[1]


def test_bad_index_is_refused_on_the_host_as_before():
    with pytest.raises(api.OptError, match="vertex index outside its space at edge 1"):
        api.schur_pattern(3, 2, [(i32(0, 3), i32(0, 1))], device=True)
    with pytest.raises(api.OptError, match="vertex index outside its space at edge 1"):
        api.normal_pattern(3, [i32(0, 3), i32(0, 1)], device=True)


def test_more_retained_elements_than_a_four_byte_key_takes():
    """Above 65 536 retained elements the sort keys are 8 bytes wide."""
    rng = np.random.default_rng(9)
    ev, rv = rng.integers(0, 50, 400).astype(np.int32), rng.integers(0, 70000, 400).astype(np.int32)
    rv[:3] = [69999, 65536, 0]
    schur(50, 70000, [(ev, rv)])
    normal(70000, [rv[:200], rv[200:]])


# ------------------------------------------------------------------ distinct mode only
def test_self_loops():
    counts, row_ptr, col_ind, pair_ptr, pairs = normal(4, [i32(0, 1, 2, 2), i32(0, 2, 2, 3)])
    assert counts["pairs"] == 8 and pair_ptr[1] - pair_ptr[0] == 2   # block (0, 0): (q0, q4), (q4, q0)


def test_four_slot_edges():
    rng = np.random.default_rng(2)
    lists = [rng.integers(0, 30, 45).astype(np.int32) for _ in range(4)]
    assert normal(30, lists)[0]["pairs"] == 12 * 45


def star_and_parallel(n=200):
    rng = np.random.default_rng(12)
    far = rng.choice(np.arange(10, n), 80, replace=False)
    ring = np.arange(n)
    i = np.concatenate([ring, np.zeros(80, np.int64), np.full(140, 5)]).astype(np.int32)
    j = np.concatenate([(ring + 1) % n, far, np.full(140, 6)]).astype(np.int32)
    return i, j


def test_parallel_edges_and_a_hub_row():
    i, j = star_and_parallel()
    _, row_ptr, col_ind, pair_ptr, _ = normal(200, [i, j])
    assert row_ptr[1] - row_ptr[0] > LONG_ROW and (np.diff(row_ptr)[1:] <= LONG_ROW).all()
    b56 = row_ptr[5] + list(col_ind[row_ptr[5]:row_ptr[6]]).index(6)
    assert pair_ptr[b56 + 1] - pair_ptr[b56] == 141 > LONG_PAIRS
    assert (np.diff(pair_ptr) > LONG_PAIRS).sum() == 2


def test_distinct_refuses_more_pairs_than_an_int_indexes():
    """tests/test_normal_matrix_frontend.py's refusal: 256 lists of one graph, 32 897 edges."""
    ne, k = 32897, 256
    v = np.zeros(ne, np.int32)
    msgs = []
    for device in (False, True):
        with pytest.raises(api.OptError) as e:
            api.normal_pattern(1, [(0, v)] * k, [ne], device=device)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    assert 'NormalMatrix("explicit"): %d instance pairs over %d edge instances' % (k * (k - 1) * ne, k * ne) in msgs[1]
