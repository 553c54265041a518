"""CPU: the reader / writer of 2-D g2o pose graphs (opt_amd/harness/formats.py) and the arrays
problems.pose_graph_2d builds from one for energies/pose_graph_2d.t."""
import numpy as np
import pytest

from opt_amd.harness import formats, problems


def small_graph():
    rng = np.random.default_rng(5)
    V = rng.normal(size=(5, 3))
    ij = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [3, 1]], np.int32)
    z = rng.normal(size=(len(ij), 3))
    L = rng.normal(size=(len(ij), 3, 3)) + 3.0 * np.eye(3)
    info = np.einsum("eij,ekj->eik", L, L)                        # SPD, off-diagonal entries
    info = 0.5 * (info + info.transpose(0, 2, 1))
    return V, (ij, z, info)


def test_round_trip_with_ids_out_of_order_fix_and_comments(tmp_path):
    V, (ij, z, info) = small_graph()
    ids = [17, 3, 1000, 4, 0]
    path = str(tmp_path / "g.g2o")
    formats.write_g2o(path, V, (ij, z, info), fixed=[2, 4], ids=ids)
    text = open(path).read().splitlines()
    assert text[0].startswith("VERTEX_SE2 17 ") and "FIX 1000 0" in text
    assert sum(l.startswith("EDGE_SE2 ") for l in text) == len(ij) and "EDGE_SE2 4 3 " in "\n".join(text)
    # comments, blank lines and a trailing comment on a record
    text = ["# a pose graph", ""] + text[:3] + ["   ", "# half way"] + text[3:]
    text[2] += "   # the first pose"
    open(path, "w").write("\n".join(text) + "\n")
    V2, (ij2, z2, info2), fixed = formats.read_g2o(path)
    assert V2.dtype == np.float64 and np.array_equal(V2, V)       # repr round trip: exact
    assert ij2.dtype == np.int32 and np.array_equal(ij2, ij)      # ids renumbered in order of appearance
    assert np.array_equal(z2, z) and np.array_equal(info2, info)
    assert np.array_equal(info2, info2.transpose(0, 2, 1))
    assert fixed.tolist() == [2, 4]


def test_default_anchor_is_the_first_vertex(tmp_path):
    V, e = small_graph()
    path = str(tmp_path / "g.g2o")
    formats.write_g2o(path, V, e, ids=[9, 8, 7, 6, 5])
    assert "FIX" not in open(path).read()
    assert formats.read_g2o(path)[2].tolist() == [0]


def test_information_matrix_must_be_positive_definite(tmp_path):
    V, (ij, z, info) = small_graph()
    info = info.copy()
    info[3] = np.diag([1.0, -1.0, 1.0])                           # edge 3 -> 4, written as ids 13 -> 14
    path = str(tmp_path / "g.g2o")
    formats.write_g2o(path, V, (ij, z, info), ids=[10, 11, 12, 13, 14])
    with pytest.raises(ValueError, match=r"edge 13 -> 14 is not positive definite"):
        formats.read_g2o(path)
    with pytest.raises(ValueError, match=r"edge 3 \(3 -> 4\) is not positive definite"):
        problems.pose_graph_2d(V, (ij, z, info), [0])
    info[3] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])   # symmetric, indefinite
    formats.write_g2o(path, V, (ij, z, info))
    with pytest.raises(ValueError, match=r"edge 3 -> 4"):
        formats.read_g2o(path)


def test_malformed_files_name_the_line(tmp_path):
    path = str(tmp_path / "g.g2o")
    open(path, "w").write("VERTEX_SE2 0 0 0 0\nEDGE_SE2 0 5 1 0 0 1 0 0 1 0 1\n")
    with pytest.raises(ValueError, match=r":2: edge 0 -> 5 names vertex 5"):
        formats.read_g2o(path)
    open(path, "w").write("VERTEX_SE2 0 0 0 0\nVERTEX_SE3:QUAT 1 0 0 0 0 0 0 1\n")
    with pytest.raises(ValueError, match=r":2: unsupported record VERTEX_SE3:QUAT"):
        formats.read_g2o(path)


def test_problem_arrays():
    V, (ij, z, info) = small_graph()
    w, dims = problems.pose_graph_2d(V, (ij, z, info), [0, 3])
    assert dims == [5, 6] and (w["N"], w["E"]) == (5, 6)
    assert w["A"].tolist() == [1, 0, 0, 1, 0] and w["A"].dtype == np.float32
    assert np.array_equal(w["P"], V.astype(np.float32)) and np.array_equal(w["P0"], w["P"]) and w["P0"] is not w["P"]
    assert np.array_equal(w["i"], ij[:, 0]) and np.array_equal(w["j"], ij[:, 1]) and w["e"].tolist() == list(range(6))
    assert all(w[k].dtype == np.int32 for k in "ije")
    for k in range(6):                                            # U0 / U1 are the rows of U, info = U^T U
        U = np.array([w["U0"][k], [0, w["U1"][k][0], w["U1"][k][1]], [0, 0, w["U1"][k][2]]], np.float64)
        assert np.array_equal(U.astype(np.float32), np.linalg.cholesky(info[k]).T.astype(np.float32))
        np.testing.assert_allclose(U.T @ U, info[k], rtol=1e-5, atol=1e-5)
    prm = problems.pose_graph_2d_params(w, double=True)
    assert len(prm) == 10 and prm[0] == w["w_anchor"] and prm[1].dtype == np.float64 and prm[2].dtype == np.float32
