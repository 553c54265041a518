"""GPU: blocks of A^-1 from the dense Cholesky factor (the dense_cov_* kernels of
opt_amd/csrc/dense_cholesky.hip) through the stand-alone entry point OptAMD_DenseInverseBlocks
(api.dense_inverse_blocks), in fp32 and fp64.

Truth: numpy's float64 inverse refined by two Newton-Schulz steps X <- X + X (I - A X) in
np.longdouble; its error is negligible against both precisions' bars.

Bar: max |Sigma - A^-1| <= 2 (n + 1) u kappa_2(A) ||A^-1||_2, u as in test_dense_cholesky_gpu.py,
kappa_2 and the norm from float64 numpy: the first-order bound, the factor's 2 (n + 1) u backward
error and the forward chain's each amplified by kappa_2. A numpy restatement of the algorithm
(same-precision Cholesky, column-wise forward substitution, Y^T Y) on spd(n, dt) at n = 1, 5, 63,
64, 65, 129, 200 sits at 0.004 - 0.21 of the bar in both precisions. Each test prints the GPU's
ratio.

Sizes: C = 1 at one tile (1, 5, 63), an exact tile (64), one past (65), three tiles with padding
(129), four (200); C = 3 at 21 elements (one tile-row of the right-hand sides), 22 (two) and
beyond; C = 6 and C = 8 around the same boundaries."""
import numpy as np
import pytest

from opt_amd import api
from tests.test_dense_cholesky_gpu import DTYPES, U, spd

pytestmark = pytest.mark.gpu
CASES = [(1, n) for n in (1, 5, 63, 64, 65, 129, 200)] + [(3, n) for n in (63, 66, 129, 192)] + \
        [(6, n) for n in (66, 126, 132)] + [(8, n) for n in (64, 72)]
_truth = {}


def refined_inverse(A):
    """float64 inverse + two Newton-Schulz steps in long double, rounded back to float64. The
    residual I - A X and the sum are formed in long double; the correction X (I - A X), itself
    of the size of the error, is a float64 product (long double products are not BLAS calls)."""
    A = np.asarray(A, np.longdouble)
    X = np.linalg.inv(A.astype(np.float64)).astype(np.longdouble)
    eye = np.eye(len(A), dtype=np.longdouble)
    for _ in range(2):
        R = np.asarray(eye - A @ X, np.float64)
        X = X + (np.asarray(X, np.float64) @ R).astype(np.longdouble)
    return np.asarray(X, np.float64)


def bar_of(A64, u):
    s = np.linalg.svd(A64, compute_uv=False)
    return 2 * (len(A64) + 1) * u * (s[0] / s[-1]) / s[-1]


def truth(n, dt):
    if (n, dt) not in _truth:
        A64 = spd(n, dt)[0].astype(np.float64)
        inv = refined_inverse(A64)
        inv.setflags(write=False)
        _truth[(n, dt)] = (inv, bar_of(A64, U[dt]))
    return _truth[(n, dt)]


def block(M, C, s, t):
    return M[s * C:(s + 1) * C, t * C:(t + 1) * C]


def boundary(n, C):
    """The two elements either side of row 64 (clipped to the matrix)."""
    ne = n // C
    lo = min(63 // C, ne - 1)
    hi = min(lo + 1 if 64 // C == lo else 64 // C, ne - 1)
    return lo, hi


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
@pytest.mark.parametrize("C,n", CASES)
def test_blocks_against_the_refined_inverse(C, n, dt):
    A = spd(n, dt)[0]
    inv, bar = truth(n, dt)
    ne = n // C
    worst = 0.0
    full, info = api.dense_inverse_blocks(A, C)                    # all diagonal blocks
    assert info == -1 and full.shape == (ne, C, C) and full.dtype == dt
    for e in range(ne):
        worst = max(worst, np.abs(full[e].astype(np.float64) - block(inv, C, e, e)).max())
    lo, hi = boundary(n, C)
    subset = sorted({0, ne - 1, lo, hi})
    sub, info = api.dense_inverse_blocks(A, C, elements=subset)
    assert info == -1 and sub.shape == (len(subset), C, C)
    for k, e in enumerate(subset):
        worst = max(worst, np.abs(sub[k].astype(np.float64) - block(inv, C, e, e)).max())
        assert np.abs(sub[k].astype(np.float64) - full[e].astype(np.float64)).max() <= bar
    pairs = [(0, ne - 1), (ne - 1, 0), (lo, hi), (hi, lo), (lo, lo)]
    pq, info = api.dense_inverse_blocks(A, C, pairs=pairs)
    assert info == -1 and pq.shape == (len(pairs), C, C)
    for k, (s, t) in enumerate(pairs):
        worst = max(worst, np.abs(pq[k].astype(np.float64) - block(inv, C, s, t)).max())
    sym = max(np.abs(pq[0].astype(np.float64) - pq[1].astype(np.float64).T).max(),
              np.abs(pq[2].astype(np.float64) - pq[3].astype(np.float64).T).max())
    # a block requested alone (its tile-row starts at its own panel: the skipped tiles) against
    # the same block among all
    alone, _ = api.dense_inverse_blocks(A, C, elements=[ne - 1])
    skip = np.abs(alone[0].astype(np.float64) - full[ne - 1].astype(np.float64)).max()
    one, _ = api.dense_inverse_blocks(A, C, pairs=[(0, ne - 1)])
    skip = max(skip, np.abs(one[0].astype(np.float64) - pq[0].astype(np.float64)).max())
    print(f"C={C} n={n} {np.dtype(dt).name}: max |Sigma - A^-1| / bar = {worst / bar:.3e}, "
          f"|(s,t) - (t,s)^T| / bar = {sym / bar:.3e}, alone vs among all / bar = {skip / bar:.3e}")
    assert worst <= bar
    assert sym <= bar
    assert skip <= bar


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
@pytest.mark.parametrize("C", (1, 3, 6, 8))
@pytest.mark.parametrize("n", (24, 120, 192))
def test_bidiagonal_factor_gives_the_inverse_exactly(n, C, dt):
    """L lower bidiagonal, 1 on the diagonal and -1 below, A = L L^T: (A^-1)_ij = n - max(i, j) and
    every intermediate of the factorisation, the chain and the Gram sums is a small integer."""
    L = np.eye(n) - np.eye(n, k=-1)
    A = (L @ L.T).astype(dt)
    i, j = np.indices((n, n))
    inv = (n - np.maximum(i, j)).astype(np.float64)
    ne = n // C
    full, info = api.dense_inverse_blocks(A, C)
    assert info == -1
    for e in range(ne):
        assert np.array_equal(full[e].astype(np.float64), block(inv, C, e, e))
    pq, info = api.dense_inverse_blocks(A, C, pairs=[(0, ne - 1)])
    assert info == -1
    assert np.array_equal(pq[0].astype(np.float64), block(inv, C, 0, ne - 1))


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
@pytest.mark.parametrize("bad", (0.0, np.nan), ids=("zero", "nan"))
def test_pivot_failure_reports_the_row_and_leaves_the_output(bad, dt):
    A = spd(129, dt)[0].copy()
    A[70, 70] = bad
    out = np.full((43, 3, 3), 7, dt)
    got, info = api.dense_inverse_blocks(A, 3, out=out)
    assert info == 70
    assert got is out and np.all(out == 7)


def test_bad_input_raises_before_any_launch():
    A = spd(65, np.float32)[0]
    with pytest.raises(ValueError):
        api.dense_inverse_blocks(A, 3)                             # 65 is no multiple of 3
    with pytest.raises(ValueError):
        api.dense_inverse_blocks(A, 1, elements=[65])
    with pytest.raises(ValueError):
        api.dense_inverse_blocks(A, 5, pairs=[(0, 13)])
    with pytest.raises(ValueError):
        api.dense_inverse_blocks(A, 5, pairs=[(-1, 0)])
    # the C entry point itself refuses the index too
    import ctypes
    r = np.array([13], np.int32)
    out = np.zeros((1, 5, 5), np.float32)
    info = ctypes.c_longlong(0)
    assert api.load_library().OptAMD_DenseInverseBlocks(65, A.ctypes.data, 5, 1, r.ctypes.data, r.ctypes.data,
                                                        out.ctypes.data, 0, ctypes.byref(info)) == -1


@pytest.mark.parametrize("dt", DTYPES, ids=("fp32", "fp64"))
def test_two_calls_agree_bitwise(dt):
    A = spd(200, dt)[0]
    pairs = [(e, e) for e in range(200)] + [(0, 199), (63, 64), (199, 3)]
    a, _ = api.dense_inverse_blocks(A, 1, pairs=pairs)
    b, _ = api.dense_inverse_blocks(A, 1, pairs=pairs)
    assert a.tobytes() == b.tobytes()
