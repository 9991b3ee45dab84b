"""The n x n x n 7-point stencil for the tests of "stencil7-csr" (tests/test_stencil7_host.py, tests/test_stencil7_gpu.py): its COO
entries in the writer's order, built with numpy. Point (k, i, j) is row k n^2 + i n + j; neighbours at -+1 (W/E), -+n (N/S),
-+n^2 (D/U) where they exist. Test infrastructure."""
import numpy as np

from matrices import ENTRY_DTYPE


def coo(n, center=7.0, off=-1.0, rng=None):
    """Entries of one grid point in the order C, W, E, N, S, D, U (write_matrix_market_stencil7's), points in row order.
    rng: every value is drawn from it instead (uniform in [-3, 3): unsymmetric on purpose)."""
    N = n * n * n
    r = np.arange(N, dtype=np.int64)
    k, rest = np.divmod(r, n * n)
    i, j = np.divmod(rest, n)
    steps = [(0, np.ones(N, dtype=bool)), (-1, j > 0), (1, j < n - 1), (-n, i > 0), (n, i < n - 1), (-n * n, k > 0), (n * n, k < n - 1)]
    present = np.stack([ok for _, ok in steps], axis=1)              # (N, 7) in the writer's order
    cols = np.stack([r + d for d, _ in steps], axis=1)
    rows = np.broadcast_to(r[:, None], cols.shape)
    vals = np.full(cols.shape, off)
    vals[:, 0] = center
    e = np.zeros(int(present.sum()), dtype=ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = rows[present], cols[present], vals[present]
    if rng is not None:
        e["value"] = rng.uniform(-3.0, 3.0, len(e))
    return e


def nnz(n):
    return 7 * n ** 3 - 6 * n ** 2


def spd_coo(n, rng, decades=2.0):
    """Symmetric positive definite by construction: one off-diagonal value in [-1, 0) per undirected edge, diagonal 1 + sum |off|
    (strictly diagonally dominant), then S A S with a diagonal S spread over `decades` decades (a congruence: still SPD)."""
    e = coo(n)
    row, col = e["row"].astype(np.int64), e["col"].astype(np.int64)
    N = n ** 3
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    edge = lo * N + hi
    uniq, inv = np.unique(edge[row != col], return_inverse=True)
    w = -rng.uniform(1e-3, 1.0, len(uniq))
    val = np.zeros(len(e))
    val[row != col] = w[inv]
    diag = 1.0 + np.bincount(row[row != col], weights=-val[row != col], minlength=N)
    val[row == col] = diag[row[row == col]]
    s = 10.0 ** (0.5 * decades * rng.uniform(0.0, 1.0, N))
    e["value"] = s[row] * val * s[col]
    return e
