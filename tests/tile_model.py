"""A numpy model of GxB_Matrix_concat / GxB_Matrix_split on tuples — the reference of tests/test_tile_host.py and tests/test_tile_gpu.py.

A matrix is `Mat(nrows, ncols, I, J, X)`: its tuples sorted by (row, column), X of the type's numpy dtype.
  concat  "add the origins, cast": every tuple (i, j, x) of tile (a, b) becomes (i + rowb[a], j + colb[b], cast(x)).
  split   "filter by range, subtract the origin": tile (a, b) holds the tuples with rowb[a] <= i < rowb[a + 1] and colb[b] <= j < colb[b + 1].
Casts are C casts (numpy `astype`; to BOOL: x != 0); the tests keep values inside the target type's range.  tests/test_tile_model.py pins both against
np.block and slicing of a dense value array plus a presence array.
"""
from collections import namedtuple

import numpy as np

Mat = namedtuple("Mat", "nrows ncols I J X")


def cast(x, dtype):
    x = np.asarray(x)
    return (x != 0) if np.dtype(dtype) == np.bool_ else x.astype(dtype)


def make(nrows, ncols, I, J, X):
    """Tuples in any order -> a Mat (sorted by row, then column)."""
    I, J, X = np.asarray(I, np.uint64), np.asarray(J, np.uint64), np.asarray(X)
    order = np.lexsort((J, I))
    return Mat(int(nrows), int(ncols), I[order], J[order], X[order])


def bounds(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def concat(tiles, dtype):
    """tiles: a list of rows of Mat.  The caller passes a grid whose shapes conform."""
    rowb, colb = bounds([row[0].nrows for row in tiles]), bounds([t.ncols for t in tiles[0]])
    Is, Js, Xs = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)], [np.zeros(0, dtype)]
    for a, row in enumerate(tiles):
        for b, t in enumerate(row):
            assert t.nrows == rowb[a + 1] - rowb[a] and t.ncols == colb[b + 1] - colb[b]
            Is.append(t.I + np.uint64(rowb[a])); Js.append(t.J + np.uint64(colb[b])); Xs.append(cast(t.X, dtype))
    return make(rowb[-1], colb[-1], np.concatenate(Is), np.concatenate(Js), np.concatenate(Xs))


def split(A, row_sizes, col_sizes):
    rowb, colb = bounds(row_sizes), bounds(col_sizes)
    assert rowb[-1] == A.nrows and colb[-1] == A.ncols
    I, J = A.I.astype(np.int64), A.J.astype(np.int64)
    out = []
    for a in range(len(row_sizes)):
        row = []
        for b in range(len(col_sizes)):
            keep = (I >= rowb[a]) & (I < rowb[a + 1]) & (J >= colb[b]) & (J < colb[b + 1])
            row.append(Mat(int(row_sizes[a]), int(col_sizes[b]), (I[keep] - rowb[a]).astype(np.uint64), (J[keep] - colb[b]).astype(np.uint64), A.X[keep]))
        out.append(row)
    return out


def csr(A):
    """(rowptr, col, val) of a Mat: what the library's CSR image holds."""
    rp = np.zeros(A.nrows + 1, np.int64)
    np.cumsum(np.bincount(A.I.astype(np.int64), minlength=A.nrows), out=rp[1:])
    return rp, A.J.astype(np.int64), A.X


def to_dense(A):
    V, P = np.zeros((A.nrows, A.ncols), A.X.dtype), np.zeros((A.nrows, A.ncols), np.bool_)
    V[A.I.astype(np.int64), A.J.astype(np.int64)] = A.X
    P[A.I.astype(np.int64), A.J.astype(np.int64)] = True
    return V, P


def from_dense(V, P):
    I, J = np.nonzero(P)
    return make(V.shape[0], V.shape[1], I, J, V[I, J])


def same(A, B):
    """Bit for bit: shape, pattern, dtype and the values' bytes."""
    return (A.nrows == B.nrows and A.ncols == B.ncols and np.array_equal(A.I, B.I) and np.array_equal(A.J, B.J)
            and A.X.dtype == B.X.dtype and A.X.tobytes() == B.X.tobytes())


def random_mat(rng, nrows, ncols, density, dtype, lo=-100, hi=100):
    """A random Mat: each position present with probability `density`; small integers as values (exact in every type; BOOL: 0 / 1)."""
    P = rng.random((nrows, ncols)) < density
    I, J = np.nonzero(P)
    if np.dtype(dtype) == np.bool_:
        X = rng.integers(0, 2, len(I)).astype(np.bool_)
    elif np.dtype(dtype).kind == "u":
        X = rng.integers(0, hi, len(I)).astype(dtype)
    else:
        X = rng.integers(lo, hi, len(I)).astype(dtype)
    return make(nrows, ncols, I, J, X)
