"""A numpy model of GxB_Matrix_sort / GxB_Vector_sort / GrBX_*_select_topk: the yardstick of the sort tests (the reference package has no sort).

The order is total: primary "is NaN" (NaNs after every number, under LT and GT alike, all tied), then the dense rank of the value (np.unique: -0.0 and 0.0
share one rank), negated for GT — ranks are negated, never values, so UINT64 and the INT64 minimum survive — then the original index.  np.lexsort does it in
one call, with the line (row or column) as the outermost key for matrices.  Pinned by tests/test_sort_model.py on cases worked out by hand."""
import numpy as np


def cast(x, dtype):
    """The library's cast rule: anything -> BOOL is x != 0; floating point -> integer truncates toward zero, saturates, NaN -> 0; the rest is the C cast."""
    x = np.asarray(x)
    dtype = np.dtype(dtype)
    if dtype == x.dtype:
        return x
    if dtype == np.bool_:
        return x != 0
    if x.dtype.kind == "f" and dtype.kind in "iu":
        info = np.iinfo(dtype)
        y = np.where(np.isnan(x), 0.0, np.trunc(x.astype(np.float64)))
        out = np.clip(y, float(info.min), float(info.max))
        res = np.zeros(len(x), dtype)
        hi, lo = y >= float(info.max), y <= float(info.min)
        mid = ~(hi | lo)
        res[mid] = out[mid].astype(dtype)
        res[hi], res[lo] = info.max, info.min
        return res
    return x.astype(dtype)


def _rank_keys(values, gt):
    v = np.asarray(values)
    isnan = np.isnan(v) if v.dtype.kind == "f" else np.zeros(len(v), bool)
    clean = np.where(isnan, 0, v) if v.dtype.kind == "f" else v
    _, rank = np.unique(clean, return_inverse=True)
    rank = rank.astype(np.int64).reshape(-1)
    return isnan, (-rank if gt else rank)


def order(values, index, gt=False, line=None):
    """The places of `values` in sorted order; `index` the original indices (ties), `line` the row / column each belongs to (outermost key)."""
    isnan, rank = _rank_keys(values, gt)
    keys = (np.asarray(index), rank, isnan) + ((np.asarray(line),) if line is not None else ())
    return np.lexsort(keys)


def _lines(I, J, X, gt, by_col, key_dtype):
    """perm (places in sorted order, grouped by line), the line of each, and its rank q within the line."""
    I, J, X = np.asarray(I, np.uint64), np.asarray(J, np.uint64), np.asarray(X)
    line, idx = (J, I) if by_col else (I, J)
    keyvals = cast(X, key_dtype) if key_dtype is not None else X
    perm = order(keyvals, idx, gt, line)
    ln = line[perm]
    start = np.flatnonzero(np.r_[True, ln[1:] != ln[:-1]]) if len(ln) else np.zeros(0, np.int64)
    counts = np.diff(np.r_[start, len(ln)])
    q = np.arange(len(ln)) - np.repeat(start, counts)
    return perm, ln, q.astype(np.uint64), idx


def _row_major(i, j, *arrays):
    o = np.lexsort((j, i))
    return (i[o], j[o]) + tuple(a[o] for a in arrays)


def matrix_sort(I, J, X, gt=False, by_col=False, key_dtype=None):
    """(Ci, Cj, Cx, Px) in row-major order: the tuples of C, and the values of P at the same coordinates."""
    perm, ln, q, idx = _lines(I, J, X, gt, by_col, key_dtype)
    X = np.asarray(X)
    ci, cj = (q, ln) if by_col else (ln, q)
    return _row_major(ci, cj, X[perm], idx[perm].astype(np.int64))


def matrix_topk(I, J, X, k, gt=True, by_col=False, key_dtype=None):
    """(I, J, X) of the first min(k, len) entries of every line, in row-major order."""
    perm, ln, q, idx = _lines(I, J, X, gt, by_col, key_dtype)
    keep = perm[q < np.uint64(min(k, 1 << 62))]
    I, J, X = np.asarray(I, np.uint64), np.asarray(J, np.uint64), np.asarray(X)
    return _row_major(I[keep], J[keep], X[keep])


def vector_sort(idx, X, gt=False, key_dtype=None):
    """(wx, px): the values in sorted order and the index each came from; both live at positions 0 .. nvals - 1."""
    idx, X = np.asarray(idx, np.uint64), np.asarray(X)
    perm = order(cast(X, key_dtype) if key_dtype is not None else X, idx, gt)
    return X[perm], idx[perm].astype(np.int64)


def vector_topk(idx, X, k, gt=True, key_dtype=None):
    idx, X = np.asarray(idx, np.uint64), np.asarray(X)
    perm = order(cast(X, key_dtype) if key_dtype is not None else X, idx, gt)
    keep = np.sort(perm[:k])
    return idx[keep], X[keep]


def bits(x):
    """Values as unsigned words of their size: the exact comparison (NaN payloads and the sign of zero included)."""
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
