"""A numpy model of GrB_Matrix_build / GrB_Vector_build: the tuples sorted by their packed key with a STABLE sort, runs of equal keys found with
np.flatnonzero, every run folded LEFT TO RIGHT IN INPUT ORDER with the operator table of tests/operator_model.py —
z = dup(dup(dup(x0, x1), x2), ...).  Where the operator model accepts more than one result (ANY; MIN / MAX of +0.0 and -0.0) the model takes the first one
listed, which is what the library's host route returns (ANY is SECOND there).  Pinned against the host route in tests/test_build_model.py; the device route is
compared with both in tests/test_build_gpu.py."""
import numpy as np

import operator_model as om

OUT_OF_BOUNDS, DUPLICATE = "INDEX_OUT_OF_BOUNDS", "INVALID_VALUE"


def bits(dim):
    """bits(dim - 1): what an index below dim needs (grb_build_keys.hpp: build_bits)."""
    return int(dim - 1).bit_length() if dim > 1 else 0


def _scalar(t, v):
    if t == "BOOL": return bool(v)
    if om.is_fp(t): return om.NP[t](v)
    return int(v)


def fold(t, op, values):
    """The left fold of a run, in the order given."""
    z = _scalar(t, values[0])
    for v in values[1:]:
        z = om.binop(op, t, z, _scalar(t, v))[0]
    return z


def build(t, I, J, X, nrows, ncols, op):
    """(rows, cols, vals) of the built container in (row, column) order — cols is None for a vector (J is None) — or OUT_OF_BOUNDS / DUPLICATE, in
    that order of precedence.  I, J: uint64 arrays; X: an array of the type's numpy dtype; op: an operator name or None."""
    I = np.asarray(I, np.uint64); n = len(I)
    J = None if J is None else np.asarray(J, np.uint64)
    X = np.asarray(X, om.NP[t])
    if np.any(I >= np.uint64(nrows)) or (J is not None and np.any(J >= np.uint64(ncols))):
        return OUT_OF_BOUNDS
    cbits = bits(ncols) if J is not None else 0
    key = (I << np.uint64(cbits)) | (J if J is not None else np.uint64(0))      # exact in 64 bits: device dimensions need at most 32 bits each
    order = np.argsort(key, kind="stable")
    skey = key[order]
    heads = np.flatnonzero(np.concatenate([[True], skey[1:] != skey[:-1]])) if n else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64) if n else heads
    if op is None and np.any(ends - heads > 1):
        return DUPLICATE
    vals = X[order[heads]].copy() if n else X[:0].copy()
    for r in np.flatnonzero(ends - heads > 1):
        z = fold(t, op, X[order[heads[r]:ends[r]]])
        vals[r] = z
    rows = I[order[heads]] if n else I[:0]
    cols = None if J is None else (J[order[heads]] if n else J[:0])
    return rows, cols, vals


def rowptr(rows, nrows):
    """The CSR row pointer of a sorted row list, as uint32."""
    return np.concatenate([[0], np.cumsum(np.bincount(rows.astype(np.int64), minlength=nrows))]).astype(np.uint32) if nrows else np.zeros(1, np.uint32)
