"""A vectorised model of the matrix companion operations (test infrastructure), numpy only and independent of the library: what the C API 1.3 says
transpose / eWiseAdd / eWiseMult / apply / apply with a bound scalar / select / reduce to a vector and the write-back `C<M, replace> = accum(C, T)` do to
stored entries.  A matrix is its sorted (row, column) keys, `key = i * ncols + j` in int64, and one value per key; every operation is a set operation on
the keys (union1d / intersect1d / searchsorted / isin) and an element-wise numpy expression on the values, so a 70 x 60 000 shape costs what its entries
cost and no dense array is ever formed.

The rules that are not plain numpy:
  * arithmetic runs in the numpy dtype of the operator's type under errstate(over="ignore"): C integer wrap-around; typecasts are `astype`;
  * integer DIV truncates toward zero (no zero divisors reach it); floating-point MIN / MAX are fmin / fmax;
  * the BOOL column renames arithmetic to logic: PLUS = MAX = LOR, TIMES = MIN = LAND, MINUS = LXOR, DIV = FIRST, AINV = ABS = IDENTITY;
  * a mask entry is true when it is stored and its value != 0 (so -0.0 is false and NaN is true), or when it is stored and the mask is structural.

tests/test_matrix_model.py pins it to a dictionary transcription of the same rules and to the reference's own vectors; tests/test_matrix_kernels_at_size_gpu.py
compares the HIP kernels with it at sizes that span many workgroups."""
import numpy as np

NP = {"BOOL": np.bool_, "INT8": np.int8, "UINT8": np.uint8, "INT16": np.int16, "UINT16": np.uint16, "INT32": np.int32, "UINT32": np.uint32,
      "INT64": np.int64, "UINT64": np.uint64, "FP32": np.float32, "FP64": np.float64}
NAME = {np.dtype(v): k for k, v in NP.items()}
BOOL_RENAME = {"PLUS": "LOR", "MAX": "LOR", "TIMES": "LAND", "MIN": "LAND", "MINUS": "LXOR", "DIV": "FIRST", "AINV": "IDENTITY", "ABS": "IDENTITY"}


class Mat:
    """nrows x ncols, the stored entries as ascending int64 keys i * ncols + j and their values."""

    def __init__(self, nrows, ncols, keys, vals):
        self.nrows, self.ncols = int(nrows), int(ncols)
        self.keys = np.asarray(keys, np.int64); self.vals = np.asarray(vals)
        assert self.keys.shape == self.vals.shape and self.keys.ndim == 1
        assert len(self.keys) == 0 or (np.all(np.diff(self.keys) > 0) and 0 <= self.keys[0] and self.keys[-1] < self.nrows * self.ncols)

    @property
    def typ(self): return NAME[self.vals.dtype]
    @property
    def nvals(self): return len(self.keys)
    @property
    def rows(self): return self.keys // max(self.ncols, 1)
    @property
    def cols(self): return self.keys % max(self.ncols, 1)

    def cast(self, typ):
        return Mat(self.nrows, self.ncols, self.keys, cast(self.vals, typ))


def from_coo(nrows, ncols, I, J, X, typ=None):
    """Entries in any order, no duplicates."""
    X = np.asarray(X) if typ is None else np.asarray(X, NP[typ])
    k = np.asarray(I, np.int64) * np.int64(ncols) + np.asarray(J, np.int64)
    o = np.argsort(k, kind="stable")
    return Mat(nrows, ncols, k[o], X[o])


def empty(nrows, ncols, typ):
    return Mat(nrows, ncols, np.zeros(0, np.int64), np.zeros(0, NP[typ]))


def to_csr(m):
    """(row pointers, columns, values) as the library exports them: uint32 indices, columns ascending inside each row."""
    rp = np.zeros(m.nrows + 1, np.int64)
    np.cumsum(np.bincount(m.rows, minlength=m.nrows), out=rp[1:])
    return rp.astype(np.uint32), m.cols.astype(np.uint32), m.vals


def cast(x, typ):
    with np.errstate(all="ignore"):
        return np.asarray(x).astype(NP[typ])


# ---- operators ----------------------------------------------------------------------------------------------------------------------------------------
def _idiv(a, b):
    if a.dtype.kind == "u":
        return a // b
    q = (np.abs(a.astype(np.float64)) // np.abs(b.astype(np.float64))) if a.dtype.itemsize < 8 else None
    if q is not None:                                         # (exact: fewer than 53 bits)
        return np.where((a < 0) != (b < 0), -q, q).astype(a.dtype)
    f = a // b                                                # floor division; one up where it rounded away from zero
    return f + ((a % b != 0) & ((a < 0) != (b < 0))).astype(a.dtype)


def binop(op, typ, a, b):
    """z = op(a, b) element-wise: both operands cast into the operator's type `typ`, the result of that type."""
    a, b = cast(a, typ), cast(b, typ)
    if typ == "BOOL":
        op = BOOL_RENAME.get(op, op)
    fp = typ.startswith("FP")
    with np.errstate(all="ignore"):
        if op == "FIRST": r = a
        elif op == "SECOND": r = b
        elif op == "PLUS": r = a + b
        elif op == "MINUS": r = a - b
        elif op == "TIMES": r = a * b
        elif op == "MIN": r = np.fmin(a, b) if fp else np.minimum(a, b)
        elif op == "MAX": r = np.fmax(a, b) if fp else np.maximum(a, b)
        elif op == "DIV": r = a / b if fp else _idiv(a, b)
        elif op == "POW" and fp: r = np.power(a, b)
        elif op == "LOR": r = (a != 0) | (b != 0)
        elif op == "LAND": r = (a != 0) & (b != 0)
        elif op == "LXOR": r = (a != 0) ^ (b != 0)
        elif op in ("EQ", "LXNOR") and typ == "BOOL": r = a == b
        elif op == "ISEQ": r = a == b                             # (the IS* comparisons answer 0 / 1 in the operands' type)
        elif op == "ISGT": r = a > b
        elif op == "ISLT": r = a < b
        elif op == "BOR" and not fp: r = a | b
        elif op == "BAND" and not fp: r = a & b
        elif op == "BXOR" and not fp: r = a ^ b
        elif op == "BXNOR" and not fp: r = ~(a ^ b)
        else: raise ValueError(op)
        return np.asarray(r).astype(NP[typ])


def unop(op, typ, a):
    a = cast(a, typ)
    if typ == "BOOL":
        op = BOOL_RENAME.get(op, op)
    with np.errstate(all="ignore"):
        if op == "IDENTITY": r = a
        elif op == "AINV": r = np.negative(a)
        elif op == "ABS": r = a if a.dtype.kind == "u" else np.abs(a)
        elif op == "ONE": r = np.ones_like(a)
        elif op == "MINV" and typ.startswith("FP"): r = 1.0 / a
        else: raise ValueError(op)
        return np.asarray(r).astype(NP[typ])


# ---- operations: each returns T, the result before the write-back --------------------------------------------------------------------------------------
def transpose(m):
    k = m.cols * np.int64(m.nrows) + m.rows
    o = np.argsort(k, kind="stable")
    return Mat(m.ncols, m.nrows, k[o], m.vals[o])


def ewise(op, typ, a, b, union):
    """eWiseAdd (`union`) / eWiseMult of two matrices of one shape with the operator `op` of type `typ`: where both have an entry op(a, b), in that order;
    in a union an entry of one operand alone passes through, cast to the operator's type."""
    assert (a.nrows, a.ncols) == (b.nrows, b.ncols)
    both, ia, ib = np.intersect1d(a.keys, b.keys, assume_unique=True, return_indices=True)
    zboth = binop(op, typ, a.vals[ia], b.vals[ib])
    if not union:
        return Mat(a.nrows, a.ncols, both, zboth)
    keys = np.union1d(a.keys, b.keys)
    vals = np.zeros(len(keys), NP[typ])
    vals[np.searchsorted(keys, a.keys)] = cast(a.vals, typ)
    only_b = ~np.isin(b.keys, a.keys, assume_unique=True)
    vals[np.searchsorted(keys, b.keys[only_b])] = cast(b.vals[only_b], typ)
    vals[np.searchsorted(keys, both)] = zboth
    return Mat(a.nrows, a.ncols, keys, vals)


def apply(op, typ, m):
    return Mat(m.nrows, m.ncols, m.keys, unop(op, typ, m.vals))


def bind1st(op, typ, scalar, m):
    """op(scalar, A(i, j))."""
    return Mat(m.nrows, m.ncols, m.keys, binop(op, typ, np.full(m.nvals, scalar, NP[typ]), m.vals))


def bind2nd(op, typ, m, scalar):
    """op(A(i, j), scalar)."""
    return Mat(m.nrows, m.ncols, m.keys, binop(op, typ, m.vals, np.full(m.nvals, scalar, NP[typ])))


SELECT_NAMES = {"tril": "TRIL", "triu": "TRIU", "diag": "DIAG", "offdiag": "OFFDIAG", "nonzero": "NONZERO", "!=0": "NONZERO", "==0": "EQ_ZERO", ">0": "GT_ZERO",
                ">=0": "GE_ZERO", "<0": "LT_ZERO", "<=0": "LE_ZERO", "!=": "NE_THUNK", "==": "EQ_THUNK", ">": "GT_THUNK", ">=": "GE_THUNK", "<": "LT_THUNK",
                "<=": "LE_THUNK"}


def select(sel, thunk, m):
    """The entries the select operator keeps, values untouched.  Positional operators compare the diagonal index j - i with the thunk (none: 0);
    value operators compare in the matrix's own type, the thunk cast into it."""
    sel = SELECT_NAMES.get(sel, sel)
    if sel in ("TRIL", "TRIU", "DIAG", "OFFDIAG"):
        d = m.cols - m.rows; k = np.int64(0 if thunk is None else thunk)
        keep = {"TRIL": d <= k, "TRIU": d >= k, "DIAG": d == k, "OFFDIAG": d != k}[sel]
    else:
        x = m.vals
        t = np.zeros(1, x.dtype)[0] if (thunk is None or sel.endswith("_ZERO") or sel == "NONZERO") else np.asarray(thunk).astype(x.dtype)
        if x.dtype == np.bool_:
            x = x.astype(np.uint8); t = np.uint8(t)
        with np.errstate(invalid="ignore"):
            keep = {"NONZERO": x != t, "NE": x != t, "EQ": x == t, "GT": x > t, "GE": x >= t, "LT": x < t, "LE": x <= t}[sel if sel == "NONZERO" else sel[:2]]
    return Mat(m.nrows, m.ncols, m.keys[keep], m.vals[keep])


_REDUCE = {"PLUS": np.add, "TIMES": np.multiply, "MIN": np.minimum, "MAX": np.maximum, "LOR": np.logical_or, "LAND": np.logical_and, "LXOR": np.logical_xor}
_REDUCE_FP = {"MIN": np.fmin, "MAX": np.fmax}


def reduce_rows(monoid, typ, m):
    """Every non-empty row folded with the monoid of type `typ`: an nrows x 1 Mat (a vector: key = row)."""
    if typ == "BOOL":
        monoid = BOOL_RENAME.get(monoid, monoid)
    x = cast(m.vals, typ); r = m.rows
    if not len(r):
        return empty(m.nrows, 1, typ)
    starts = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1])))
    uf = _REDUCE_FP.get(monoid, _REDUCE[monoid]) if typ.startswith("FP") else _REDUCE[monoid]
    with np.errstate(all="ignore"):
        z = uf.reduceat(x, starts, dtype=x.dtype)
    return Mat(m.nrows, 1, r[starts], z.astype(NP[typ]))


# ---- the write-back ------------------------------------------------------------------------------------------------------------------------------------
def mask_truth(vals):
    """The truth of stored mask values: != 0 (-0.0 is false, NaN is true)."""
    return np.asarray(vals) != 0


def mask_allows(mask, struct, comp, keys):
    """For each key: does the mask (None: no mask) let the position be written?"""
    if mask is None:
        return np.full(len(keys), not comp)
    pos = np.searchsorted(mask.keys, keys)
    stored = np.zeros(len(keys), bool)
    inside = pos < mask.nvals
    stored[inside] = mask.keys[pos[inside]] == keys[inside]
    truth = stored.copy()
    if not struct:
        truth[stored] = mask_truth(mask.vals[pos[stored]])
    return truth != comp


def write_back(C, T, mask=None, struct=False, comp=False, replace=False, accum=None):
    """C<M, replace> = accum(C, T), C API 1.3 section 3.5.4 and the operations' own last two steps: Z = T, or accum(C, T) on the union of the two patterns in
    the accumulator's type (`accum` = (operator, type) or None); Z is cast to C's type; where the mask allows, C takes Z's entry or loses its own; where it
    does not, C keeps its entry, unless `replace` deletes it.  The mask and T have C's shape.  Returns the new C."""
    assert (C.nrows, C.ncols) == (T.nrows, T.ncols) and (mask is None or (mask.nrows, mask.ncols) == (C.nrows, C.ncols))
    Z = T if accum is None else ewise(accum[0], accum[1], C, T, True)
    Z = Z.cast(C.typ)
    za = mask_allows(mask, struct, comp, Z.keys)
    keys, vals = Z.keys[za], Z.vals[za]
    if not replace:
        ck = ~mask_allows(mask, struct, comp, C.keys)
        keys = np.concatenate([keys, C.keys[ck]]); vals = np.concatenate([vals, C.vals[ck]])
        o = np.argsort(keys, kind="stable"); keys, vals = keys[o], vals[o]
    return Mat(C.nrows, C.ncols, keys, vals)
