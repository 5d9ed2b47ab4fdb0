"""A vectorised numpy model of the matrix-vector products (test infrastructure), independent of the library: `t = M (+).(x) u` for a CSR matrix (a
matrix_model.Mat: sorted keys, one value per key) and a bitmap operand (a vector_model.Vec: values plus presence), then `w<mask, replace> = accum(w, t)`.
Operators, typecasts, the row fold, the truth of a mask value and the write-back are those of tests/matrix_model.py and tests/vector_model.py (`binop`, `cast`,
`reduce_rows`, `mask_truth` through `write_back`); this file adds what a product is about:
  * an entry M(i, j) contributes mult(M(i, j), u(j)) only where u has an entry at j; a row all of whose contributions are absent has no entry in t;
  * both operands are cast into the semiring's type; `flip` hands the multiplier its arguments the other way round (u(j) first: the order of GrB_vxm);
  * PAIR is 1 and RDIV is DIV the other way round; the monoids beside matrix_model's folds: ANY keeps the contribution with the largest column (what the
    sequential oracle does: its ANY is SECOND), EQ / LXNOR is true iff an even number of contributions is false;
  * `mxv(w, A, u)` is `w = A u` (desc T0: A transposed), `vxm(w, u, A)` is `w' = u' A`, i.e. `A' u` with the multiplier's arguments flipped (desc T1: A).
  * `masked_mxm` / `mxm` are the matrix product `C<M> = accum(C, A (+).(x) B)` on the same rules: the products expanded, pruned by the true mask entries,
    folded per (i, j) in ascending k (tests/test_spgemm_masked_at_size_gpu.py compares the masked SpGEMM kernels with it).
A product over 10^6 rows costs a few passes over the entries; the oracle (oracle/grb_oracle.c, through sorted n x 1 matrices) is what
tests/test_product_model.py pins this file to, on small cases."""
import numpy as np

import matrix_model as MM
import vector_model as VM

NP = MM.NP


def mult(op, typ, a, b):
    """mult(a, b) element-wise in the semiring's type."""
    if op == "PAIR":
        return np.ones(len(a), NP[typ])
    if op == "RDIV":
        return MM.binop("DIV", typ, b, a)
    return MM.binop(op, typ, a, b)


def fold_rows(monoid, typ, m):
    """Every non-empty row of `m` folded with the monoid: (rows, values)."""
    if typ == "BOOL":
        monoid = MM.BOOL_RENAME.get(monoid, monoid)
    if not m.nvals:
        return np.zeros(0, np.int64), np.zeros(0, NP[typ])
    if monoid == "ANY":
        r = m.rows; last = np.flatnonzero(np.concatenate((r[1:] != r[:-1], [True])))
        return r[last], MM.cast(m.vals[last], typ)
    if monoid in ("EQ", "LXNOR"):
        odd = MM.reduce_rows("LXOR", "BOOL", MM.Mat(m.nrows, m.ncols, m.keys, ~MM.cast(m.vals, "BOOL")))
        return odd.keys, ~odd.vals
    t = MM.reduce_rows(monoid, typ, m)
    return t.keys, t.vals


def product(add, mul, typ, M, u, allow=None, flip=False):
    """t = M (+).(x) u as a Vec of the semiring's type over M's rows; `allow` (one bool per row, or None) leaves the rows it rejects without an entry."""
    assert M.ncols == u.n and (allow is None or len(allow) == M.nrows)
    rows, cols = M.rows, M.cols
    live = u.pres[cols] if allow is None else u.pres[cols] & np.asarray(allow, bool)[rows]
    a, b = M.vals[live], u.val[cols[live]]
    z = mult(mul, typ, b, a) if flip else mult(mul, typ, a, b)
    at, x = fold_rows(add, typ, MM.Mat(M.nrows, M.ncols, M.keys[live], z))
    t = VM.empty(M.nrows, typ)
    t.val[at] = x; t.pres[at] = True
    return t


# the types, mask types and semirings the masked-product tests run (the CPU pin of the model and the GPU file share them)
MXM_TYPES = ["BOOL", "INT8", "UINT16", "INT32", "FP32", "INT64", "FP64"]
MXM_MASK_TYPES = ["BOOL", "INT8", "UINT16", "FP32", "INT64", "FP64"]


def mxm_semirings(typ):
    """PLUS_TIMES, PLUS_PAIR, MIN_PLUS, a monoid without a native atomic (TIMES over floating point rounds, so there it is MAX), and MAX_FIRST."""
    if typ == "BOOL": return ["LOR_LAND", "LXOR_LAND"]
    return ["PLUS_TIMES", "PLUS_PAIR", "MIN_PLUS", "MAX_PLUS" if typ.startswith("FP") else "TIMES_PLUS", "MAX_FIRST"]


def masked_mxm(add, mul, typ, A, B, M, struct=False):
    """T<M> = A (+).(x) B before the write-back, as a Mat of the semiring's type: the products of every entry A(i, k) with row B(k, :), expanded with np.repeat
    in (i, k, j) order; those whose key (i, j) is a true entry of M (`matrix_model.mask_truth`; `struct`: every stored entry; M None: all of them) are
    kept, sorted by key — stable, so by k inside a key — and folded with the monoid (`fold_rows`: its ANY keeps the largest k).  A mask entry that
    receives no product has no entry in T.  Both operands are cast into the semiring's type."""
    assert A.ncols == B.nrows and (M is None or (M.nrows, M.ncols) == (A.nrows, B.ncols))
    nc = np.int64(B.ncols)
    brp = np.searchsorted(B.keys, np.arange(B.nrows + 1, dtype=np.int64) * nc)        # row pointers of B
    cnt = (brp[1:] - brp[:-1])[A.cols]
    first = np.cumsum(cnt) - cnt
    pb = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first - brp[A.cols], cnt)   # the entry of B behind every product
    pa = np.repeat(np.arange(A.nvals, dtype=np.int64), cnt)
    key = np.repeat(A.rows, cnt) * nc + B.cols[pb]
    if M is not None:
        allowed = M.keys if struct else M.keys[MM.mask_truth(M.vals)]
        at = np.searchsorted(allowed, key)
        hit = np.zeros(len(key), bool); inside = at < len(allowed)
        hit[inside] = allowed[at[inside]] == key[inside]
        key, pa, pb = key[hit], pa[hit], pb[hit]
    o = np.argsort(key, kind="stable")
    key, z = key[o], mult(mul, typ, MM.cast(A.vals, typ)[pa[o]], MM.cast(B.vals, typ)[pb[o]])
    if not len(key):
        return MM.empty(A.nrows, B.ncols, typ)
    head = np.concatenate(([True], key[1:] != key[:-1]))
    group = np.cumsum(head) - 1; starts = np.flatnonzero(head)
    rank = np.arange(len(key), dtype=np.int64) - starts[group]                       # the products of one key as one row of a Mat, in k order
    width = np.int64(rank.max() + 1)
    at, x = fold_rows(add, typ, MM.Mat(len(starts), width, group * width + rank, z))
    assert np.array_equal(at, np.arange(len(starts)))
    return MM.Mat(A.nrows, B.ncols, key[starts], x)


def mxm(C, A, B, add, mul, typ, mask=None, struct=False, comp=False, replace=False, accum=None, tran_a=False, tran_b=False):
    """C<mask, replace> = accum(C, op(A) add.mul op(B)); a plain mask prunes the product (`masked_mxm`), a complemented one acts in the write-back alone."""
    A = MM.transpose(A) if tran_a else A; B = MM.transpose(B) if tran_b else B
    t = masked_mxm(add, mul, typ, A, B, None if comp else mask, struct)
    return MM.write_back(C, t, mask, struct, comp, replace, accum)


def mxv(w, A, u, add, mul, typ, mask=None, struct=False, comp=False, replace=False, accum=None, tran=False):
    """w<mask, replace> = accum(w, op(A) add.mul u); `tran`: desc INP0; `accum` = (operator, type) or None."""
    t = product(add, mul, typ, MM.transpose(A) if tran else A, u)
    return VM.write_back(w, t, mask, struct, comp, replace, accum)


def vxm(w, u, A, add, mul, typ, mask=None, struct=False, comp=False, replace=False, accum=None, tran=False):
    """w'<mask', replace> = accum(w', u' add.mul op(A)); `tran`: desc INP1.  The multiplier sees u(i) first."""
    t = product(add, mul, typ, A if tran else MM.transpose(A), u, flip=True)
    return VM.write_back(w, t, mask, struct, comp, replace, accum)
