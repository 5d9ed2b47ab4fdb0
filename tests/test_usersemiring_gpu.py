"""User-defined monoids and semirings on the device (GrBX_Monoid_new_user / GrBX_Semiring_new_user, `T.new_monoid` / `T.new_semiring`): GrB_mxm, GrB_mxv, GrB_vxm
and the matrix-to-vector reduction through the two compiled kernels of pygraphblas_amd/csrc/grb_usersr.cpp.

Where a user-defined semiring spells a built-in one in exact arithmetic the results must be the built-in call's bits, under every mask form, replace, a built-in
accumulator and transposed inputs; the product is also checked against a sequential model (every entry the left-to-right sum of its products in ascending k, the
write-back that of tests/matrix_model.py).  The two semantic rules have tests of their own: the monoid's identity is never combined into a result, and the
multiplier's argument order is mul(A(i,k), B(k,j)) for mxv / mxm and mul(u(i), A(i,j)) for vxm.

Shapes: a 300-row matrix whose row lengths include 0, 1, 63, 64, 65 and 200 (the lane stride of 64 and the wave tree), an operand vector with holes, an empty one, a
matrix without entries; for the product 200 x 150 times 150 x 180 with ~3 000 entries each, one row of A with 130 entries reaching rows of B whose supports (20 consecutive columns) shift by
one column from one to the next (the same output column falls on the neighbouring lane at successive k), and output rows on both sides of the 128 entries whose
accumulators live in LDS."""
import ctypes as C
import json
import os
import subprocess
import sys
from math import exp, log1p

import numpy as np
import pytest

import matrix_model as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPT = {"INT64": np.int64, "INT32": np.int32, "UINT8": np.uint8, "FP64": np.float64, "FP32": np.float32}


# ---- the operators (module level: their source must be readable) -----------------------------------------------------------------------------------------------
def u_add(x, y):
    return x + y


def u_mul(x, y):
    return x * y


def u_max(x, y):
    return max(x, y)


def u_order(x, y):
    return x * 4 + y


def log_plus(x, y):
    return x + log1p(exp(y - x))


def log_times(x, y):
    return x + y


# ---- data -------------------------------------------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 63, 64, 65, 200]


def rows_matrix(rng, typ, n=300):
    """n x n; rows 0..5 have 0, 1, 63, 64, 65, 200 entries, the others 0..8."""
    I, J = [], []
    for i in range(n):
        k = ROW_LENGTHS[i] if i < len(ROW_LENGTHS) else int(rng.integers(0, 9))
        c = np.sort(rng.choice(n, size=k, replace=False))
        I += [i] * k; J += c.tolist()
    return np.array(I, np.uint64), np.array(J, np.uint64), values(rng, typ, len(I))


def values(rng, typ, k):
    if typ == "UINT8":
        return rng.integers(0, 256, k).astype(np.uint8)                      # products and sums wrap
    if typ.startswith("FP"):
        return (rng.integers(-64, 65, k) / 8.0).astype(NPT[typ])            # sums of these are exact
    return rng.integers(-9, 10, k).astype(NPT[typ])


def product_operands(rng, typ):
    """A 200 x 150, B 150 x 180.  Row 7 of A has 130 entries (columns 10..139); row k of B for those k holds the 20 consecutive columns k .. k + 19, its support
    shifted by one column from one k to the next: B(k,:) and B(k+1,:) share 19 columns, each at a rank one lower in the next row, so in output row 7 the same
    column is written by one lane at k and read and rewritten by its neighbour at k + 1 (`shifted_ranks` counts them).  Output row 7 has the 149 columns
    10..158 (> 128: the global-memory path).  The other rows of A have 0..30 entries, the other rows of B 0..40: short output rows (the LDS path) among longer."""
    ai, aj, bi, bj = [], [], [], []
    for i in range(200):
        c = np.arange(10, 140) if i == 7 else np.sort(rng.choice(150, size=int(rng.integers(0, 31)), replace=False))
        if i == 9:
            c = c[:0]
        ai += [i] * len(c); aj += c.tolist()
    for k in range(150):
        if 10 <= k < 140:
            c = np.unique((k + np.arange(20)) % 180)
        else:
            c = np.sort(rng.choice(180, size=int(rng.integers(0, 41)), replace=False))
        bi += [k] * len(c); bj += c.tolist()
    ai, aj, bi, bj = (np.array(x, np.uint64) for x in (ai, aj, bi, bj))
    return (ai, aj, values(rng, typ, len(ai))), (bi, bj, values(rng, typ, len(bi)))


def shifted_ranks(ca, cb, row=7):
    """How many (column, k) of output row `row` are produced at two successive positions of A(row,:) by entries of different rank in their rows of B — i.e.
    by different lanes of the wave at successive steps."""
    ks = ca[1][ca[0] == row].astype(np.int64)
    rank = {}
    for k in ks.tolist():
        for r, j in enumerate(cb[1][cb[0] == k].tolist()):
            rank[(k, j)] = r % 64
    n = 0
    for k, k2 in zip(ks[:-1].tolist(), ks[1:].tolist()):
        n += sum(1 for (kk, j), r in rank.items() if kk == k and (k2, j) in rank and rank[(k2, j)] != r)
    return n


def mat(gb, coo, nrows, ncols, typ):
    return gb.Matrix.from_arrays(coo[0], coo[1], coo[2], nrows, ncols, getattr(gb, typ))


def vec(gb, idx, x, n, typ):
    return gb.Vector.from_arrays(np.asarray(idx, np.uint64), np.asarray(x, NPT[typ]), n, getattr(gb, typ))


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def semirings(gb, form):
    """(user semiring, the built-in one it spells, user monoid, built-in monoid, type name) — the objects stay alive in the returned tuple."""
    if form in ("INT64", "INT32", "UINT8"):
        T = getattr(gb, form)
        add, mul = gb.binary_op(T)(u_add), gb.binary_op(T)(u_mul)
        mon = T.new_monoid(add, 0)
        return T.new_semiring(mon, mul), T.PLUS_TIMES, mon, T.PLUS_MONOID, form, (add, mul)
    if form == "FP64_MAX_PLUS":
        T = gb.FP64
        add, mul = gb.binary_op(T)(u_max), gb.binary_op(T)(u_add)
        mon = T.new_monoid(add, -np.inf)
        return T.new_semiring(mon, mul), T.MAX_PLUS, mon, T.MAX_MONOID, "FP64", (add, mul)
    T = gb.INT64
    if form == "user_add_builtin_mul":
        add = gb.binary_op(T)(u_add)
        mon = T.new_monoid(add, 0)
        return T.new_semiring(mon, T.TIMES), T.PLUS_TIMES, mon, T.PLUS_MONOID, "INT64", (add,)
    mul = gb.binary_op(T)(u_mul)
    return T.new_semiring(T.PLUS_MONOID, mul), T.PLUS_TIMES, None, T.PLUS_MONOID, "INT64", (mul,)


FORMS = ["INT64", "INT32", "UINT8", "FP64_MAX_PLUS", "user_add_builtin_mul", "builtin_add_user_mul"]


# ---- 1. the reference's log semiring ---------------------------------------------------------------------------------------------------------------------------
def test_reference_log_semiring(gb, gpu):
    with open(os.path.join(ROOT, "tests", "golden", "reference_log_semiring.json")) as f:
        g = json.load(f)

    class Log32(gb.FP32):
        PLUS = gb.binary_op(gb.FP32)(log_plus)
        TIMES = gb.binary_op(gb.FP32)(log_times)

    I, J, X = zip(*g["input"])
    A = gb.Matrix.from_arrays(np.array(I, np.uint64), np.array(J, np.uint64), np.log(np.array(X)).astype(np.float32), g["nrows"], g["ncols"], gb.FP32)
    monoid = Log32.new_monoid(Log32.PLUS, g["identity"])          # 1.0 = Log32.default_one, as the reference passes it: not the monoid's true identity (-inf)
    semiring = Log32.new_semiring(monoid, Log32.TIMES)
    with semiring:
        B = A @ A
    bi, bj, bx = B.to_arrays()
    ei, ej, ex = zip(*g["expected"])
    assert bi.tolist() == list(ei) and bj.tolist() == list(ej)
    err = np.abs(np.exp(bx.astype(np.float64)) - np.array(ex))
    print("log semiring: largest |exp(value) - expected| =", err.max())
    assert err.max() < g["tolerance_abs"]
    assert same_bits(semiring(A, A).to_arrays(), (bi, bj, bx))      # as a callable


# ---- 2. the same bits as the built-in semiring where arithmetic is exact -----------------------------------------------------------------------------------------
def vector_variants(gb, rng, n, typ):
    """(mask, accum, desc, non-empty output or None) for the vector operations."""
    D = gb.descriptor
    mask = vec(gb, np.arange(0, n, 2), rng.integers(0, 2, len(range(0, n, 2))), n, "INT32")      # half the positions, about half of them false
    T = getattr(gb, typ)
    w0 = (np.arange(1, n, 3), values(rng, typ, len(range(1, n, 3))))
    return [(None, None, None, None), (mask, None, None, None), (mask, None, D.C, None), (mask, None, D.S, None), (mask, None, D.R, w0), (mask, None, D.C & D.R, w0),
            (None, T.PLUS, None, w0), (mask, T.PLUS, D.S, w0)]


@pytest.mark.parametrize("form", FORMS)
def test_rows_kernel_equals_builtin(gb, gpu, form):
    usr, ref, umon, rmon, typ, _keep = semirings(gb, form)
    rng = np.random.default_rng(11)
    n = 300
    coo = rows_matrix(rng, typ, n)
    A = mat(gb, coo, n, n, typ)
    Z = gb.Matrix.sparse(getattr(gb, typ), n, n)                                               # no entries
    holes = np.array([i for i in range(n) if i % 3], np.uint64)
    operands = [vec(gb, holes, values(rng, typ, len(holes)), n, typ), vec(gb, np.arange(n), values(rng, typ, n), n, typ), gb.Vector.sparse(getattr(gb, typ), n)]
    D = gb.descriptor
    checked = 0
    for u in operands:
        for mask, accum, desc, w0 in vector_variants(gb, rng, n, typ):
            for M in (A, Z):
                outs = []
                for sr in (usr, ref):
                    r = []
                    for tr in (False, True):
                        for op in ("mxv", "vxm"):
                            out = vec(gb, w0[0], w0[1], n, typ) if w0 is not None else gb.Vector.sparse(getattr(gb, typ), n)
                            d = desc
                            if tr:
                                t = D.T0 if op == "mxv" else D.T1
                                d = t if d is None else d & t
                            if op == "mxv":
                                M.mxv(u, sr, out=out, mask=mask, accum=accum, desc=d)
                            else:
                                u.vxm(M, sr, out=out, mask=mask, accum=accum, desc=d)
                            r.append(out.to_arrays())
                    outs.append(r)
                for a, b in zip(*outs):
                    assert same_bits(a, b), (form, "vector product", mask is not None, accum, desc)
                    checked += 1
    assert checked > 100
    # the matrix-to-vector reduction with the user monoid (the mixed form with a built-in monoid has none)
    if umon is not None:
        for mask, accum, desc, w0 in vector_variants(gb, rng, n, typ):
            for tr in (False, True):
                d = desc if not tr else (D.T0 if desc is None else desc & D.T0)
                outs = []
                for mon in (umon, rmon):
                    out = vec(gb, w0[0], w0[1], n, typ) if w0 is not None else gb.Vector.sparse(getattr(gb, typ), n)
                    A.reduce_vector(mon, out=out, mask=mask, accum=accum, desc=d)
                    outs.append(out.to_arrays())
                assert same_bits(*outs), (form, "reduce_vector", mask is not None, accum, desc, tr)
        # against the model: the row sums of the matrix
        i, x = A.reduce_vector(umon).to_arrays()
        m = mm.reduce_rows("MAX" if form == "FP64_MAX_PLUS" else "PLUS", typ, mm.from_coo(n, n, coo[0], coo[1], coo[2]))
        assert np.array_equal(i, m.keys) and x.tobytes() == m.vals.tobytes()


def model_product(A, B, typ, add, mul):
    """T = A (+).(x) B over dict-of-rows operands: every entry the left-to-right sum of its products in ascending k, in the type's own arithmetic."""
    npt = NPT[typ]
    brow = {}
    for k, j, x in zip(*B):
        brow.setdefault(int(k), []).append((int(j), x))
    T = {}
    with np.errstate(over="ignore"):
        for i, k, a in zip(*A):                                                                   # (entries are in (row, column) order)
            for j, b in brow.get(int(k), ()):
                p = npt(mul(a, b)); key = (int(i), j)
                T[key] = npt(add(T[key], p)) if key in T else p
    keys = sorted(T)
    return keys, np.array([T[k] for k in keys], npt)


def mask_matrix(gb, rng, nrows, ncols):
    k = nrows * ncols // 3
    flat = np.sort(rng.choice(nrows * ncols, size=k, replace=False))
    return (flat // ncols).astype(np.uint64), (flat % ncols).astype(np.uint64), rng.integers(0, 2, k).astype(np.int32)


@pytest.mark.parametrize("form", FORMS)
def test_product_kernel_equals_builtin_and_model(gb, gpu, form):
    usr, ref, _umon, _rmon, typ, _keep = semirings(gb, form)
    rng = np.random.default_rng(5)
    ca, cb = product_operands(rng, typ)
    assert 2500 <= len(ca[0]) <= 4000 and 2500 <= len(cb[0]) <= 4000
    assert shifted_ranks(ca, cb) > 2000                         # the across-k hazard: in row 7 the same column falls on another lane at the next k
    A, B = mat(gb, ca, 200, 150, typ), mat(gb, cb, 150, 180, typ)
    T = getattr(gb, typ)
    D = gb.descriptor
    cm = mask_matrix(gb, rng, 200, 180)
    M = gb.Matrix.from_arrays(cm[0], cm[1], cm[2], 200, 180, gb.INT32)
    c0 = mask_matrix(gb, rng, 200, 180)
    c0 = (c0[0], c0[1], values(rng, typ, len(c0[0])))
    variants = [(None, None, None, False), (M, None, None, False), (M, None, D.C, False), (M, None, D.S, False), (M, None, D.R, True), (M, None, D.C & D.R, True),
                (None, T.PLUS, None, True), (M, T.PLUS, D.S, True)]
    add = (lambda x, y: max(x, y)) if form == "FP64_MAX_PLUS" else (lambda x, y: x + y)
    mul = (lambda x, y: x + y) if form == "FP64_MAX_PLUS" else (lambda x, y: x * y)
    keys, vals = model_product(ca, cb, typ, add, mul)
    assert max(sum(1 for k in keys if k[0] == i) for i in (7,)) > 128 and any(0 < sum(1 for k in keys if k[0] == i) <= 128 for i in range(200))      # both paths
    tm = mm.from_coo(200, 180, [k[0] for k in keys], [k[1] for k in keys], vals)
    for mask, accum, desc, filled in variants:
        outs = []
        for sr in (usr, ref):
            out = mat(gb, c0, 200, 180, typ) if filled else gb.Matrix.sparse(T, 200, 180)
            A.mxm(B, sr, out=out, mask=mask, accum=accum, desc=desc)
            outs.append(out.to_arrays())
        assert same_bits(*outs), (form, "mxm", mask is not None, accum, desc)
        # ... and the model: T through matrix_model's write-back
        cmod = mm.from_coo(200, 180, c0[0], c0[1], c0[2]) if filled else mm.empty(200, 180, typ)
        want = mm.write_back(cmod, tm, mask=None if mask is None else mm.from_coo(200, 180, cm[0], cm[1], cm[2]), struct=desc is not None and D.S in desc,
                             comp=desc is not None and D.C in desc, replace=desc is not None and D.R in desc, accum=None if accum is None else ("PLUS", typ))
        gi, gj, gx = outs[0]
        assert np.array_equal(gi.astype(np.int64) * 180 + gj.astype(np.int64), want.keys) and gx.tobytes() == want.vals.astype(NPT[typ]).tobytes(), (form, "mxm model", desc)
    # each input transposed: A' B with A' stored as its transpose, A B' likewise
    At = gb.Matrix.from_arrays(ca[1], ca[0], ca[2], 150, 200, T)
    Bt = gb.Matrix.from_arrays(cb[1], cb[0], cb[2], 180, 150, T)
    plain = A.mxm(B, usr, out=gb.Matrix.sparse(T, 200, 180)).to_arrays()
    assert same_bits(At.mxm(B, usr, out=gb.Matrix.sparse(T, 200, 180), desc=D.T0).to_arrays(), plain)
    assert same_bits(A.mxm(Bt, usr, out=gb.Matrix.sparse(T, 200, 180), desc=D.T1).to_arrays(), plain)
    assert same_bits(At.mxm(Bt, usr, out=gb.Matrix.sparse(T, 200, 180), desc=D.T0 & D.T1).to_arrays(), plain)
    # a matrix without entries on either side
    Z = gb.Matrix.sparse(T, 150, 180)
    assert A.mxm(Z, usr, out=gb.Matrix.sparse(T, 200, 180)).nvals == 0
    assert gb.Matrix.sparse(T, 200, 150).mxm(B, usr, out=gb.Matrix.sparse(T, 200, 180)).nvals == 0


# ---- 3. argument order --------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_order(gb, gpu):
    T = gb.INT64
    add, mul = gb.binary_op(T)(u_add), gb.binary_op(T)(u_order)
    sr = T.new_semiring(T.new_monoid(add, 0), mul)
    rng = np.random.default_rng(3)
    n = 300
    coo = rows_matrix(rng, "INT64", n)
    A = mat(gb, coo, n, n, "INT64")
    uvals = rng.integers(1, 50, n).astype(np.int64)
    u = vec(gb, np.arange(n), uvals, n, "INT64")
    I, J, X = coo[0].astype(np.int64), coo[1].astype(np.int64), coo[2]

    def model(rows, cols, first, second):                 # t(rows) += first * 4 + second
        t = np.zeros(n, np.int64); np.add.at(t, rows, first * 4 + second)
        return t, np.unique(rows)
    # mxv: mul(A(i,j), u(j)) summed into i
    want, pat = model(I, J, X, uvals[J])
    gi, gx = A.mxv(u, sr).to_arrays()
    assert np.array_equal(gi, pat) and np.array_equal(gx, want[pat])
    # vxm: mul(u(i), A(i,j)) summed into j — the model of mxv over the transpose WITH THE ARGUMENTS SWAPPED
    want_v, pat_v = model(J, I, uvals[I], X)
    gi, gx = u.vxm(A, sr).to_arrays()
    assert np.array_equal(gi, pat_v) and np.array_equal(gx, want_v[pat_v])
    unswapped, _ = model(J, I, X, uvals[I])
    assert not np.array_equal(gx, unswapped[pat_v])        # the data tell the two orders apart: the test cannot pass by symmetry
    # and GrB_mxv of the transpose differs from GrB_vxm accordingly
    gi2, gx2 = A.mxv(u, sr, desc=gb.descriptor.T0).to_arrays()
    assert np.array_equal(gi2, pat_v) and np.array_equal(gx2, unswapped[pat_v])
    # mxm: mul(A(i,k), B(k,j))
    ca, cb = product_operands(rng, "INT64")
    keys, vals = model_product(ca, cb, "INT64", lambda x, y: x + y, lambda x, y: x * 4 + y)
    ci, cj, cx = mat(gb, ca, 200, 150, "INT64").mxm(mat(gb, cb, 150, 180, "INT64"), sr).to_arrays()
    assert list(zip(ci.tolist(), cj.tolist())) == keys and np.array_equal(cx, vals)
    keys2, vals2 = model_product(ca, cb, "INT64", lambda x, y: x + y, lambda x, y: y * 4 + x)
    assert keys2 == keys and not np.array_equal(vals2, vals)


# ---- 4. the identity is not folded ----------------------------------------------------------------------------------------------------------------------------------
def test_identity_is_never_combined(gb, gpu):
    T = gb.INT64
    add, mul = gb.binary_op(T)(u_add), gb.binary_op(T)(u_mul)
    mon = T.new_monoid(add, 12345)
    sr = T.new_semiring(mon, mul)
    rng = np.random.default_rng(8)
    n = 300
    A = mat(gb, rows_matrix(rng, "INT64", n), n, n, "INT64")            # row 1 has one entry: a sum of one product
    u = vec(gb, np.arange(n), values(rng, "INT64", n), n, "INT64")
    assert same_bits(A.mxv(u, sr).to_arrays(), A.mxv(u, T.PLUS_TIMES).to_arrays())
    assert same_bits(u.vxm(A, sr).to_arrays(), u.vxm(A, T.PLUS_TIMES).to_arrays())
    assert same_bits(A.reduce_vector(mon).to_arrays(), A.reduce_vector(T.PLUS_MONOID).to_arrays())
    ca, cb = product_operands(rng, "INT64")
    P, Q = mat(gb, ca, 200, 150, "INT64"), mat(gb, cb, 150, 180, "INT64")
    got, want = P.mxm(Q, sr).to_arrays(), P.mxm(Q, T.PLUS_TIMES).to_arrays()
    assert same_bits(got, want)
    # a monoid and a semiring made of built-ins only take the same route and keep the same rule
    bmon = T.new_monoid(T.PLUS, 12345)
    bsr = T.new_semiring(bmon, T.TIMES)
    assert same_bits(A.mxv(u, bsr).to_arrays(), A.mxv(u, T.PLUS_TIMES).to_arrays())
    assert same_bits(A.mxv(u, bsr).to_arrays(), A.mxv(u, sr).to_arrays()) and gb.last_kernel_plan().startswith("usersr<add=u_add")
    A.mxv(u, bsr)
    assert gb.last_kernel_plan().startswith("usersr<add=GrB_PLUS_INT64,mul=GrB_TIMES_INT64,type=GrB_INT64,kind=mxv>"), gb.last_kernel_plan()
    assert same_bits(A.reduce_vector(bmon).to_arrays(), A.reduce_vector(T.PLUS_MONOID).to_arrays())
    A.reduce_vector(bmon)
    assert gb.last_kernel_plan().startswith("usersr<add=GrB_PLUS_INT64,mul=none,type=GrB_INT64,kind=reduce_rows>"), gb.last_kernel_plan()
    assert same_bits(P.mxm(Q, bsr).to_arrays(), want)
    # GrB_Semiring_new over such a monoid: the same route and rule with a multiplier of the list, GrB_DOMAIN_MISMATCH naming any other — never another operator's result
    h = C.c_void_p()
    assert gb.lib.GrB_Semiring_new(C.byref(h), C.c_void_p(bmon.get_op()), C.c_void_p(T.TIMES.get_op())) == 0
    w1, w2 = gb.Vector.sparse(T, n), gb.Vector.sparse(T, n)
    assert gb.lib.GrB_mxv(w1._h, None, None, h, A._h, u._h, None) == 0 and gb.last_kernel_plan().startswith("usersr<add=GrB_PLUS_INT64,mul=GrB_TIMES_INT64")
    assert same_bits(w1.to_arrays(), A.mxv(u, T.PLUS_TIMES).to_arrays())
    gb.lib.GrB_Semiring_free(C.byref(h))
    assert gb.lib.GrB_Semiring_new(C.byref(h), C.c_void_p(bmon.get_op()), C.c_void_p(T.DIV.get_op())) == 0
    assert gb.lib.GrB_mxv(w2._h, None, None, h, A._h, u._h, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and w2.nvals == 0
    assert gb.lib.GrB_mxm(gb.Matrix.sparse(T, 200, 180)._h, None, None, h, P._h, Q._h, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    gb.lib.GrB_Semiring_free(C.byref(h))
    one = gb.Matrix.from_lists([0, 1], [1, 0], [3, 5], 2, 2, T)          # every entry of the square is one product
    assert one.mxm(one, sr).to_lists() == [[0, 1], [0, 1], [15, 15]]


# ---- 5. the order of the product's additions ------------------------------------------------------------------------------------------------------------------------
def test_product_adds_left_to_right_in_ascending_k(gb, gpu):
    T = gb.FP64
    add, mul = gb.binary_op(T)(u_add), gb.binary_op(T)(u_mul)
    sr = T.new_semiring(T.new_monoid(add, 0.0), mul)
    rng = np.random.default_rng(21)
    ca, cb = product_operands(rng, "FP64")
    big = lambda k: (rng.choice([-1.0, 1.0], k) * np.ldexp(rng.random(k) + 0.5, rng.integers(-20, 62, k))).astype(np.float64)      # magnitudes up to 2^61, mixed signs
    ca, cb = (ca[0], ca[1], big(len(ca[0]))), (cb[0], cb[1], np.ldexp(rng.random(len(cb[0])) + 0.5, rng.integers(-4, 5, len(cb[0]))) * rng.choice([-1.0, 1.0], len(cb[0])))
    A, B = mat(gb, ca, 200, 150, "FP64"), mat(gb, cb, 150, 180, "FP64")
    keys, vals = model_product(ca, cb, "FP64", lambda x, y: x + y, lambda x, y: x * y)
    _, descending = model_product((ca[0][::-1], ca[1][::-1], ca[2][::-1]), cb, "FP64", lambda x, y: x + y, lambda x, y: x * y)
    assert descending.tobytes() != vals.tobytes()                       # on these data the order of the additions shows
    first = A.mxm(B, sr).to_arrays()
    assert list(zip(first[0].tolist(), first[1].tolist())) == keys and first[2].tobytes() == vals.tobytes()
    assert same_bits(A.mxm(B, sr).to_arrays(), first)                   # and the same bits on a second run


# ---- 6. the log semiring at size -----------------------------------------------------------------------------------------------------------------------------------
# (operation, type) -> twice the largest relative error measured on the MI355X.  FP32 is not the 0 ulp of the eWise
# case: the order of the additions differs from the model's.
# Measured: FP32 mxv 4.047e-05, mxm 4.131e-03; FP64 mxv 4.285e-14, mxm 1.105e-11 — the largest ones at results near zero (the logarithm of a sum near 1), where the
# absolute error of a few units in the last place of the terms is divided by a tiny value.
LOG_BOUND = {("mxv", "FP32"): 2 * 4.047e-05, ("mxm", "FP32"): 2 * 4.131e-03, ("mxv", "FP64"): 2 * 4.285e-14, ("mxm", "FP64"): 2 * 1.105e-11}


@pytest.mark.parametrize("typ", ["FP32", "FP64"])
def test_log_semiring_at_size(gb, gpu, typ):
    """mxv over the 300-row matrix and mxm over the product shapes against a float64 model: np.logaddexp.reduce over the products.  Prints the largest relative
    error of each; each bound is twice the value measured on the MI355X."""
    T = getattr(gb, typ)
    plus, times = gb.binary_op(T)(log_plus), gb.binary_op(T)(log_times)
    sr = T.new_semiring(T.new_monoid(plus, 1.0), times)
    rng = np.random.default_rng(13)
    n = 300
    I, J, _ = rows_matrix(rng, typ, n)
    X = np.log(rng.random(len(I)) + 0.05).astype(NPT[typ])
    uv = np.log(rng.random(n) + 0.05).astype(NPT[typ])
    gi, gx = gb.Matrix.from_arrays(I, J, X, n, n, T).mxv(gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), uv, n, T), sr).to_arrays()
    prods = X.astype(np.float64) + uv.astype(np.float64)[J.astype(np.int64)]
    rows = I.astype(np.int64)
    want = np.array([np.logaddexp.reduce(prods[rows == i]) for i in gi])
    assert np.array_equal(gi, np.unique(rows))
    rel_v = float(np.max(np.abs(gx.astype(np.float64) - want) / np.abs(want)))
    ca, cb = product_operands(rng, typ)
    ca = (ca[0], ca[1], np.log(rng.random(len(ca[0])) + 0.05).astype(NPT[typ])); cb = (cb[0], cb[1], np.log(rng.random(len(cb[0])) + 0.05).astype(NPT[typ]))
    ci, cj, cx = mat(gb, ca, 200, 150, typ).mxm(mat(gb, cb, 150, 180, typ), sr).to_arrays()
    terms = {}
    brow = {}
    for k, j, x in zip(cb[0].tolist(), cb[1].tolist(), cb[2].astype(np.float64).tolist()):
        brow.setdefault(k, []).append((j, x))
    for i, k, a in zip(ca[0].tolist(), ca[1].tolist(), ca[2].astype(np.float64).tolist()):
        for j, b in brow.get(k, ()):
            terms.setdefault((i, j), []).append(a + b)
    keys = sorted(terms)
    assert list(zip(ci.tolist(), cj.tolist())) == keys
    want = np.array([np.logaddexp.reduce(np.array(terms[k])) for k in keys])
    rel_m = float(np.max(np.abs(cx.astype(np.float64) - want) / np.abs(want)))
    print(f"log semiring at size, {typ}: largest relative error mxv {rel_v:.3e} mxm {rel_m:.3e}")
    assert rel_v <= LOG_BOUND[("mxv", typ)] and rel_m <= LOG_BOUND[("mxm", typ)]


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------------------------------------------------------
def stats(gb):
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert gb.lib.GrBX_userop_stats(C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


def got_dict(x):
    a = x.to_arrays()
    return {(tuple(int(v) for v in k) if len(a) == 3 else int(k[0])): float(v) for *k, v in zip(*a)}


def test_plan_string_and_compile_once(gb, gpu):
    T = gb.FP64
    add, mul = gb.binary_op(T)(u_add), gb.binary_op(T)(u_order)
    mon = T.new_monoid(add, 0.0)
    sr = T.new_semiring(mon, mul)
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    for call, kind in ((lambda: A.mxv(v, sr), "mxv"), (lambda: v.vxm(A, sr), "vxm"), (lambda: A.mxm(A, sr), "mxm"), (lambda: A.reduce_vector(mon), "reduce_rows")):
        call()
        plan = gb.last_kernel_plan()
        mul_name = "none" if kind == "reduce_rows" else "u_order"
        assert plan.startswith(f"usersr<add=u_add,mul={mul_name},type=GrB_FP64,kind={kind}>"), plan
        assert ("grb_usersr_product" if kind == "mxm" else "grb_usersr_rows") in plan
        before = stats(gb)
        call()
        after = stats(gb)
        assert after[0] == before[0] and after[1] == before[1] and after[2] == before[2] + 1, (kind, before, after)      # nothing compiled, nothing loaded: one launch


def test_a_definition_that_does_not_compile(gb, gpu):
    h, t = C.c_void_p(), C.c_void_p(gb.FP64._h)
    assert gb.lib.GxB_BinaryOp_new(C.byref(h), None, t, t, t, b"broken", b"void broken (double *z, const double *x, const double *y) { (*z) = (*x) +* ; }") == 0
    s = C.c_void_p()
    assert gb.lib.GrBX_Semiring_new_user(C.byref(s), C.c_void_p(gb.FP64.PLUS_MONOID.get_op()), h) == 0
    A = gb.Matrix.from_lists([0, 1], [1, 0], [1.0, 2.0])
    out = gb.Matrix.from_lists([0], [0], [5.0], 2, 2)
    info = gb.lib.GrB_mxm(out._h, None, None, s, A._h, A._h, None)
    assert info == gb._capi.constants["GrB_INVALID_VALUE"]
    msg = C.c_char_p()
    assert gb.lib.GrB_Matrix_error(C.byref(msg), out._h) == 0
    text = msg.value.decode()
    assert "broken" in text and "error" in text and "expected expression" in text, text
    assert got_dict(out) == {(0, 0): 5.0}
    w = gb.Vector.from_lists([1], [6.0], 2)
    v = gb.Vector.from_lists([0, 1], [1.0, 1.0])
    assert gb.lib.GrB_mxv(w._h, None, None, s, A._h, v._h, None) == gb._capi.constants["GrB_INVALID_VALUE"]
    assert got_dict(w) == {1: 6.0}
    gb.lib.GrB_Semiring_free(C.byref(s)); gb.lib.GrB_BinaryOp_free(C.byref(h))


def test_what_stays_refused_leaves_the_output_alone(gb, gpu):
    DM = gb.DomainMismatch
    T = gb.FP64
    add, mul = gb.binary_op(T)(u_add), gb.binary_op(T)(u_mul)
    mon = T.new_monoid(add, 0.0)
    sr = T.new_semiring(mon, mul)
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    out = gb.Matrix.from_lists([0], [0], [5.0], 3, 3)
    w = gb.Vector.from_lists([1], [6.0], 3)
    for what, fn in (("accumulator of mxm", lambda: A.mxm(A, sr, out=out, accum=add)), ("accumulator of mxv", lambda: A.mxv(v, sr, out=w, accum=add)),
                     ("accumulator of vxm", lambda: v.vxm(A, sr, out=w, accum=add)), ("accumulator of reduce_vector", lambda: A.reduce_vector(mon, out=w, accum=add)),
                     ("kronecker", lambda: A.kronecker(A, add, out=gb.Matrix.sparse(T, 9, 9)))):
        with pytest.raises(DM, match="u_add"):
            fn()
        assert got_dict(out) == {(0, 0): 5.0} and got_dict(w) == {1: 6.0}, what
    # reduction to a scalar with a user monoid
    x = C.c_double(1.5)
    assert gb.lib.GrB_Matrix_reduce_FP64(C.byref(x), None, C.c_void_p(mon.get_op()), A._h, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and x.value == 1.5
    assert gb.lib.GrB_Vector_reduce_FP64(C.byref(x), None, C.c_void_p(mon.get_op()), v._h, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and x.value == 1.5
    buf = C.create_string_buffer(1024)
    gb.lib.GrBX_last_error(buf, C.c_int(1024))
    assert b"u_add" in buf.value
    # hypersparse operands
    H = gb.Matrix.sparse(T)
    H[3, 1 << 40] = 2.0
    H2 = gb.Matrix.sparse(T)
    H2[7, 7] = 1.0
    hv, hv2 = gb.Vector.sparse(T), gb.Vector.sparse(T)
    hv[1 << 40] = 2.0
    hv2[5] = 1.0
    for fn in (lambda: H.mxm(H, sr, out=H2), lambda: H.mxv(hv, sr, out=hv2), lambda: hv.vxm(H, sr, out=hv2), lambda: H.reduce_vector(mon, out=hv2)):
        with pytest.raises(DM, match="hypersparse"):
            fn()
        assert got_dict(H2) == {(7, 7): 1.0} and got_dict(hv2) == {5: 1.0}


_MODE_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import pygraphblas_amd as gb
import test_usersemiring_gpu as t
n = 2000
rng = np.random.default_rng(1)
idx = np.arange(n, dtype=np.uint64)
u = gb.Vector.from_arrays(idx, rng.integers(-16, 17, n) / 8.0, n, gb.FP64)
v = gb.Vector.from_arrays(idx, rng.integers(-16, 17, n) / 8.0, n, gb.FP64)
A = gb.Matrix.from_arrays(idx, (idx * 7 + 1) % n, rng.integers(1, 9, n) / 4.0, n, n, gb.FP64)
add = gb.binary_op(gb.FP64)(t.u_max); mul = gb.binary_op(gb.FP64)(t.u_add)
sr = gb.FP64.new_semiring(gb.FP64.new_monoid(add, 0.0), mul)
w = u.eadd(v, gb.FP64.PLUS)            # deferred in non-blocking mode
w = w.apply(gb.FP64.AINV)              # ... and chained
r = A.mxv(w, sr)                       # the user semiring: the pending chain is completed, then the product runs eagerly
plan = gb.last_kernel_plan()
r2 = r.apply(gb.FP64.ABS)              # built-in work queued after it reads the result
I, X = r2.to_arrays()
print(plan.split(">")[0])
print(float(X.sum()), float(np.abs(X).max()), len(I), X[:5].tolist())
"""


def test_nonblocking_chain_completes_before_the_product(gb, gpu):
    code = _MODE_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    outs = []
    for blocking in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GRB_MI355X_BLOCKING=blocking), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.strip().splitlines()[-2:])
    assert outs[0] == outs[1], outs
    assert outs[0][0] == "usersr<add=u_max,mul=u_add,type=GrB_FP64,kind=mxv"
    rng = np.random.default_rng(1)
    n = 2000
    a = rng.integers(-16, 17, n) / 8.0
    b = rng.integers(-16, 17, n) / 8.0
    x = rng.integers(1, 9, n) / 4.0
    w = -(a + b)
    want = np.abs(x + w[(np.arange(n) * 7 + 1) % n])
    assert outs[0][1].startswith(repr(float(want.sum())) + " ")
