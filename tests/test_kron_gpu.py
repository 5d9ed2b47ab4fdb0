"""The Kronecker product on the device (grb_kron.hip behind GrB_Matrix_kronecker_BinaryOp / _Monoid / _Semiring / GxB_kron) and Matrix.kronpow.

References, none of them the code under test:
  * a dict model of the rule written here: T[(ia br + ib, ja bc + jb)] = op(a, b) in the operator's domain, then C<M, replace> = accum(C, T);
  * numpy key arithmetic ia br + ib, ja bc + jb for the shapes that strain the index arithmetic and for the 6.4e7-entry product;
  * numpy float64 products for the Kronecker power;
  * the forced host route (GRB_MI355X_KRON=0): the code every earlier version ran.
Values are 0 .. 5 with explicit zeros, exact in all eleven types, so every comparison is bit-exact, floating point included.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUTES = (0, 1)
TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
MASKS = [None, "valued", "structural", "complemented", "structural+complemented"]
ACCUMS = [None, "PLUS", "SECOND"]
OPS = ["TIMES", "PLUS", "MIN", "FIRST", "SECOND", "PAIR", "EQ"]


# ---- helpers (the conventions of the extract / assign tests) ---------------------------------------------------------------
@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def typ(gb, name):
    return getattr(gb, name)


def npdt(gb, name):
    return np.dtype(typ(gb, name)._np)


def values(rng, gb, name, n):
    """0 .. 5 (BOOL: 0 / 1), explicit zeros included: exact in all eleven types; products stay below 2^5, sums with one below 2^6."""
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    return rng.integers(0, 6, n).astype(npdt(gb, name))


def random_tuples(rng, gb, name, nrows, ncols, density):
    total = nrows * ncols
    nnz = min(total, int(round(total * density)))
    flat = np.sort(rng.choice(total, size=nnz, replace=False)) if total else np.zeros(0, np.int64)
    I, J = (np.divmod(flat, ncols) if total else (flat, flat))
    return I.astype(np.uint64), J.astype(np.uint64), values(rng, gb, name, nnz)


def cast(v, dt):
    if dt == np.bool_:
        return np.bool_(v != 0)
    return np.asarray(v).astype(dt)[()]


def binop(name, a, b):
    """The operator in its own domain: a and b already have that dtype, so has the result (a comparison gives 0 / 1 in it)."""
    dt = a.dtype
    if name == "FIRST":
        return a
    if name == "SECOND":
        return b
    if name == "PAIR":
        return cast(1, dt)
    if name == "EQ":
        return cast(a == b, dt)
    if dt == np.bool_:
        return (a | b) if name == "PLUS" else (a & b)                   # BOOL: PLUS is LOR, TIMES and MIN are LAND
    if name == "PLUS":
        return (a + b).astype(dt)
    if name == "TIMES":
        return (a * b).astype(dt)
    return min(a, b)


def as_sorted(d, cdt):
    keys = sorted(d)
    X = np.array([d[k] for k in keys], dtype=cdt) if keys else np.zeros(0, cdt)
    return np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64), X


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and g.dtype == e.dtype and np.array_equal(g, e), f"{what}: got {g[:12]} expected {e[:12]} (lengths {g.shape} / {e.shape})"


def descriptor(gb, mask_kind, replace, t0, t1):
    d = None
    parts = []
    if replace:
        parts.append(gb.descriptor.R)
    if mask_kind and "structural" in mask_kind:
        parts.append(gb.descriptor.S)
    if mask_kind and "complemented" in mask_kind:
        parts.append(gb.descriptor.C)
    if t0:
        parts.append(gb.descriptor.T0)
    if t1:
        parts.append(gb.descriptor.T1)
    for p in parts:
        d = p if d is None else (d & p)
    return d


def other_plan(gb):
    """Some other plan string: the host route of kronecker leaves the last one alone."""
    ones = gb.Vector.from_arrays(np.arange(3, dtype=np.uint64), np.ones(3, np.int32), 3, gb.INT32)
    gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1, 2, 3], 3, 3, gb.INT32).mxv(ones, semiring=gb.INT32.PLUS_TIMES)
    assert not gb.last_kernel_plan().startswith("kronecker<")


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_kron(A, B, br, bc, opname, odt, C, cdt, M, mask_kind, accum, replace):
    """C<M, replace> = accum(C, op(A) (x)_op op(B)) on dicts.  A, B: {(i, j): value} of op(A), op(B); odt: the operator's domain."""
    T = {}
    for (ia, ja), a in A.items():
        for (ib, jb), b in B.items():
            T[(ia * br + ib, ja * bc + jb)] = binop(opname, cast(a, odt), cast(b, odt))
    Z = {}
    if accum:
        Z = dict(C)
        for p, t in T.items():
            Z[p] = binop(accum, Z[p], cast(t, cdt)) if p in Z else cast(t, cdt)      # the accumulator is taken from C's type: both sides in it
    else:
        Z = {p: cast(t, cdt) for p, t in T.items()}
    comp = mask_kind is not None and "complemented" in mask_kind
    structural = mask_kind is not None and "structural" in mask_kind

    def allows(p):
        if M is None:
            return not comp
        return ((p in M) and (structural or bool(M[p]))) != comp
    out = {p: v for p, v in C.items() if not allows(p) and not replace}
    out.update({p: v for p, v in Z.items() if allows(p)})
    return out


def make_case(i, rng):
    c = {"atype": TYPES[i % 11], "op": OPS[i % 7], "mask": MASKS[(i // 2) % 5], "accum": ACCUMS[(i // 3) % 3], "replace": (i // 5) % 2 == 1,
         "t0": (i // 7) % 2 == 1, "t1": (i // 13) % 2 == 1, "prefill": (i // 4) % 3 != 0}
    c["btype"] = c["atype"] if i % 3 else TYPES[(i * 5 + 2) % 11]          # mixed operand types: both are cast into the operator's domain
    c["optype"] = c["atype"] if i % 4 else TYPES[(i * 3 + 1) % 11]
    c["ctype"] = c["optype"] if i % 2 else TYPES[(i * 7 + 3) % 11]
    c["mtype"] = ["BOOL", "INT8", "FP32"][i % 3]
    c["ar"], c["ac"], c["br"], c["bc"] = int(rng.integers(1, 13)), int(rng.integers(1, 10)), int(rng.integers(1, 8)), int(rng.integers(1, 11))
    c["da"], c["db"] = float(rng.choice([0.0, 0.3, 1.0])), float(rng.choice([0.0, 0.3, 1.0]))
    return c


def run_case(gb, c, rng):
    ar, ac, br, bc = c["ar"], c["ac"], c["br"], c["bc"]
    am, an = (ac, ar) if c["t0"] else (ar, ac)                      # the operands' own shapes: op(A) is ar x ac
    bm, bn = (bc, br) if c["t1"] else (br, bc)
    nr, nc = ar * br, ac * bc
    AI, AJ, AX = random_tuples(rng, gb, c["atype"], am, an, c["da"])
    BI, BJ, BX = random_tuples(rng, gb, c["btype"], bm, bn, c["db"])
    CI, CJ, CX = random_tuples(rng, gb, c["ctype"], nr, nc, 0.3 if c["prefill"] else 0.0)
    MI, MJ, MX = random_tuples(rng, gb, c["mtype"], nr, nc, 0.5) if c["mask"] else (None, None, None)
    cdt, odt = npdt(gb, c["ctype"]), npdt(gb, c["optype"])
    Ad = {((int(b), int(a)) if c["t0"] else (int(a), int(b))): x for a, b, x in zip(AI, AJ, AX)}
    Bd = {((int(b), int(a)) if c["t1"] else (int(a), int(b))): x for a, b, x in zip(BI, BJ, BX)}
    Cd = {(int(a), int(b)): x for a, b, x in zip(CI, CJ, CX)}
    Md = {(int(a), int(b)): x for a, b, x in zip(MI, MJ, MX)} if c["mask"] else None
    exp = as_sorted(model_kron(Ad, Bd, br, bc, c["op"], odt, Cd, cdt, Md, c["mask"], c["accum"], c["replace"]), cdt)
    got = {}
    for route in ROUTES:
        A = gb.Matrix.from_arrays(AI, AJ, AX, am, an, typ(gb, c["atype"]))
        B = gb.Matrix.from_arrays(BI, BJ, BX, bm, bn, typ(gb, c["btype"]))
        Cm = gb.Matrix.from_arrays(CI, CJ, CX, nr, nc, typ(gb, c["ctype"]))
        M = gb.Matrix.from_arrays(MI, MJ, MX, nr, nc, typ(gb, c["mtype"])) if c["mask"] else None
        acc = getattr(typ(gb, c["ctype"]), c["accum"]) if c["accum"] else None
        op = getattr(typ(gb, c["optype"]), c["op"])
        with env(GRB_MI355X_KRON=route):
            A.kronecker(B, op=op, out=Cm, mask=M, accum=acc, desc=descriptor(gb, c["mask"], c["replace"], c["t0"], c["t1"]))
            plan = gb.last_kernel_plan()
        if route == 1:
            assert plan.startswith("kronecker<"), (plan, c)
        got[route] = Cm.to_arrays()
        same(got[route], exp, f"route {route} vs model, case {c}")
    same(got[1], got[0], f"device route vs host route, case {c}")
    return True


# ---- 1. model parity, both routes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(6))
def test_parity(gb, gpu, block):
    rng = np.random.default_rng(21000 + block)
    ran = 0
    for i in range(block * 77, block * 77 + 77):                    # 462 cases: every (type, operator) pair six times, every mask / accum / replace / transpose setting
        ran += bool(run_case(gb, make_case(i, rng), rng))
    assert ran == 77


def test_cast_of_mixed_operands(gb, gpu):
    """INT8 (x) FP32 with `cast`: the output is made in that type, the default multiplier is the promoted type's TIMES."""
    A = gb.Matrix.from_lists([0, 1], [1, 0], [2, 3], 2, 2, gb.INT8)
    B = gb.Matrix.from_lists([0, 0], [0, 2], [1.5, 4.0], 1, 3, gb.FP32)
    for route in ROUTES:
        with env(GRB_MI355X_KRON=route):
            K = A.kronecker(B, cast=gb.INT64)
        assert K.type is gb.INT64 and K.shape == (2, 6)
        assert K.to_lists() == [[0, 0, 1, 1], [3, 5, 0, 2], [3, 8, 4, 12]]      # 2 x 1.5 = 3.0, 3 x 1.5 = 4.5 -> 4 in INT64


def test_route_and_plan(gb, gpu):
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [2, 3, 4], 3, 3, gb.INT64)
    B = gb.Matrix.from_lists([0, 1], [1, 0], [5, 6], 2, 2, gb.INT64)
    exp = [[0, 1, 2, 3, 4, 5], [3, 2, 5, 4, 1, 0], [10, 12, 15, 18, 20, 24]]
    for route in (0, None):                                         # forced host route; and a 6-entry host-resident product keeps it by itself
        other_plan(gb)
        with env(GRB_MI355X_KRON=route):
            K = A.kronecker(B)
            assert not gb.last_kernel_plan().startswith("kronecker<"), gb.last_kernel_plan()
        assert K.to_lists() == exp
    with env(GRB_MI355X_KRON=1):
        K = A.kronecker(B)
        assert gb.last_kernel_plan().startswith("kronecker<op=") and "transpose0=0,transpose1=0,accum=none> k_kron_rowptr k_kron_fill" in gb.last_kernel_plan(), gb.last_kernel_plan()
        assert K.to_lists() == exp
        A.kronecker(B, out=K, accum=gb.INT64.PLUS, desc=gb.descriptor.T0 & gb.descriptor.T1)
        assert "transpose0=1,transpose1=1" in gb.last_kernel_plan() and "accum=none" not in gb.last_kernel_plan(), gb.last_kernel_plan()
        other_plan(gb)
        K2 = gb.Matrix.from_lists([0], [0], [1], 9, 9, gb.INT64)
        K2.kronecker(gb.Matrix.from_lists([0], [0], [2], 1, 1, gb.INT64), out=K2)            # an operand that is the output: the host route
        assert not gb.last_kernel_plan().startswith("kronecker<"), gb.last_kernel_plan()
        assert K2.to_lists() == [[0], [0], [2]]
    # an operand that lives in HBM only: the device route with nothing set
    rp, ci, x = A.to_csr()
    Ad = gb.Matrix.from_csr(gb.INT64, 3, 3, rp, ci, x)
    other_plan(gb)
    with env(GRB_MI355X_KRON=None):
        K = Ad.kronecker(B)
        assert gb.last_kernel_plan().startswith("kronecker<"), gb.last_kernel_plan()
    assert K.to_lists() == exp


# ---- 2. shapes that break index arithmetic -----------------------------------------------------------------------------------
def numpy_kron(AI, AJ, AX, BI, BJ, BX, br, bc):
    """Sorted (rows, columns, values) of the product by key arithmetic in 64 bits; values multiplied in the operands' dtype."""
    rows = (AI.astype(np.uint64)[:, None] * np.uint64(br) + BI.astype(np.uint64)[None, :]).ravel()
    cols = (AJ.astype(np.uint64)[:, None] * np.uint64(bc) + BJ.astype(np.uint64)[None, :]).ravel()
    vals = (AX[:, None] * BX[None, :]).ravel()
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]


def check_shape(gb, t, A, ashape, B, bshape, routes=ROUTES):
    exp = numpy_kron(*A, *B, bshape[0], bshape[1])
    for route in routes:
        Am = gb.Matrix.from_arrays(*A, ashape[0], ashape[1], t)
        Bm = gb.Matrix.from_arrays(*B, bshape[0], bshape[1], t)
        with env(GRB_MI355X_KRON=route):
            K = Am.kronecker(Bm)
            plan = gb.last_kernel_plan()
        if route == 1:
            assert plan.startswith("kronecker<"), plan
        assert K.shape == (ashape[0] * bshape[0], ashape[1] * bshape[1]) and K.nvals == len(exp[0])
        same(K.to_arrays(), exp, f"shape {ashape} (x) {bshape}, route {route}")


def tuples(I, J, X, dt):
    return np.asarray(I, np.uint64), np.asarray(J, np.uint64), np.asarray(X, dt)


def test_empty_operands(gb, gpu):
    full = tuples([0, 0, 1, 2], [0, 3, 1, 2], [1, 2, 3, 4], np.int32)
    none = tuples([], [], [], np.int32)
    check_shape(gb, gb.INT32, none, (5, 6), full, (3, 4))
    check_shape(gb, gb.INT32, full, (3, 4), none, (5, 6))
    check_shape(gb, gb.INT32, none, (2, 2), none, (3, 3))


def test_row_times_column(gb, gpu):
    n = 50
    row = tuples(np.zeros(n), np.arange(n), np.arange(n) % 5 + 1, np.int64)
    col = tuples(np.arange(n), np.zeros(n), np.arange(n) % 4 + 1, np.int64)
    check_shape(gb, gb.INT64, row, (1, n), col, (n, 1))
    check_shape(gb, gb.INT64, col, (n, 1), row, (1, n))


def test_empty_rows_between_full_ones(gb, gpu):
    rng = np.random.default_rng(5)
    # rows 0, 3 and 9 of A full, the others empty (the first row of B too): every bisection lands on runs of equal row-pointer words
    AI = np.repeat([0, 3, 9], 7); AJ = np.tile(np.arange(7), 3)
    BI = np.repeat([1, 2, 6], 5); BJ = np.tile(np.arange(5), 3)
    A = tuples(AI, AJ, rng.integers(1, 6, len(AI)), np.float64)
    B = tuples(BI, BJ, rng.integers(1, 6, len(BI)), np.float64)
    check_shape(gb, gb.FP64, A, (11, 7), B, (8, 5))
    check_shape(gb, gb.FP64, B, (8, 5), A, (11, 7))


def test_one_long_row(gb, gpu):
    """One 3 000-entry row times one 3 000-entry row: a single output row of 9e6 entries, spread over the lanes like any other 9e6 entries (device route only:
    the host route's map of 9e6 nodes is what this kernel replaces)."""
    n = 3000
    rng = np.random.default_rng(6)
    A = tuples(np.zeros(n), np.arange(n), rng.integers(0, 6, n), np.float32)
    B = tuples(np.zeros(n), np.arange(n), rng.integers(0, 6, n), np.float32)
    check_shape(gb, gb.FP32, A, (1, n), B, (1, n), routes=(1,))


def test_wide_dimensions_few_entries(gb, gpu):
    """40 000 x 1 (x) 1 x 40 000: 1.6e9 positions, a handful of entries; and 1 x 60 000 (x) 1 x 60 000: column keys ja bc + jb up to 3.6e9, beyond 2^31."""
    rng = np.random.default_rng(7)
    n = 40000
    ia = np.sort(rng.choice(n, 20, replace=False)); ib = np.sort(rng.choice(n, 20, replace=False))
    ia[-1] = n - 1; ib[-1] = n - 1
    col = tuples(ia, np.zeros(20), rng.integers(1, 6, 20), np.int64)
    row = tuples(np.zeros(20), ib, rng.integers(1, 6, 20), np.int64)
    check_shape(gb, gb.INT64, col, (n, 1), row, (1, n))
    check_shape(gb, gb.INT64, row, (1, n), col, (n, 1))
    n = 60000
    ja = np.sort(rng.choice(n, 20, replace=False)); jb = np.sort(rng.choice(n, 20, replace=False))
    ja[-1] = n - 1; jb[-1] = n - 1
    r1 = tuples(np.zeros(20), ja, rng.integers(1, 6, 20), np.int64)
    r2 = tuples(np.zeros(20), jb, rng.integers(1, 6, 20), np.int64)
    check_shape(gb, gb.INT64, r1, (1, n), r2, (1, n))


# ---- 3. large, device route only ---------------------------------------------------------------------------------------------
def random_csr(rng, n, nnz, dt):
    flat = np.sort(rng.choice(n * n, size=nnz, replace=False))
    I, J = np.divmod(flat, n)
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, I + 1, 1); rp = np.cumsum(rp)
    return rp.astype(np.uint32), J.astype(np.uint32), rng.random(nnz).astype(dt)


def test_large_product_in_hbm(gb, gpu):
    """Two FP32 4 096 x 4 096 operands of 8 000 entries that live in HBM only: 6.4e7 entries through the device route with nothing set."""
    rng = np.random.default_rng(8)
    n, nnz = 4096, 8000
    arp, acol, aval = random_csr(rng, n, nnz, np.float32)
    brp, bcol, bval = random_csr(rng, n, nnz, np.float32)
    A = gb.Matrix.from_csr(gb.FP32, n, n, arp, acol, aval)
    B = gb.Matrix.from_csr(gb.FP32, n, n, brp, bcol, bval)
    other_plan(gb)
    with env(GRB_MI355X_KRON=None):
        K = A.kronecker(B)
        plan = gb.last_kernel_plan()
    assert plan.startswith("kronecker<") and "k_kron_rowptr k_kron_fill" in plan, plan
    assert K.type is gb.FP32 and K.shape == (n * n, n * n) and K.nvals == nnz * nnz
    rp, col, val = K.to_csr()
    arp64, brp64 = arp.astype(np.int64), brp.astype(np.int64)
    alen, blen = np.diff(arp64), np.diff(brp64)
    # row pointers by the closed form
    exp_rp = (arp64[:-1, None] * nnz + alen[:, None] * brp64[None, :-1]).ravel()
    assert np.array_equal(rp[:-1].astype(np.int64), exp_rp) and int(rp[-1]) == nnz * nnz
    del exp_rp
    # columns and values: per row of A, every (entry of that row, entry of B) pair at its closed-form position
    brow = np.repeat(np.arange(n), blen)                            # row of each entry of B
    bpos = np.arange(nnz) - brp64[brow]                             # ... and its position in that row
    bcol64 = bcol.astype(np.int64)
    seen = 0
    for ia in np.flatnonzero(alen):
        la, start = int(alen[ia]), int(arp64[ia]) * nnz
        base = start + la * brp64[brow] + bpos
        for ka in range(la):
            e = int(arp64[ia]) + ka
            dst = base + ka * blen[brow]
            assert np.array_equal(col[dst].astype(np.int64), int(acol[e]) * n + bcol64), (ia, ka)
            assert np.array_equal(val[dst], aval[e] * bval), (ia, ka)
            seen += nnz
    assert seen == nnz * nnz
    # sorted rows: columns increase strictly except across a row boundary
    ends = np.unique(rp[1:-1].astype(np.int64))
    ends = ends[(ends > 0) & (ends < nnz * nnz)]
    step = 1 << 24
    for lo in range(0, nnz * nnz - 1, step):
        hi = min(lo + step, nnz * nnz - 1)
        inc = col[lo + 1:hi + 1].astype(np.int64) > col[lo:hi].astype(np.int64)
        b = ends[(ends > lo) & (ends <= hi)] - 1 - lo
        inc[b] = True
        assert inc.all(), lo


# ---- 4. kronpow ----------------------------------------------------------------------------------------------------------------
def test_kronpow(gb, gpu):
    init = gb.Matrix.from_lists([0, 0, 1], [0, 1, 1], [0.77, 0.88, 0.99])
    assert init.kronpow(0).iseq(gb.Matrix.identity(gb.FP64, 2))
    assert init.kronpow(1).iseq(init)
    p3 = init.kronpow(3)
    assert p3.shape == (16, 16) and p3.nvals == 81
    I, J, V = (np.array(x) for x in ([0, 0, 1], [0, 1, 1], [0.77, 0.88, 0.99]))
    n = 2
    for _ in range(3):                                              # three squarings with numpy float64: one product per squaring, in the same association
        I = (I[:, None] * n + I[None, :]).ravel(); J = (J[:, None] * n + J[None, :]).ravel(); V = (V[:, None] * V[None, :]).ravel()
        n *= n
    assert n == 256 and len(V) == 6561
    p5 = init.kronpow(5)
    assert gb.last_kernel_plan().startswith("kronecker<"), gb.last_kernel_plan()
    assert p5.type is gb.FP64 and p5.shape == (65536, 65536) and p5.nvals == 3 ** 16 == 43046721
    rp, col, val = p5.to_csr()
    key = ((I[:, None] * n + I[None, :]) * 65536 + (J[:, None] * n + J[None, :])).ravel()
    order = np.argsort(key, kind="stable")
    key = key[order]
    assert np.array_equal(col, (key & 0xFFFF).astype(np.uint32))
    assert np.array_equal(rp.astype(np.int64), np.searchsorted(key >> 16, np.arange(65537)))
    del key
    exp = (V[:, None] * V[None, :]).ravel()[order]
    assert val.dtype == np.float64 and np.array_equal(val.view(np.uint64), exp.view(np.uint64))      # bit for bit


# ---- 5. the other C entry points ---------------------------------------------------------------------------------------------
def test_monoid_semiring_and_gxb_forms(gb, gpu):
    rng = np.random.default_rng(9)
    AI, AJ, AX = random_tuples(rng, gb, "INT32", 6, 5, 0.4)
    BI, BJ, BX = random_tuples(rng, gb, "INT32", 4, 7, 0.4)
    for route in ROUTES:
        with env(GRB_MI355X_KRON=route):
            A = gb.Matrix.from_arrays(AI, AJ, AX, 6, 5, gb.INT32)
            B = gb.Matrix.from_arrays(BI, BJ, BX, 4, 7, gb.INT32)
            forms = [("GrB_Matrix_kronecker_Monoid", gb.INT32.PLUS_MONOID, gb.INT32.PLUS), ("GrB_Matrix_kronecker_Semiring", gb.INT32.PLUS_TIMES, gb.INT32.TIMES),
                     ("GxB_kron", gb.INT32.MIN, gb.INT32.MIN)]
            for name, handle, binary in forms:
                exp = A.kronecker(B, op=binary)
                out = gb.Matrix.sparse(gb.INT32, 24, 35)
                info = getattr(gb.lib, name)(out._h, None, None, C.c_void_p(handle.get_op()), A._h, B._h, None)
                assert info == 0, (name, info)
                if route == 1:
                    assert gb.last_kernel_plan().startswith("kronecker<op="), gb.last_kernel_plan()
                assert exp.nvals == len(AX) * len(BX)
                same(out.to_arrays(), exp.to_arrays(), f"{name} on route {route}")
            assert getattr(gb.lib, "GrB_Matrix_kronecker_Monoid")(out._h, None, None, None, A._h, B._h, None) == 4      # GrB_NULL_POINTER


# ---- 6. errors keep their codes ------------------------------------------------------------------------------------------------
def test_dimension_mismatch_on_both_routes(gb, gpu):
    A = gb.Matrix.from_lists([0, 1], [1, 0], [2, 3], 2, 2, gb.INT64)
    B = gb.Matrix.from_lists([0, 2], [1, 0], [5, 6], 3, 2, gb.INT64)
    for route in (0, 1, None):
        with env(GRB_MI355X_KRON=route):
            for shape in ((6, 5), (5, 4), (4, 6)):
                out = gb.Matrix.from_lists([0], [0], [9], shape[0], shape[1], gb.INT64)
                with pytest.raises(gb.DimensionMismatch):
                    A.kronecker(B, out=out)
                assert out.to_lists() == [[0], [0], [9]]
            with pytest.raises(gb.DimensionMismatch):
                A.kronecker(B, mask=gb.Matrix.sparse(gb.BOOL, 6, 5))
            with pytest.raises(gb.DimensionMismatch):
                A.kronecker(B, out=gb.Matrix.sparse(gb.INT64, 6, 4), desc=gb.descriptor.T1)      # op(B) is 2 x 3: 4 x 6


def test_over_wide_product_is_declined(gb, gpu):
    """Dimensions that multiply past 2^32: the device route declines (the output is hypersparse), the host route gives the four entries."""
    n = 70000
    A = gb.Matrix.from_lists([0, n - 1], [1, n - 1], [2, 3], n, n, gb.INT64)
    B = gb.Matrix.from_lists([5, n - 1], [0, n - 1], [5, 7], n, n, gb.INT64)
    for route in (1, None):
        other_plan(gb)
        with env(GRB_MI355X_KRON=route):
            K = A.kronecker(B)
            assert not gb.last_kernel_plan().startswith("kronecker<"), gb.last_kernel_plan()
        assert K.shape == (n * n, n * n) and K.nvals == 4
        assert K.to_lists() == [[5, n - 1, (n - 1) * n + 5, n * n - 1], [n, n + n - 1, (n - 1) * n, n * n - 1], [10, 14, 15, 21]]
