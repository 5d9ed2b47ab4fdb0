"""Index-list assign on the device (grb_assign.hip behind GrB_Matrix_assign / GrB_Row_assign / GrB_Col_assign / GrB_Vector_assign).

Three references, none of them the code under test:
  * a dict model of the C API 1.3 rule written here: T = op(A) moved to (I[a], J[b]); without an accumulator Z = (C without its entries
    inside I x J) u T, with one Z = accum(C, T) on the union of the patterns; then C<M, replace> = Z, the mask and `replace` spanning all of
    C (matrix / vector assign) or only row i / column j (row / column assign);
  * numpy set operations on the keys i * ncols + j for the R-MAT-20 cases;
  * the forced host route (GRB_MI355X_ASSIGN=0): the code every earlier version ran.
Values are 0 .. 5 with explicit zeros, exact in all eleven types, so every comparison is bit-exact, floating point included.
"""
import contextlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROUTES = (0, 1)
TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
MASKS = [None, "valued", "structural", "complemented", "structural+complemented"]
ACCUMS = [None, "PLUS", "SECOND", "MIN"]


# ---- helpers (the same conventions as the extract tests) ---------------------------------------------------------------
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
    """0 .. 5 (BOOL: 0 / 1), explicit zeros included: exact in all eleven types, sums of two stay below 2^7."""
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    return rng.integers(0, 6, n).astype(npdt(gb, name))


def pick(kind, d, rng):
    """(argument for the Python surface, the positions it names) for one index kind over a dimension of d >= 1."""
    if kind == "all":
        return None, list(range(d))
    if kind in ("range", "stride", "backwards"):
        a, b = sorted(int(x) for x in rng.integers(0, d, 2))
        s = int(rng.integers(1, 5))
        if kind == "range":
            return slice(a, b), list(range(a, b + 1))                  # the reference's slices include their stop
        if kind == "stride":
            return slice(a, b, s), list(range(a, b + 1, s))
        return slice(b, a, -s), list(range(b, a - 1, -s))
    if kind == "increasing":
        k = int(rng.integers(1, d + 1))
        lst = np.sort(rng.choice(d, size=k, replace=False))
        return (lst.astype(np.int32) if k % 2 else [int(x) for x in lst]), [int(x) for x in lst]      # an ndarray of another dtype, or a list
    if kind == "shuffled":
        k = int(rng.integers(1, d + 1))
        lst = [int(x) for x in rng.permutation(d)[:k]]
        return lst, lst
    if kind == "repeats":
        k = int(rng.integers(2, d + 8))
        lst = [int(x) for x in rng.integers(0, d, k)]
        lst[-1] = lst[0]
        return lst, lst
    if kind == "empty":
        return [], []
    i = int(rng.integers(0, d))
    return [i], [i]


def random_tuples(rng, gb, name, nrows, ncols, density):
    total = nrows * ncols
    nnz = min(total, int(round(total * density)))
    flat = np.sort(rng.choice(total, size=nnz, replace=False)) if total else np.zeros(0, np.int64)
    I, J = (np.divmod(flat, ncols) if total else (flat, flat))
    return I.astype(np.uint64), J.astype(np.uint64), values(rng, gb, name, nnz)


def accum_op(name, a, b):
    if name == "SECOND":
        return b
    if a.dtype == np.bool_:
        return (a | b) if name == "PLUS" else (a & b)
    return (a + b).astype(a.dtype) if name == "PLUS" else min(a, b)


def as_sorted(d, cdt, vector=False):
    keys = sorted(d)
    X = np.array([d[k] for k in keys], dtype=cdt) if keys else np.zeros(0, cdt)
    if vector:
        return np.array([k[0] for k in keys], np.uint64), X
    return np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64), X


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and np.array_equal(g, e), f"{what}: got {g[:12]} expected {e[:12]} (lengths {g.shape} / {e.shape})"


def descriptor(gb, mask_kind, replace, t0):
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
    for p in parts:
        d = p if d is None else (d & p)
    return d

KINDS = ["all", "range", "stride", "backwards", "increasing", "shuffled", "empty", "single"]      # (a list with a repeat is undefined for assign: its own test below)


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_assign(C, cdt, A, rows, cols, M, mask_kind, accum, replace, scope=None):
    """C<M, replace>(rows, cols) = accum(C(rows, cols), A) on dicts.  A: {(a, b): value} of op(A).  scope: None (the mask is a matrix over all
    of C), ("row", i) or ("col", j) (the mask is a vector over that row / column, and `replace` touches nothing else)."""
    T = {(rows[a], cols[b]): np.asarray(v).astype(cdt)[()] for (a, b), v in A.items()}
    rset, cset = set(rows), set(cols)
    if accum:
        Z = dict(C)
        for p, t in T.items():
            Z[p] = accum_op(accum, Z[p], t) if p in Z else t
    else:
        Z = {p: v for p, v in C.items() if not (p[0] in rset and p[1] in cset)}
        Z.update(T)
    comp = mask_kind is not None and "complemented" in mask_kind
    structural = mask_kind is not None and "structural" in mask_kind

    def in_scope(p):
        return scope is None or (p[0] == scope[1] if scope[0] == "row" else p[1] == scope[1])

    def allows(p):
        if M is None:
            return not comp
        k = p if scope is None else ((p[1], 0) if scope[0] == "row" else (p[0], 0))
        return ((k in M) and (structural or bool(M[k]))) != comp
    out = {}
    for p, v in C.items():
        if not in_scope(p) or (not allows(p) and not replace):
            out[p] = v
    for p, v in Z.items():
        if in_scope(p) and allows(p):
            out[p] = v
    return out


def make_case(i, rng):
    c = {"atype": TYPES[i % 11], "rk": KINDS[i % 8], "ck": KINDS[(i // 8) % 8], "mask": MASKS[(i // 2) % 5], "accum": ACCUMS[(i // 3) % 4],
         "replace": (i // 5) % 2 == 1, "t0": (i // 7) % 2 == 1, "prefill": (i // 4) % 3 != 0}
    c["ctype"] = c["atype"] if i % 3 else TYPES[(i * 7 + 3) % 11]
    c["mtype"] = ["BOOL", "INT8", "FP32"][i % 3]
    c["nrows"], c["ncols"] = int(rng.integers(1, 40)), int(rng.integers(1, 30))
    c["density"] = float(rng.choice([0.1, 0.4, 1.0]))
    return c


def run_matrix_case(gb, c, rng):
    atype, ctype = c["atype"], c["ctype"]
    nr, nc = c["nrows"], c["ncols"]
    rarg, rows = pick(c["rk"], nr, rng)
    carg, cols = pick(c["ck"], nc, rng)
    m, n = len(rows), len(cols)
    am, an = (n, m) if c["t0"] else (m, n)                          # A's own shape: op(A) is |I| x |J|
    AI, AJ, AX = random_tuples(rng, gb, atype, am, an, c["density"])
    CI, CJ, CX = random_tuples(rng, gb, ctype, nr, nc, 0.3 if c["prefill"] else 0.0)
    MI, MJ, MX = random_tuples(rng, gb, c["mtype"], nr, nc, 0.5) if c["mask"] else (None, None, None)
    cdt = npdt(gb, ctype)
    Ad = {((int(b), int(a)) if c["t0"] else (int(a), int(b))): x for a, b, x in zip(AI, AJ, AX)}
    Cd = {(int(a), int(b)): x for a, b, x in zip(CI, CJ, CX)}
    Md = {(int(a), int(b)): x for a, b, x in zip(MI, MJ, MX)} if c["mask"] else None
    exp = as_sorted(model_assign(Cd, cdt, Ad, rows, cols, Md, c["mask"], c["accum"], c["replace"]), cdt)
    got = {}
    for route in ROUTES:
        A = gb.Matrix.from_arrays(AI, AJ, AX, am, an, typ(gb, atype))
        C = gb.Matrix.from_arrays(CI, CJ, CX, nr, nc, typ(gb, ctype))
        M = gb.Matrix.from_arrays(MI, MJ, MX, nr, nc, typ(gb, c["mtype"])) if c["mask"] else None
        acc = getattr(typ(gb, ctype), c["accum"]) if c["accum"] else None
        whole = c["rk"] == "all" and c["ck"] == "all" and acc is not None and M is None and not c["t0"]      # the eWiseAdd shortcut stays first
        with env(GRB_MI355X_ASSIGN=route):
            C.assign_matrix(A, rarg, carg, mask=M, accum=acc, desc=descriptor(gb, c["mask"], c["replace"], c["t0"]))
            plan = gb.last_kernel_plan()
        if route == 1 and not whole:
            assert plan.startswith("assign_matrix"), (plan, c)
        got[route] = C.to_arrays()
        same(got[route], exp, f"route {route} vs model, case {c}")
    same(got[ROUTES[-1]], got[0], f"device route vs host route, case {c}")
    return True


@pytest.mark.parametrize("block", range(8))
def test_parity_matrix(gb, gpu, block):
    rng = np.random.default_rng(11000 + block)
    ran = 0
    for i in range(block * 80, block * 80 + 80):                    # 640 cases: every (row kind, column kind) pair ten times
        ran += bool(run_matrix_case(gb, make_case(i, rng), rng))
    assert ran == 80


def run_line_case(gb, c, rng, which):
    """which: "row" (C(i, J) = u), "col" (C(I, j) = u) or "vector" (w(I) = u)."""
    atype, ctype = c["atype"], c["ctype"]
    cdt = npdt(gb, ctype)
    nr, nc = c["nrows"], c["ncols"]
    if which == "vector":
        nr, nc = nr * 3, 1
    length = nc if which == "row" else nr
    iarg, idx = pick(c["rk"], length, rng)
    k = len(idx)
    UI = np.sort(rng.choice(k, size=int(round(k * c["density"])), replace=False)).astype(np.uint64)
    UX = values(rng, gb, atype, len(UI))
    CI, CJ, CX = random_tuples(rng, gb, ctype, nr, nc, 0.3 if c["prefill"] else 0.0)
    MI = MX = None
    if c["mask"]:
        MI = np.sort(rng.choice(length, size=int(round(length * 0.5)), replace=False)).astype(np.uint64)
        MX = values(rng, gb, c["mtype"], len(MI))
    Md = {(int(a), 0): x for a, x in zip(MI, MX)} if c["mask"] else None
    Cd = {(int(a), int(b)): x for a, b, x in zip(CI, CJ, CX)}
    fixed = int(rng.integers(0, nr if which == "row" else nc))
    if which == "row":
        Ad, rows, cols, scope = {(0, int(a)): x for a, x in zip(UI, UX)}, [fixed], idx, ("row", fixed)
    elif which == "col":
        Ad, rows, cols, scope = {(int(a), 0): x for a, x in zip(UI, UX)}, idx, [fixed], ("col", fixed)
    else:
        Ad, rows, cols, scope = {(int(a), 0): x for a, x in zip(UI, UX)}, idx, [0], None
    exp = as_sorted(model_assign(Cd, cdt, Ad, rows, cols, Md, c["mask"], c["accum"], c["replace"], scope), cdt, vector=which == "vector")
    got = {}
    for route in ROUTES:
        u = gb.Vector.from_arrays(UI, UX, k, typ(gb, atype))
        M = gb.Vector.from_arrays(MI, MX, length, typ(gb, c["mtype"])) if c["mask"] else None
        acc = getattr(typ(gb, ctype), c["accum"]) if c["accum"] else None
        desc = descriptor(gb, c["mask"], c["replace"], False)
        if which == "vector":
            C = gb.Vector.from_arrays(CI, CX, nr, typ(gb, ctype))
        else:
            C = gb.Matrix.from_arrays(CI, CJ, CX, nr, nc, typ(gb, ctype))
        whole = which == "vector" and c["rk"] == "all" and acc is not None and M is None      # the eWiseAdd shortcut stays first
        with env(GRB_MI355X_ASSIGN=route):
            if which == "row":
                C.assign_row(fixed, u, iarg, mask=M, accum=acc, desc=desc)
            elif which == "col":
                C.assign_col(fixed, u, iarg, mask=M, accum=acc, desc=desc)
            else:
                C.assign(u, iarg, mask=M, accum=acc, desc=desc)
            plan = gb.last_kernel_plan()
        if route == 1 and not whole:
            assert plan.startswith("assign_" + which), (plan, c)
        got[route] = C.to_arrays()
        same(got[route], exp, f"{which}: route {route} vs model, case {c}")
    same(got[ROUTES[-1]], got[0], f"{which}: device route vs host route, case {c}")
    return True


@pytest.mark.parametrize("which", ["row", "col", "vector"])
@pytest.mark.parametrize("block", range(3))
def test_parity_line(gb, gpu, which, block):
    rng = np.random.default_rng(12000 + block + 10 * ["row", "col", "vector"].index(which))
    ran = 0
    for i in range(block * 96, block * 96 + 96):                    # 3 x 288 cases
        ran += bool(run_line_case(gb, make_case(i, rng), rng, which))
    assert ran == 96


# ---- 1. which route ---------------------------------------------------------------------------------------------------------
def small(gb):
    rng = np.random.default_rng(1)
    I, J, X = random_tuples(rng, gb, "INT32", 50, 40, 0.2)
    return I, J, X


def test_route_and_plan(gb, gpu):
    I, J, X = small(gb)
    ones = gb.Vector.from_arrays(np.arange(40, dtype=np.uint64), np.ones(40, np.int32), 40, gb.INT32)
    B = gb.Matrix.from_arrays(np.array([0, 1, 2], np.uint64), np.array([0, 3, 8], np.uint64), np.array([7, 8, 9], np.int32), 3, 10, gb.INT32)
    u40 = gb.Vector.from_arrays(np.arange(0, 40, 2, dtype=np.uint64), np.arange(20, dtype=np.int32), 40, gb.INT32)
    u50 = gb.Vector.from_arrays(np.arange(0, 50, 5, dtype=np.uint64), np.arange(10, dtype=np.int32), 50, gb.INT32)
    u3 = gb.Vector.from_arrays(np.array([0, 2], np.uint64), np.array([4, 5], np.int32), 3, gb.INT32)
    for route in ROUTES[::-1]:
        C = gb.Matrix.from_arrays(I, J, X, 50, 40, gb.INT32)
        w = gb.Vector.from_arrays(np.arange(0, 40, 2, dtype=np.uint64), np.arange(20, dtype=np.int32), 40, gb.INT32)
        calls = [("assign_matrix", lambda: C.assign_matrix(B, [3, 1, 2], slice(0, 9))), ("assign_row", lambda: C.assign_row(2, u40)), ("assign_col", lambda: C.assign_col(2, u50)),
                 ("assign_vector", lambda: w.assign(u3, [5, 4, 7]))]
        for name, call in calls:
            with env(GRB_MI355X_ASSIGN=route):
                C.mxv(ones, semiring=gb.INT32.PLUS_TIMES)          # some other plan in between
                call()
                plan = gb.last_kernel_plan()
            if route == 1:
                assert plan.startswith(name + "<"), (name, plan)
            else:
                assert not plan.startswith("assign_"), (name, plan)
    C = gb.Matrix.from_arrays(I, J, X, 50, 40, gb.INT32)
    with env(GRB_MI355X_ASSIGN=None):                               # a small host-resident matrix keeps the host route
        C.mxv(ones, semiring=gb.INT32.PLUS_TIMES)
        C.assign_matrix(B, [3, 1, 2], slice(0, 9))
        assert not gb.last_kernel_plan().startswith("assign_")
    with env(GRB_MI355X_ASSIGN=1):                                  # the plan names the index shapes, the row sort, the transpose and the accumulator
        C.assign_matrix(B, [3, 1, 2], slice(0, 9))
        assert "rows=list,cols=range,rowsort=0,transpose=0,accum=none" in gb.last_kernel_plan(), gb.last_kernel_plan()
        C.assign_matrix(B, slice(4, 6), [9, 8, 7, 6, 5, 4, 3, 2, 1, 0], accum=gb.INT32.PLUS)
        assert "rows=range,cols=list,rowsort=1" in gb.last_kernel_plan() and "accum=" in gb.last_kernel_plan() and "accum=none" not in gb.last_kernel_plan(), gb.last_kernel_plan()
        Bt = gb.Matrix.from_arrays(np.array([0, 3, 8], np.uint64), np.array([0, 1, 2], np.uint64), np.array([7, 8, 9], np.int32), 10, 3, gb.INT32)
        C.assign_matrix(Bt, [3, 1, 2], slice(0, 9), desc=gb.descriptor.T0)
        assert "transpose=1" in gb.last_kernel_plan()


def test_route_by_size_and_residency(gb, gpu):
    """Unset variable: an R-MAT-18 matrix (host mirror valid, on the device after an mxv) and a device-only result of extract_matrix take the device route."""
    from pygraphblas_amd import rmat
    import scipy.sparse as sp
    scale = 18
    n = 1 << scale
    rp, col = rmat.csr_numpy(scale, seed=42)
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    A = gb.Matrix.from_arrays(rows, col.astype(np.uint64), np.ones(len(col), np.float32), n, n, gb.FP32)
    x = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.ones(n, np.float32), n, gb.FP32)
    B = gb.Matrix.from_arrays(np.array([0, 1], np.uint64), np.array([1, 0], np.uint64), np.array([5, 6], np.float32), 2, 2, gb.FP32)
    with env(GRB_MI355X_ASSIGN=None, GRB_MI355X_EXTRACT=None):
        A.mxv(x, semiring=gb.FP32.PLUS_TIMES)
        A.assign_matrix(B, [7, 3], [2, 9])
        assert gb.last_kernel_plan().startswith("assign_matrix"), gb.last_kernel_plan()
        S = sp.csr_matrix((np.ones(len(col), np.float32), col.astype(np.int64), rp.astype(np.int64)), shape=(n, n)).tolil()
        S[7, 2] = 0; S[7, 9] = 5; S[3, 2] = 6; S[3, 9] = 0
        keys = set(zip(*S.nonzero()))
        sub = A.extract_matrix(slice(0, 99), slice(0, 99))          # device-only and small
        assert gb.last_kernel_plan().startswith("extract_matrix")
        gi, gj, gx = sub.to_arrays()
        exp = sorted((i, j) for i, j in keys if i < 100 and j < 100)
        assert [(int(a), int(b)) for a, b in zip(gi, gj)] == exp
        assert {(int(a), int(b)): float(v) for a, b, v in zip(gi, gj, gx)}.get((7, 9)) == 5.0
        sub2 = A.extract_matrix(slice(0, 99), slice(0, 99))
        sub2.assign_matrix(B, [0, 1], [0, 1])
        assert gb.last_kernel_plan().startswith("assign_matrix"), gb.last_kernel_plan()
        d = {(int(a), int(b)): float(v) for a, b, v in zip(*sub2.to_arrays())}
        assert d.get((0, 1)) == 5.0 and d.get((1, 0)) == 6.0 and (0, 0) not in d and (1, 1) not in d


def test_host_route_when_the_device_route_is_not_defined(gb, gpu):
    """A list with a repeat, an operand that is the output, and a complex container keep the host route under GRB_MI355X_ASSIGN=1, with the host result."""
    I, J, X = small(gb)
    B = gb.Matrix.from_arrays(np.array([0, 1, 2], np.uint64), np.array([0, 1, 2], np.uint64), np.array([7, 8, 9], np.int32), 3, 3, gb.INT32)
    u3 = gb.Vector.from_arrays(np.array([0, 1, 2], np.uint64), np.array([4, 5, 6], np.int32), 3, gb.INT32)
    ones = gb.Vector.from_arrays(np.arange(40, dtype=np.uint64), np.ones(40, np.int32), 40, gb.INT32)
    got = {}
    for route in ROUTES:
        with env(GRB_MI355X_ASSIGN=route):
            C = gb.Matrix.from_arrays(I, J, X, 50, 40, gb.INT32)
            w = gb.Vector.from_arrays(np.arange(0, 40, 2, dtype=np.uint64), np.arange(20, dtype=np.int32), 40, gb.INT32)
            plans = []
            for call in (lambda: C.assign_matrix(B, [3, 1, 3], [0, 1, 2]), lambda: C.assign_matrix(B, [0, 1, 2], [5, 6, 5]), lambda: C.assign_row(4, u3, [9, 9, 1]),
                         lambda: C.assign_col(4, u3, [9, 2, 9]), lambda: w.assign(u3, [8, 8, 3])):
                C.mxv(ones, semiring=gb.INT32.PLUS_TIMES)
                call()
                plans.append(gb.last_kernel_plan())
            assert not any(p.startswith("assign_") for p in plans), plans
            sq = gb.Matrix.from_arrays(np.array([0, 1, 2], np.uint64), np.array([1, 2, 0], np.uint64), np.array([1, 2, 3], np.int32), 3, 3, gb.INT32)
            sq.mxv(gb.Vector.from_arrays(np.arange(3, dtype=np.uint64), np.ones(3, np.int32), 3, gb.INT32), semiring=gb.INT32.PLUS_TIMES)
            sq.assign_matrix(sq, [2, 0, 1], None)                   # the operand is the output
            assert not gb.last_kernel_plan().startswith("assign_")
            got[route] = (C.to_arrays(), w.to_arrays(), sq.to_arrays(), complex_assign(gb))
    for a, b in zip(got[0][:3], got[1][:3]):
        same(a, b, "host route taken under =1")
    assert got[0][3] == got[1][3] == (2, 3.0, -1.0), got


def complex_assign(gb):
    """Z(1:3:2, 0:2:2) = Y on FC64 containers, through the C interface (the Python surface has no complex types): (nvals(Z), Z(1, 2))."""
    import ctypes as C

    class FC64(C.Structure):
        _fields_ = [("re", C.c_double), ("im", C.c_double)]
    lib, u64 = gb.lib, C.c_uint64
    fc64 = C.c_void_p.in_dll(lib, "GxB_FC64")
    lib.GxB_Matrix_setElement_FC64.argtypes = [C.c_void_p, FC64, u64, u64]
    Z, Y = C.c_void_p(), C.c_void_p()
    assert lib.GrB_Matrix_new(C.byref(Z), fc64, u64(4), u64(4)) == 0 and lib.GrB_Matrix_new(C.byref(Y), fc64, u64(2), u64(2)) == 0
    assert lib.GxB_Matrix_setElement_FC64(Z, FC64(1.0, 2.0), 1, 0) == 0 and lib.GxB_Matrix_setElement_FC64(Z, FC64(5.0, 5.0), 0, 0) == 0
    assert lib.GxB_Matrix_setElement_FC64(Y, FC64(3.0, -1.0), 0, 1) == 0
    rows, cols = (u64 * 2)(1, 3), (u64 * 2)(0, 2)
    ones = gb.Vector.from_arrays(np.arange(3, dtype=np.uint64), np.ones(3, np.int32), 3, gb.INT32)
    gb.Matrix.from_arrays(np.array([0], np.uint64), np.array([1], np.uint64), np.array([1], np.int32), 3, 3, gb.INT32).mxv(ones, semiring=gb.INT32.PLUS_TIMES)
    assert lib.GrB_Matrix_assign(Z, None, None, Y, rows, u64(2), cols, u64(2), None) == 0
    assert not gb.last_kernel_plan().startswith("assign_")
    nv, x = u64(0), FC64()
    assert lib.GrB_Matrix_nvals(C.byref(nv), Z) == 0 and lib.GxB_Matrix_extractElement_FC64(C.byref(x), Z, u64(1), u64(2)) == 0
    return int(nv.value), x.re, x.im


def test_accumulator_of_another_domain(gb, gpu):
    """INT64 containers under FP32.PLUS: the touched entries go through FP32 as the host's `combine` does, every other value keeps its bits
    (2^40 + 1 is not an FP32 number) — for the vector, the row and the column form; both routes and the rule."""
    big = (1 << 40) + 1
    n = 12
    idx = [7, 2, 9]
    got = {}
    for route in ROUTES:
        with env(GRB_MI355X_ASSIGN=route):
            w = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.array([big + i for i in range(n)], np.int64), n, gb.INT64)
            w[2] = 5
            u = gb.Vector.from_arrays(np.array([0, 1], np.uint64), np.array([3, 4], np.int64), 3, gb.INT64)
            m = gb.Vector.from_arrays(np.arange(0, n, 3, dtype=np.uint64), np.ones(4, np.bool_), n, gb.BOOL)
            w.assign(u, idx, accum=gb.FP32.PLUS)
            plans = [gb.last_kernel_plan()]
            C = gb.Matrix.from_arrays(np.repeat(np.arange(3, dtype=np.uint64), n), np.tile(np.arange(n, dtype=np.uint64), 3), np.array([big + i for i in range(3 * n)], np.int64), 3, n, gb.INT64)
            C[1, 2] = 5
            C.assign_row(1, u, idx, accum=gb.FP32.PLUS)
            plans.append(gb.last_kernel_plan())
            D = gb.Matrix.from_arrays(np.tile(np.arange(n, dtype=np.uint64), 3), np.repeat(np.arange(3, dtype=np.uint64), n), np.array([big + i for i in range(3 * n)], np.int64), n, 3, gb.INT64)
            D[2, 1] = 5
            D.assign_col(1, u, idx, mask=m, accum=gb.FP32.PLUS, desc=gb.descriptor.C)
            plans.append(gb.last_kernel_plan())
            if route == 1:
                assert [p.split("<")[0] for p in plans] == ["assign_vector", "assign_row", "assign_col"], plans
            got[route] = (w.to_arrays(), C.to_arrays(), D.to_arrays())
    f32 = lambda a, b: int(np.float32(np.float32(a) + np.float32(b)))
    ew = [big + i for i in range(n)]
    ew[2] = 5
    ew[7] = f32(ew[7], 3); ew[2] = f32(ew[2], 4)                   # u(2) is absent: w(9) is kept under an accumulator
    assert got[0][0][1].tolist() == ew
    rowvals = got[0][1][2].reshape(3, n)
    er = [big + n + i for i in range(n)]
    er[2] = 5
    er[7] = f32(er[7], 3); er[2] = f32(er[2], 4)
    assert rowvals[1].tolist() == er and rowvals[0].tolist() == [big + i for i in range(n)] and rowvals[2].tolist() == [big + 2 * n + i for i in range(n)]
    for a, b in zip(got[0], got[ROUTES[-1]]):
        same(a, b, "device route vs host route, accumulator of another domain")


# ---- 3. at scale ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat20():
    from pygraphblas_amd import rmat
    scale = 20
    n = 1 << scale
    rp, col = rmat.csr_numpy(scale, seed=42)
    vals = (np.arange(len(col), dtype=np.int64) % 251 + 1).astype(np.float32)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    return n, rp, col, vals, rows


def selections(n, rp, col):
    rng = np.random.default_rng(7)
    deg = np.diff(rp.astype(np.int64))
    hubs = np.argsort(-deg, kind="stable")[:64]
    nb = np.unique(np.concatenate([col[rp[h]:rp[h + 1]].astype(np.int64) for h in hubs[:4]] + [hubs]))
    sample = np.sort(rng.choice(n, size=n // 10, replace=False))
    shuffled = rng.permutation(sample)
    return {"range": (slice(0, n // 2 - 1), np.arange(n // 2)), "sorted sample": (sample, sample), "shuffled": (shuffled, shuffled), "hubs and neighbours": (nb, nb)}, hubs, deg


def csr_arrays(M, n):
    """(keys i * n + j, values) of a matrix, in row-major order"""
    i, j, x = M.to_arrays()
    return i.astype(np.int64) * n + j.astype(np.int64), x


@pytest.mark.parametrize("mode", ["plain", "masked replace", "masked replace plus"])
@pytest.mark.parametrize("which", ["range", "sorted sample", "shuffled", "hubs and neighbours"])
def test_rmat20_block_written_back(gb, gpu, rmat20, which, mode):
    n, rp, col, vals, rows = rmat20
    sel, hubs, deg = selections(n, rp, col)
    arg, idx = sel[which]
    if which == "hubs and neighbours":
        assert int((deg[hubs] >= 4096).sum()) >= 1 and set(hubs.tolist()) <= set(idx.tolist())
    inI = np.zeros(n, bool)
    inI[idx] = True
    region = inI[rows] & inI[col.astype(np.int64)]
    keys = rows * n + col.astype(np.int64)
    with env(GRB_MI355X_ASSIGN=None, GRB_MI355X_EXTRACT=None):
        C = gb.Matrix.from_csr(gb.FP32, n, n, rp, col, vals)         # lives in HBM only
        S = C.extract_matrix(arg, arg)
        assert gb.last_kernel_plan().startswith("extract_matrix")
        assert S.nvals == int(region.sum())
        if mode == "plain":
            C.assign_matrix(S, arg, arg)                            # the unchanged block: C bit for bit
            assert gb.last_kernel_plan().startswith("assign_matrix"), gb.last_kernel_plan()
            gk, gx = csr_arrays(C, n)
            assert np.array_equal(gk, keys) and np.array_equal(gx, vals)
            S2 = S.apply_second(gb.FP32.TIMES, 2.0)
            C.assign_matrix(S2, arg, arg)
            assert gb.last_kernel_plan().startswith("assign_matrix"), gb.last_kernel_plan()
            gk, gx = csr_arrays(C, n)
            assert np.array_equal(gk, keys)
            assert np.array_equal(gx, np.where(region, vals * 2, vals).astype(np.float32))
        else:
            S2 = S.apply_second(gb.FP32.TIMES, 2.0)
            even = (col & 1) == 0
            cs = np.concatenate([[0], np.cumsum(even)]).astype(np.int64)
            M = gb.Matrix.from_csr(gb.BOOL, n, n, cs[rp.astype(np.int64)], col[even], np.zeros(int(even.sum()), np.bool_))      # structural: its values are all false
            plus = mode.endswith("plus")                            # without the accumulator: region removal, union and the masked write-back of Z
            C.assign_matrix(S2, arg, arg, mask=M, accum=gb.FP32.PLUS if plus else None, desc=gb.descriptor.R & gb.descriptor.S)
            assert gb.last_kernel_plan().startswith("assign_matrix"), gb.last_kernel_plan()
            assert ("k_assign_region_keep" in gb.last_kernel_plan()) == (not plus)
            gk, gx = csr_arrays(C, n)
            assert np.array_equal(gk, keys[even])
            assert np.array_equal(gx, np.where(region, vals * (3 if plus else 2), vals).astype(np.float32)[even])


def test_rmat20_rows_and_columns(gb, gpu, rmat20):
    n, rp, col, vals, rows = rmat20
    deg = np.diff(rp.astype(np.int64))
    hub, leaf = int(np.argmax(deg)), int(np.flatnonzero(deg == 1)[0])
    keys = rows * n + col.astype(np.int64)
    vi = np.arange(0, n, 3, dtype=np.int64)
    vx = (vi % 5).astype(np.float32)
    v = gb.Vector.from_arrays(vi.astype(np.uint64), vx, n, gb.FP32)
    with env(GRB_MI355X_ASSIGN=None):
        for r in (hub, leaf):
            C = gb.Matrix.from_csr(gb.FP32, n, n, rp, col, vals)
            C.assign_row(r, v)
            assert gb.last_kernel_plan().startswith("assign_row"), gb.last_kernel_plan()
            keep = rows != r
            ek = np.concatenate([keys[keep], r * n + vi]); ex = np.concatenate([vals[keep], vx])
            o = np.argsort(ek, kind="stable")
            gk, gx = csr_arrays(C, n)
            assert np.array_equal(gk, ek[o]) and np.array_equal(gx, ex[o]), f"row {r}"
            C = gb.Matrix.from_csr(gb.FP32, n, n, rp, col, vals)
            C.assign_col(r, v, accum=gb.FP32.PLUS)
            assert gb.last_kernel_plan().startswith("assign_col"), gb.last_kernel_plan()
            ck = vi * n + r                                         # keys is sorted (row-major): the column's entries that C already has, and the new ones
            pos = np.searchsorted(keys, ck)
            both = (pos < len(keys)) & (keys[np.minimum(pos, len(keys) - 1)] == ck)
            ex = vals.copy()
            ex[pos[both]] += vx[both]
            ek = np.concatenate([keys, ck[~both]]); ex = np.concatenate([ex, vx[~both]])
            o = np.argsort(ek, kind="stable")
            gk, gx = csr_arrays(C, n)
            assert np.array_equal(gk, ek[o]) and np.array_equal(gx, ex[o]), f"column {r}"


def test_vector_at_scale(gb, gpu):
    n = 1 << 22
    rng = np.random.default_rng(9)
    wi = np.flatnonzero(rng.random(n) < 0.5)
    wx = (wi % 6).astype(np.float64)
    idx = rng.permutation(n)[: n // 4]                              # a shuffled list without repeats
    ui = np.flatnonzero(rng.random(len(idx)) < 0.5)
    ux = (ui % 5).astype(np.float32)
    mi = np.flatnonzero(rng.random(n) < 0.7)
    dense_w = np.zeros(n); pres_w = np.zeros(n, bool); dense_w[wi] = wx; pres_w[wi] = True
    allow = np.zeros(n, bool); allow[mi] = True
    tgt = idx[ui]
    in_region = np.zeros(n, bool); in_region[idx] = True
    has_u = np.zeros(n, bool); has_u[tgt] = True
    uval = np.zeros(n); uval[tgt] = ux
    for accum in (None, "PLUS"):
        w = gb.Vector.from_arrays(wi.astype(np.uint64), wx, n, gb.FP64)
        u = gb.Vector.from_arrays(ui.astype(np.uint64), ux, len(idx), gb.FP32)
        m = gb.Vector.from_arrays(mi.astype(np.uint64), np.zeros(len(mi), np.bool_), n, gb.BOOL)
        with env(GRB_MI355X_ASSIGN=None):
            w.assign(u, idx, mask=m, accum=getattr(gb.FP64, accum) if accum else None, desc=gb.descriptor.S)
            assert gb.last_kernel_plan().startswith("assign_vector<index=list"), gb.last_kernel_plan()
        if accum:
            ev = np.where(allow & has_u, np.where(pres_w, dense_w + uval, uval), dense_w); ep = pres_w | (allow & has_u)
        else:
            ev = np.where(allow & has_u, uval, dense_w); ep = np.where(allow & in_region, has_u, pres_w)
        gi, gx = w.to_arrays()
        assert np.array_equal(gi, np.flatnonzero(ep).astype(np.uint64)) and np.array_equal(gx, ev[ep])


# ---- 4. errors: the same exception and message on both routes ----------------------------------------------------------------
def test_errors_unchanged(gb, gpu):
    import ctypes
    rng = np.random.default_rng(5)
    I, J, X = random_tuples(rng, gb, "INT64", 20, 10, 0.3)
    seen = {}
    for route in ROUTES:
        C = gb.Matrix.from_arrays(I, J, X, 20, 10, gb.INT64)
        B = gb.Matrix.sparse(gb.INT64, 2, 3)
        w = gb.Vector.from_arrays(np.arange(10, dtype=np.uint64), np.arange(10, dtype=np.int64), 10, gb.INT64)
        u2 = gb.Vector.sparse(gb.INT64, 2)
        u10 = gb.Vector.sparse(gb.INT64, 10)
        calls = {
            "matrix row index out of bounds": lambda: C.assign_matrix(B, [1, 20], [0, 1, 2]),
            "matrix column range out of bounds": lambda: C.assign_matrix(B, [1, 2], slice(8, 10)),
            "matrix wrong operand shape": lambda: C.assign_matrix(B, [1, 2, 3], [0, 1, 2]),
            "matrix mask shape": lambda: C.assign_matrix(B, [1, 2], [0, 1, 2], mask=gb.Matrix.sparse(gb.BOOL, 20, 9)),
            "row index out of range": lambda: C.assign_row(20, u10),
            "row wrong operand size": lambda: C.assign_row(2, u2),
            "row list out of bounds": lambda: C.assign_row(2, u2, [0, 10]),
            "row mask size": lambda: C.assign_row(2, u10, mask=gb.Vector.sparse(gb.BOOL, 9)),
            "col index out of range": lambda: C.assign_col(10, u2, [0, 1]),
            "col wrong operand size": lambda: C.assign_col(1, u2),
            "col list out of bounds": lambda: C.assign_col(1, u2, [0, 20]),
            "col mask size": lambda: C.assign_col(1, u2, [0, 1], mask=gb.Vector.sparse(gb.BOOL, 19)),
            "vector index out of bounds": lambda: w.assign(u2, [3, 10]),
            "vector wrong operand size": lambda: w.assign(u2, [3, 4, 5]),
            "vector mask size": lambda: w.assign(u2, [3, 4], mask=gb.Vector.sparse(gb.BOOL, 5)),
            "NULL list": lambda: gb.base.check(gb.lib.GrB_Vector_assign(w._h, None, None, u2._h, None, ctypes.c_uint64(2), None), w),
        }
        with env(GRB_MI355X_ASSIGN=route):
            for name, call in calls.items():
                with pytest.raises(Exception) as e:
                    call()
                seen.setdefault(name, []).append((e.type, str(e.value)))
    for name, (host, device) in seen.items():
        assert host == device, (name, host, device)
        assert host[0].__module__.startswith("pygraphblas_amd"), (name, host)      # a GraphBLAS error of the package, not a Python accident


def test_uninitialised_operand(gb, gpu):
    import ctypes
    C = gb.Matrix.sparse(gb.INT64, 4, 4)
    junk = ctypes.create_string_buffer(512)
    seen = []
    for route in ROUTES:
        with env(GRB_MI355X_ASSIGN=route):
            seen.append(int(gb.lib.GrB_Matrix_assign(C._h, None, None, ctypes.cast(junk, ctypes.c_void_p), None, 4, None, 4, None)))
    assert seen[0] == seen[1] and seen[0] != 0, seen


# ---- 5. the reference's own assign examples ----------------------------------------------------------------------------------
def _key(k):
    if k is None:
        return slice(None)
    if isinstance(k, dict):
        return slice(*k["slice"])
    return k


def _container(gb, src):
    T = typ(gb, src["type"])
    if "J" in src:
        return gb.Matrix.from_arrays(np.array(src["I"], np.uint64), np.array(src["J"], np.uint64), np.array(src["V"], T._np), src["nrows"], src["ncols"], T)
    return gb.Vector.from_arrays(np.array(src["I"], np.uint64), np.array(src["V"], T._np), src["size"], T)


def test_reference_assign_examples(gb, gpu):
    with open(os.path.join(HERE, "golden", "reference_assign_vectors.json")) as f:
        doc = json.load(f)
    assert len(doc["cases"]) >= 8
    for route in ROUTES:
        with env(GRB_MI355X_ASSIGN=route):
            for case in doc["cases"]:
                where = f"{case['source']} on route {route}"
                target, operand = _container(gb, case["target"]), _container(gb, case["operand"])
                key = [_key(k) for k in case["key"]]
                target[key[0] if len(key) == 1 else (key[0], key[1])] = operand
                e = case["expect"]
                if "J" in e:
                    same(target.to_arrays(), (np.array(e["I"], np.uint64), np.array(e["J"], np.uint64), np.array(e["V"], target.type._np)), where)
                else:
                    same(target.to_arrays(), (np.array(e["I"], np.uint64), np.array(e["V"], target.type._np)), where)
