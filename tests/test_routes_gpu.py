"""Host route or device route: the one policy of grb_route.hpp as every container operation applies it, on the device.

For each operation (index-list extract and assign in their vector, matrix and line forms, kronecker, the two diagonal forms, matrix and vector sort) the cases are:
a host-resident operand one entry below the operation's threshold with the hook unset (host route), the same operand at the threshold (device route), an operand
that lives in HBM only with one entry (device route), the hook at 0 at the threshold (host route), the hook at 1 with one entry (device route), and a co-operand
without an HBM layout — a complex mask, or hypersparse dimensions — under the hook at 1 (host route).  The route is read from the plan string: a sentinel plan
is left before the call, and the device route is the one that replaces it with the operation's own word.  Every case is compared with the opposite route's result on
the same input (with the same route's, where only one is legal): these operations move values and do not round, so the comparison is of bits.

The thresholds are written out here as they stand in pygraphblas_amd/csrc/grb_route.hpp (tests/route_policy_check.cpp holds them to these values without a
device).  GrB_Row_assign's 3 000 000 is covered there only: a matrix of that size is not built here, and the row form has the hook and residency cases."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# grb_route.hpp
EXTRACT_MIN, ASSIGN_MATRIX_MIN, ASSIGN_COL_MIN, ASSIGN_VECTOR_MIN, KRON_MIN, DIAG_MATRIX_MIN, DIAG_VECTOR_MIN, SORT_MIN = 10000, 30000, 100000, 500, 1000, 1000, 10000, 10000
NCOLS = 16                          # the matrices hold entries k -> (k // 16, k % 16): rows of 16, one wave each in the sort


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


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def sentinel(gb):
    """Some other plan string: the host routes of extract, assign and kronecker leave the last one alone, those of diag and sort clear it."""
    ones = gb.Vector.from_arrays(np.arange(3, dtype=np.uint64), np.ones(3, np.int32), 3, gb.INT32)
    gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1, 2, 3], 3, 3, gb.INT32).mxv(ones, semiring=gb.INT32.PLUS_TIMES)
    assert gb.last_kernel_plan() and not re.match(r"(extract|assign|kronecker|diag|sort|topk)", gb.last_kernel_plan())


def vals(n, seed=0):
    return (np.arange(n, dtype=np.float64) * 0.5 - 3.0) * (1 + seed)      # fractions and negative numbers, no two equal


def vector(gb, state, n, size=None, seed=0):
    """n entries at 0 .. n - 1 of a vector of `size` (default n + 3) positions; "host": built on the host mirror, "hbm": imported straight into HBM."""
    size = n + 3 if size is None else size
    if state == "host":
        with env(GRB_MI355X_BUILD=0):
            v = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), vals(n, seed), size, gb.FP64)
        assert residency(gb, v) == 1
        return v
    dense, present = np.zeros(size), np.zeros(size, np.uint8)
    dense[:n] = vals(n, seed); present[:n] = 1
    v = gb.Vector.from_dense_array(dense, gb.FP64, present=present)
    assert residency(gb, v) == 2
    return v


def matrix(gb, state, n, nrows=None, ncols=NCOLS, seed=0):
    """n entries at (k // ncols, k % ncols) of a matrix with `nrows` (default: what they need, plus two empty ones) rows."""
    k = np.arange(n, dtype=np.uint64)
    nrows = n // ncols + 3 if nrows is None else nrows
    if state == "host":
        with env(GRB_MI355X_BUILD=0):
            A = gb.Matrix.from_arrays(k // np.uint64(ncols), k % np.uint64(ncols), vals(n, seed), nrows, ncols, gb.FP64)
        assert residency(gb, A) == 1
        return A
    rowptr = np.minimum(np.arange(nrows + 1, dtype=np.int64) * ncols, n).astype(np.uint32)
    A = gb.Matrix.from_csr(gb.FP64, nrows, ncols, rowptr, (k % np.uint64(ncols)).astype(np.uint32), vals(n, seed))
    assert residency(gb, A) == 2
    return A


class FC64(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


def complex_mask(gb, nrows, ncols=None):
    """A GxB_FC64 container with entries at its first and last position, made through the C interface (the Python surface has no complex types): no HBM layout.
    Used as a structural mask."""
    lib, u64 = gb.lib, C.c_uint64
    fc64 = C.c_void_p.in_dll(lib, "GxB_FC64")
    h = C.c_void_p()
    if ncols is None:
        lib.GxB_Vector_setElement_FC64.argtypes = [C.c_void_p, FC64, u64]
        assert lib.GrB_Vector_new(C.byref(h), fc64, u64(nrows)) == 0
        for i in (0, nrows - 1):
            assert lib.GxB_Vector_setElement_FC64(h, FC64(1.0, -1.0), i) == 0
        return gb.Vector(h, gb.FP64)
    lib.GxB_Matrix_setElement_FC64.argtypes = [C.c_void_p, FC64, u64, u64]
    assert lib.GrB_Matrix_new(C.byref(h), fc64, u64(nrows), u64(ncols)) == 0
    for i, j in ((0, 0), (nrows - 1, ncols - 1)):
        assert lib.GxB_Matrix_setElement_FC64(h, FC64(1.0, -1.0), i, j) == 0
    return gb.Matrix(h, gb.FP64)


def arrays(*objs):
    out = []
    for o in objs:
        out.extend(o.to_arrays())
    return out


# ---- the operations.  Each takes (gb, state, n, incapable) and returns the arrays of its result; `n` is the entry count of the container that the route is
# decided on, `incapable` adds the co-operand that has no HBM layout ----------------------------------------------------------------------------------------------
def op_vector_extract(gb, state, n, incapable):
    u = vector(gb, state, n)
    idx = [0, n - 1, 0, u.size - 1]
    mask = complex_mask(gb, len(idx)) if incapable else None
    return arrays(u.extract(idx, mask=mask, desc=gb.descriptor.S if incapable else None))


def op_matrix_extract(gb, state, n, incapable):
    A = matrix(gb, state, n)
    rows = [A.nrows - 1, 0, (n - 1) // NCOLS, 0]
    mask = complex_mask(gb, len(rows), 9) if incapable else None
    return arrays(A.extract_matrix(rows, slice(0, 8), mask=mask, desc=gb.descriptor.S if incapable else None))


def op_vector_assign(gb, state, n, incapable):
    w, u = vector(gb, state, n), vector(gb, "host", 2, size=3, seed=1)
    w.assign(u, [w.size - 1, 0, w.size - 2], mask=complex_mask(gb, w.size) if incapable else None, desc=gb.descriptor.S if incapable else None)
    return arrays(w)


def op_matrix_assign(gb, state, n, incapable):
    Cm, B = matrix(gb, state, n), matrix(gb, "host", 5, nrows=3, ncols=4, seed=1)
    Cm.assign_matrix(B, [Cm.nrows - 1, 0, Cm.nrows - 2], [1, 5, 9, 15], mask=complex_mask(gb, Cm.nrows, NCOLS) if incapable else None, desc=gb.descriptor.S if incapable else None)
    return arrays(Cm)


def op_col_assign(gb, state, n, incapable):
    Cm = matrix(gb, state, n)
    u = vector(gb, "host", 2, size=Cm.nrows, seed=1)
    Cm.assign_col(3, u, mask=complex_mask(gb, Cm.nrows) if incapable else None, desc=gb.descriptor.S if incapable else None)
    return arrays(Cm)


def op_row_assign(gb, state, n, incapable):
    Cm = matrix(gb, state, n)
    u = vector(gb, "host", 5, size=NCOLS, seed=1)
    Cm.assign_row(Cm.nrows - 1, u, mask=complex_mask(gb, NCOLS) if incapable else None, desc=gb.descriptor.S if incapable else None)
    return arrays(Cm)


def kron_factors(n):
    """nnz(A) x nnz(B) == n with both factors small: the route is decided on the product."""
    a = next(a for a in range(int(n ** 0.5), 0, -1) if n % a == 0)
    return a, n // a


def op_kron(gb, state, n, incapable):
    na, nb = kron_factors(n)
    A, B = matrix(gb, state, na, nrows=7, ncols=8), matrix(gb, "host", nb, nrows=7, ncols=8, seed=1)
    mask = complex_mask(gb, 49, 64) if incapable else None
    return arrays(A.kronecker(B, op=gb.FP64.TIMES, mask=mask, desc=gb.descriptor.S if incapable else None))


def op_diag_matrix(gb, state, n, incapable):
    if incapable:                                                       # C must be square of size(v): hypersparse dimensions on both
        v = gb.Vector.sparse(gb.FP64)
        v[5] = 2.5
        return arrays(gb.Matrix.from_diag(v))
    return arrays(gb.Matrix.from_diag(vector(gb, state, n), 2))


def op_diag_vector(gb, state, n, incapable):
    if incapable:
        A = gb.Matrix.sparse(gb.FP64)
        A[5, 5] = 2.5
        return arrays(A.vector_diag())
    return arrays(matrix(gb, state, n).vector_diag(1))


def op_matrix_sort(gb, state, n, incapable):
    if incapable:                                                       # the outputs have A's dimensions
        A = gb.Matrix.sparse(gb.FP64)
        A[5, 7] = 2.5; A[5, 2] = -1.0
        return arrays(*A.sort(op=gb.FP64.GT))
    return arrays(*matrix(gb, state, n).sort(op=gb.FP64.GT))


def op_vector_sort(gb, state, n, incapable):
    if incapable:
        u = gb.Vector.sparse(gb.FP64)
        u[7] = 2.5; u[2] = -1.0
        return arrays(*u.sort(op=gb.FP64.GT))
    return arrays(*vector(gb, state, n).sort(op=gb.FP64.GT))


#       name              hook                    min                word of the device route's plan   the call     cases at the threshold
OPS = [("vector_extract", "GRB_MI355X_EXTRACT", EXTRACT_MIN,       "extract_vector<",                op_vector_extract, True),
       ("matrix_extract", "GRB_MI355X_EXTRACT", EXTRACT_MIN,       "extract_matrix<",                op_matrix_extract, True),
       ("vector_assign",  "GRB_MI355X_ASSIGN",  ASSIGN_VECTOR_MIN, "assign_vector<",                 op_vector_assign,  True),
       ("matrix_assign",  "GRB_MI355X_ASSIGN",  ASSIGN_MATRIX_MIN, "assign_matrix<",                 op_matrix_assign,  True),
       ("col_assign",     "GRB_MI355X_ASSIGN",  ASSIGN_COL_MIN,    "assign_col<",                    op_col_assign,     True),
       ("row_assign",     "GRB_MI355X_ASSIGN",  64,                "assign_row<",                    op_row_assign,     False),     # (3 000 000: the truth table only)
       ("kron",           "GRB_MI355X_KRON",    KRON_MIN,          "kronecker<",                     op_kron,           True),
       ("diag_matrix",    "GRB_MI355X_DIAG",    DIAG_MATRIX_MIN,   "diag_matrix<",                   op_diag_matrix,    True),
       ("diag_vector",    "GRB_MI355X_DIAG",    DIAG_VECTOR_MIN,   "diag_vector<",                   op_diag_vector,    True),
       ("matrix_sort",    "GRB_MI355X_SORT",    SORT_MIN,          "sort<on=matrix,",                op_matrix_sort,    True),
       ("vector_sort",    "GRB_MI355X_SORT",    SORT_MIN,          "sort<on=vector,",                op_vector_sort,    True)]
#        case            hook   state   entries (of min)   incapable   device route expected
CASES = [("below-min",   None,  "host", lambda m: m - 1,   False,      False),
         ("at-min",      None,  "host", lambda m: m,       False,      True),
         ("hbm-only",    None,  "hbm",  lambda m: 1,       False,      True),
         ("hook-0",      0,     "host", lambda m: m,       False,      False),
         ("hook-1",      1,     "host", lambda m: 1,       False,      True),
         ("incapable",   1,     "host", lambda m: 64,      True,       False)]


def run(gb, hook_name, hook, word, call, state, n, incapable):
    sentinel(gb)
    with env(**{hook_name: hook}):
        got = call(gb, state, n, incapable)
        plan = gb.last_kernel_plan()
    return got, plan.startswith(word), plan


def same(got, exp, what):
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g.view(np.uint8), e.view(np.uint8)), f"{what}: got {g[:8]} expected {e[:8]} (lengths {g.shape} / {e.shape})"


# (GrB_Row_assign has no case at its threshold: 3 000 000 entries, checked by tests/route_policy_check.cpp)
PAIRS = [(o, c) for o in OPS for c in CASES if o[5] or c[0] not in ("below-min", "at-min")]


@pytest.mark.parametrize("op,case", PAIRS, ids=[o[0] + "-" + c[0] for o, c in PAIRS])
def test_route_taken_and_both_routes_agree(gb, gpu, op, case):
    name, hook_name, minimum, word, call, _ = op
    label, hook, state, entries, incapable, device = case
    n = entries(minimum)
    got, on_device, plan = run(gb, hook_name, hook, word, call, state, n, incapable)
    assert on_device == device, (name, label, n, plan)
    other, other_on_device, plan = run(gb, hook_name, 0 if (device or incapable) else 1, word, call, state, n, incapable)
    assert other_on_device == (not device and not incapable), (name, label, n, plan)
    same(got, other, f"{name} {label}")


@pytest.mark.parametrize("form", ["matrix", "vector"])
def test_sort_prim_keeps_the_choice_by_size(gb, gpu, form):
    """GRB_MI355X_SORT=prim reads as "unset" for the route: host below the threshold, device from it on — there with every row in the segmented radix sort."""
    call, word = (op_matrix_sort, "sort<on=matrix,") if form == "matrix" else (op_vector_sort, "sort<on=vector,")
    below, on_device, plan = run(gb, "GRB_MI355X_SORT", "prim", word, call, "host", SORT_MIN - 1, False)
    assert not on_device and plan == "", plan
    at, on_device, plan = run(gb, "GRB_MI355X_SORT", "prim", word, call, "host", SORT_MIN, False)
    assert on_device, plan
    if form == "matrix":
        m = re.search(r"wave=(\d+),lds=(\d+),prim=(\d+)", plan)
        assert m and tuple(int(g) for g in m.groups()) == (0, 0, SORT_MIN // NCOLS + 3), plan
    for got, n in ((below, SORT_MIN - 1), (at, SORT_MIN)):
        other, other_on_device, plan = run(gb, "GRB_MI355X_SORT", 1 if n < SORT_MIN else 0, word, call, "host", n, False)
        assert other_on_device == (n < SORT_MIN), plan
        same(got, other, f"{form} sort under prim, {n} entries")
