"""User-defined select operators on the device: `@select_op` predicates and hand-written definitions through GxB_Matrix_select / GxB_Vector_select.

The model is the Python predicate itself, applied entry by entry on the host, and the C API's mask / replace / accumulator rule of
tests/test_userop_gpu.py (`model_write_back`, imported).  Select copies values, so EVERY comparison is exact: the same pattern and the same bits; there is no
tolerance anywhere.  Predicates that call the math library get values on a grid of multiples of 1/8 and a threshold at least 1/16 away from every f(x), so
the device's and the host's rounding cannot disagree about an entry; the test asserts that margin for its inputs."""
import ctypes as C
import math
import os
import subprocess
import sys
import zlib
from math import exp

import numpy as np
import pytest

import test_userop_gpu as U
from test_userop_gpu import got_dict, model_write_back, pyval, same_bits, to_type

pytestmark = pytest.mark.gpu

NPT = {"BOOL": np.bool_, "INT8": np.int8, "INT16": np.int16, "INT32": np.int32, "INT64": np.int64, "UINT64": np.uint64, "FP32": np.float32, "FP64": np.float64}
TYPES = list(NPT)
DIM_DEVICE_MAX = 0xFFFFFFF0                            # the widest container with an HBM layout (32-bit indices)


# ---- the predicates (module level: the translator reads their source) ------------------------------------------------------------------------------
def u_tril(i, j, x, v):
    return j - i <= v


def u_triu(i, j, x, v):
    return j - i >= v


def u_diag(i, j, x, v):
    return j - i == v


def u_offdiag(i, j, x, v):
    return j - i != v


def u_nonzero(i, j, x, v):
    return x != 0


def u_ne(i, j, x, v):
    return x != v


def u_eq(i, j, x, v):
    return x == v


def u_gt(i, j, x, v):
    return x > v


def u_ge(i, j, x, v):
    return x >= v


def u_lt(i, j, x, v):
    return x < v


def u_le(i, j, x, v):
    return x <= v


def mixed(i, j, x, v):
    return (i + j) % 3 == 0 and x * x > v


def softplus_above(i, j, x, v):
    return math.log1p(exp(x)) > v


def checker(i, j, x, v):
    return (i // 2 + j // 3) % 2 == 0


def always(i, j, x, v):
    return True


def never(i, j, x, v):
    return 0


def right_half(i, j, x, v):
    return j >= 2147483648


def hand(i, j, x, v):                                  # the Python model of HAND_DEFN below
    return abs(i - j) <= 2 and float(np.float32(x) * np.float32(2)) > float(v)


HAND_DEFN = ("static int close_by (GrB_Index a, GrB_Index b) { return a > b ? a - b <= 2 : b - a <= 2 ; }\n"
             "bool hand (GrB_Index i, GrB_Index j, const float *x, const int32_t *thunk) { return close_by (i, j) && (*x) * 2 > (float) (*thunk) ; }\n")

POSITIONAL = {"TRIL": u_tril, "TRIU": u_triu, "DIAG": u_diag, "OFFDIAG": u_offdiag}
VALUE = {"NONZERO": u_nonzero, "NE_THUNK": u_ne, "EQ_THUNK": u_eq, "GT_THUNK": u_gt, "GE_THUNK": u_ge, "LT_THUNK": u_lt, "LE_THUNK": u_le}
_OPS = {}


def sel(gb, func, typ, ttyp=None):
    key = (func.__name__, typ, ttyp)
    if key not in _OPS:
        _OPS[key] = gb.select_op(getattr(gb, typ), getattr(gb, ttyp) if ttyp else None)(func)
    return _OPS[key]


# ---- operands and the model --------------------------------------------------------------------------------------------------------------------------------
def edge_values(rng, typ, n):
    """Small values around the thunks used below; the floating-point types also get NaN, both zeros and both infinities."""
    if typ == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    if typ.startswith("FP"):
        pool = np.array([-2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 1.5, 3.0, np.nan, np.inf, -np.inf], dtype=NPT[typ])
        return pool[rng.integers(0, len(pool), n)]
    if typ == "UINT64":
        pool = np.array([0, 1, 2, 3, 7, 1 << 40], dtype=np.uint64)
        return pool[rng.integers(0, len(pool), n)]
    return rng.integers(-3, 4, n).astype(NPT[typ])


def mat_of(gb, typ, nr, nc, I, J, X):
    I, J = np.asarray(I, dtype=np.uint64), np.asarray(J, dtype=np.uint64)
    X = np.asarray(X, dtype=NPT[typ])
    d = {(int(i), int(j)): pyval(typ, x) for i, j, x in zip(I, J, X)}
    return gb.Matrix.from_arrays(I, J, X, nr, nc, getattr(gb, typ)), d


def rand_mat(gb, rng, typ, nr, nc, k, values=edge_values):
    flat = np.sort(rng.choice(nr * nc, size=k, replace=False))
    I, J = np.divmod(flat, nc)
    return mat_of(gb, typ, nr, nc, I, J, values(rng, typ, k))


def rand_vec(gb, rng, typ, n, k, values=edge_values):
    I = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint64)
    X = np.asarray(values(rng, typ, k), dtype=NPT[typ])
    return gb.Vector.from_arrays(I, X, n, getattr(gb, typ)), {int(i): pyval(typ, x) for i, x in zip(I, X)}


def model_select(func, xtyp, ttyp, Ad, thunk):
    """The entries of A (a dict) the predicate keeps: it sees the value cast into its type and the thunk cast into its thunk type; the kept value is A's own."""
    v = pyval(ttyp, to_type(ttyp, thunk if thunk is not None else 0))
    out = {}
    for p, a in Ad.items():
        i, j = p if isinstance(p, tuple) else (p, 0)
        if func(i, j, pyval(xtyp, to_type(xtyp, a)), v):
            out[p] = a
    return out


def assert_same(got, want, what):
    assert set(got) == set(want), f"{what}: pattern differs: {sorted(set(got) ^ set(want))[:8]}"
    for p in want:
        assert same_bits(got[p], want[p]), f"{what}: entry {p}: got {got[p]!r}, expected {want[p]!r} (bit-exact required)"


def plan_of(gb, func, xtyp, ttyp, on):
    return f"userselect<name={func.__name__},xtype=GrB_{xtyp},ttype=GrB_{ttyp},on={on}> grb_userselect"


def stats(gb):
    c, d, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert gb.lib.GrBX_userop_stats(C.byref(c), C.byref(d), C.byref(n)) == 0
    return c.value, d.value, n.value


def new_selectop(gb, xtyp, ttyp, name, defn):
    h = C.c_void_p()
    assert gb.lib.GxB_SelectOp_new(C.byref(h), None, C.c_void_p(getattr(gb, xtyp)._h), C.c_void_p(getattr(gb, ttyp)._h) if ttyp else None, name.encode(), defn.encode()) == 0
    return h


def select_raw(gb, A, oph, thunk_handle, out, mask=None, accum=None, desc=None):
    """The C entry point itself (a thunk of any type, an operator made through the C ABI); returns GrB_Info."""
    from pygraphblas_amd.matrix import get_args
    mh, ah, dh = get_args(mask, accum, desc)
    fn = gb.lib.GxB_Matrix_select if A._kind == "matrix" else gb.lib.GxB_Vector_select
    return fn(out._h, mh, ah, oph, A._h, thunk_handle, dh)


# ---- 1. parity with the built-in select operators ---------------------------------------------------------------------------------------------------
THUNK = {"BOOL": False, "UINT64": 2}


@pytest.mark.parametrize("typ", TYPES)
def test_parity_with_the_built_ins_on_a_matrix(gb, gpu, typ):
    rng = np.random.default_rng(zlib.crc32(f"parity matrix {typ}".encode()))
    A, Ad = rand_mat(gb, rng, typ, 37, 53, 37 * 53 * 2 // 5)
    for name, func in POSITIONAL.items():
        op = sel(gb, func, typ, "INT64")
        for k in (-2, 0, 3):
            want = got_dict(A.select(name, k))
            got = A.select(op, k)
            assert gb.last_kernel_plan().startswith(plan_of(gb, func, typ, "INT64", "matrix"))
            assert_same(got_dict(got), want, f"{typ} user {name}({k}) against the built-in")
            assert 0 < len(want) < len(Ad)
    thunk = THUNK.get(typ, 1)
    for name, func in VALUE.items():
        op = sel(gb, func, typ)
        want = got_dict(A.select(name) if name == "NONZERO" else A.select(name, thunk))
        got = A.select(op) if name == "NONZERO" else A.select(op, thunk)
        assert gb.last_kernel_plan().startswith(plan_of(gb, func, typ, typ, "matrix"))
        assert_same(got_dict(got), want, f"{typ} user {name} against the built-in")
        assert got.type is A.type


@pytest.mark.parametrize("typ", TYPES)
def test_parity_with_the_built_ins_on_a_vector(gb, gpu, typ):
    rng = np.random.default_rng(zlib.crc32(f"parity vector {typ}".encode()))
    u, ud = rand_vec(gb, rng, typ, 301, 180)
    thunk = THUNK.get(typ, 1)
    for name, func in VALUE.items():
        op = sel(gb, func, typ)
        want = got_dict(u.select(name) if name == "NONZERO" else u.select(name, thunk))
        got = u.select(op) if name == "NONZERO" else u.select(op, thunk)
        assert gb.last_kernel_plan().startswith(plan_of(gb, func, typ, typ, "vector"))
        assert_same(got_dict(got), want, f"{typ} vector user {name} against the built-in")


# ---- 2. mixed predicates against the Python model ------------------------------------------------------------------------------------------------------
def grid_values(rng, typ, n):
    if typ.startswith("FP"):
        return (rng.integers(-24, 25, n) / 8.0).astype(NPT[typ])                     # multiples of 1/8 in [-3, 3]
    return rng.integers(-40, 41, n).astype(NPT[typ])


@pytest.mark.parametrize("typ", ["FP64", "FP32", "INT64", "INT8"])
def test_index_and_value_predicate_against_python(gb, gpu, typ):
    rng = np.random.default_rng(zlib.crc32(f"mixed {typ}".encode()))
    op = sel(gb, mixed, typ)
    thunk = 2.25 if typ.startswith("FP") else 9
    A, Ad = rand_mat(gb, rng, typ, 37, 53, 700, grid_values)
    want = model_select(mixed, typ, typ, Ad, thunk)
    assert 0 < len(want) < len(Ad)
    assert_same(got_dict(A.select(op, thunk)), want, f"{typ} matrix mixed")
    u, ud = rand_vec(gb, rng, typ, 1027, 600, grid_values)
    want = model_select(mixed, typ, typ, ud, thunk)                                  # (a vector's entry: j is 0)
    assert 0 < len(want) < len(ud)
    assert_same(got_dict(u.select(op, thunk)), want, f"{typ} vector mixed")


def half_steps(rng, typ, n):
    return (rng.integers(-6, 7, n) / 2.0).astype(NPT[typ])                           # multiples of 1/2 (so of 1/8) in [-3, 3]


@pytest.mark.parametrize("typ", ["FP64", "FP32"])
def test_math_library_predicate_with_a_safe_margin(gb, gpu, typ):
    rng = np.random.default_rng(11)
    op = sel(gb, softplus_above, typ)
    thunk = 0.8125                                                                   # between f(0) = 0.693 and f(0.5) = 0.974
    A, Ad = rand_mat(gb, rng, typ, 37, 53, 600, half_steps)
    u, ud = rand_vec(gb, rng, typ, 301, 200, half_steps)
    for x in list(Ad.values()) + list(ud.values()):
        assert x * 8 == int(x * 8) and abs(math.log1p(exp(x)) - thunk) >= 1 / 16, x      # the margin rule: no rounding can flip a decision
    want = model_select(softplus_above, typ, typ, Ad, thunk)
    assert 0 < len(want) < len(Ad)
    assert_same(got_dict(A.select(op, thunk)), want, f"{typ} matrix log1p(exp(x)) > v")
    assert_same(got_dict(u.select(op, thunk)), model_select(softplus_above, typ, typ, ud, thunk), f"{typ} vector log1p(exp(x)) > v")


def test_index_only_predicate(gb, gpu):
    rng = np.random.default_rng(12)
    op = sel(gb, checker, "BOOL")
    A, Ad = rand_mat(gb, rng, "BOOL", 37, 53, 900)
    want = model_select(checker, "BOOL", "BOOL", Ad, None)
    assert 0 < len(want) < len(Ad)
    assert_same(got_dict(A.select(op)), want, "checkerboard")


def test_hand_written_definition_with_a_helper_through_the_c_abi(gb, gpu):
    rng = np.random.default_rng(13)
    h = new_selectop(gb, "FP32", "INT32", "hand", HAND_DEFN)
    A, Ad = rand_mat(gb, rng, "FP32", 37, 53, 900, grid_values)
    out = gb.Matrix.sparse(gb.FP32, 37, 53)
    s = U.scalar_handle(gb, "INT32", 1)
    try:
        assert select_raw(gb, A, h, s, out) == 0
        assert gb.last_kernel_plan().startswith("userselect<name=hand,xtype=GrB_FP32,ttype=GrB_INT32,on=matrix> grb_userselect")
        want = model_select(hand, "FP32", "INT32", Ad, 1)
        assert 0 < len(want) < len(Ad)
        assert_same(got_dict(out), want, "hand-written definition")
    finally:
        gb.lib.GxB_Scalar_free(C.byref(s))
        assert gb.lib.GxB_SelectOp_free(C.byref(h)) == 0 and h.value is None


# ---- 3. variants on one rectangular matrix ------------------------------------------------------------------------------------------------------------------
# (name, mask: None | "value" | "struct", complemented, replace, accumulator PLUS, transposed input)
VARIANTS = [("plain", None, False, False, False, False), ("value mask", "value", False, False, False, False), ("structural mask", "struct", False, False, False, False),
            ("complemented mask", "value", True, False, False, False), ("complemented structural mask + replace", "struct", True, True, False, False),
            ("mask + replace", "value", False, True, False, False), ("accum PLUS", None, False, False, True, False), ("mask + accum PLUS", "value", False, False, True, False),
            ("transposed", None, False, False, False, True), ("transposed + mask + replace + accum", "struct", False, True, True, True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_variants_of_the_write_back(gb, gpu, variant):
    name, mask_kind, comp, replace, accum_plus, transposed = variant
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    typ, nr, nc, thunk = "FP64", 37, 53, 2.25
    op = sel(gb, mixed, typ)
    A, Ad = rand_mat(gb, rng, typ, nc if transposed else nr, nr if transposed else nc, 800, grid_values)
    if transposed:
        Ad = {(j, i): x for (i, j), x in Ad.items()}                                 # i and j are those of the transposed matrix
    Cm, Cd = rand_mat(gb, rng, typ, nr, nc, 500, grid_values)
    M, Md = rand_mat(gb, rng, "INT32", nr, nc, 900, grid_values) if mask_kind else (None, None)
    desc = U.descriptor(gb, mask_kind == "struct", comp, replace, transposed, False)
    T = model_select(mixed, typ, typ, Ad, thunk)
    assert 0 < len(T) < len(Ad)
    want = model_write_back(Cd, typ, T, typ, Md, mask_kind == "struct", comp, replace, accum_plus)
    A.select(op, thunk, out=Cm, mask=M, accum=gb.FP64.PLUS if accum_plus else None, desc=desc)
    assert_same(got_dict(Cm), want, f"select [{name}]")


def test_operand_of_another_type_keeps_its_own_values(gb, gpu):
    rng = np.random.default_rng(21)
    op = sel(gb, mixed, "FP64")                                                      # an FP64 operator on an INT32 matrix: the cast serves the predicate only
    A, Ad = rand_mat(gb, rng, "INT32", 37, 53, 800, grid_values)
    got = A.select(op, 2.25)
    assert got.type is gb.INT32
    want = model_select(mixed, "FP64", "FP64", Ad, 2.25)
    assert 0 < len(want) < len(Ad) and all(isinstance(x, int) for x in want.values())
    assert_same(got_dict(got), want, "INT32 operand, FP64 operator")
    u, ud = rand_vec(gb, rng, "INT32", 301, 200, grid_values)
    gv = u.select(op, 2.25)
    assert gv.type is gb.INT32
    assert_same(got_dict(gv), model_select(mixed, "FP64", "FP64", ud, 2.25), "INT32 vector, FP64 operator")


def test_thunk_of_another_type_no_thunk_and_an_empty_thunk(gb, gpu):
    rng = np.random.default_rng(22)
    op = sel(gb, mixed, "FP64")
    A, Ad = rand_mat(gb, rng, "FP64", 37, 53, 800, grid_values)
    oph = C.c_void_p(op.get_op())
    # a thunk given as INT32 is cast into the operator's thunk type (FP64)
    s = U.scalar_handle(gb, "INT32", 3)
    out = gb.Matrix.sparse(gb.FP64, 37, 53)
    assert select_raw(gb, A, oph, s, out) == 0
    assert_same(got_dict(out), model_select(mixed, "FP64", "FP64", Ad, 3), "INT32 thunk")
    gb.lib.GxB_Scalar_free(C.byref(s))
    # a fractional thunk into an INT64 thunk type truncates, as a C cast does
    opi = sel(gb, mixed, "FP64", "INT64")
    assert_same(got_dict(A.select(opi, 2)), model_select(mixed, "FP64", "INT64", Ad, 2), "INT64 thunk type")
    s = U.scalar_handle(gb, "FP64", 2.75)
    out = gb.Matrix.sparse(gb.FP64, 37, 53)
    assert select_raw(gb, A, C.c_void_p(opi.get_op()), s, out) == 0
    assert_same(got_dict(out), model_select(mixed, "FP64", "INT64", Ad, 2), "FP64 thunk 2.75 into an INT64 thunk type")
    gb.lib.GxB_Scalar_free(C.byref(s))
    # no thunk, and a GxB_Scalar without an entry: the zero of the thunk type
    want0 = model_select(mixed, "FP64", "FP64", Ad, 0)
    assert 0 < len(want0) < len(Ad)
    assert_same(got_dict(A.select(op)), want0, "no thunk")
    e = C.c_void_p()
    assert gb.lib.GxB_Scalar_new(C.byref(e), C.c_void_p(gb.FP64._h)) == 0
    out = gb.Matrix.sparse(gb.FP64, 37, 53)
    assert select_raw(gb, A, oph, e, out) == 0
    assert_same(got_dict(out), want0, "empty thunk")
    gb.lib.GxB_Scalar_free(C.byref(e))


def test_output_aliasing_the_input(gb, gpu):
    rng = np.random.default_rng(23)
    op = sel(gb, mixed, "FP64")
    A, Ad = rand_mat(gb, rng, "FP64", 37, 53, 800, grid_values)
    A.select(op, 2.25, out=A)
    assert_same(got_dict(A), model_select(mixed, "FP64", "FP64", Ad, 2.25), "out is the input")
    u, ud = rand_vec(gb, rng, "FP64", 301, 200, grid_values)
    u.select(op, 2.25, out=u)
    assert_same(got_dict(u), model_select(mixed, "FP64", "FP64", ud, 2.25), "vector: out is the input")


# ---- 4. matrix shapes where the kernel can go wrong -------------------------------------------------------------------------------------------------------
def check_shape(gb, typ, A, Ad, what, thunk=2.25):
    for func in (mixed, always, never):
        got = got_dict(A.select(sel(gb, func, typ), thunk))
        assert_same(got, model_select(func, typ, typ, Ad, thunk), f"{what}: {func.__name__}")
    assert got_dict(A.select(sel(gb, never, typ))) == {}


def test_tiny_matrices(gb, gpu):
    check_shape(gb, "FP64", gb.Matrix.sparse(gb.FP64, 5, 7), {}, "nnz = 0")
    for x in (2.0, 0.5):
        A, Ad = mat_of(gb, "FP64", 1, 1, [0], [0], [x])
        check_shape(gb, "FP64", A, Ad, f"1 x 1 holding {x}")
    I, J = np.divmod(np.arange(9), 3)
    A, Ad = mat_of(gb, "FP64", 3, 3, I, J, np.arange(9) / 2.0 - 2)
    check_shape(gb, "FP64", A, Ad, "3 x 3 full")


@pytest.mark.parametrize("typ,nnz", [("FP64", 401), ("FP32", 402), ("INT16", 403), ("INT8", 7)])
def test_partial_last_group_and_empty_first_and_last_rows(gb, gpu, typ, nnz):
    """nnz = 1, 2, 3 (mod 4): the last group of four is partial; rows 0 and 36 hold nothing."""
    rng = np.random.default_rng(nnz)
    flat = np.sort(rng.choice(35 * 53, size=nnz, replace=False)) + 53
    I, J = np.divmod(flat, 53)
    A, Ad = mat_of(gb, typ, 37, 53, I, J, grid_values(rng, typ, nnz))
    assert nnz % 4 != 0 and I.min() >= 1 and I.max() <= 35
    check_shape(gb, typ, A, Ad, f"{typ} nnz = {nnz}", 2.25 if typ.startswith("FP") else 9)


def test_several_workgroups_and_a_row_longer_than_a_stride(gb, gpu):
    rng = np.random.default_rng(31)
    nr, nc = 1000, 1300
    flat = np.unique(np.concatenate([rng.choice(nr * nc, size=3800, replace=False), 500 * nc + rng.choice(nc, size=1200, replace=False)]))
    I, J = np.divmod(flat, nc)
    assert 4500 <= len(flat) <= 5500 and int((I == 500).sum()) > 1024
    for typ in ("FP64", "INT8"):
        A, Ad = mat_of(gb, typ, nr, nc, I, J, grid_values(rng, typ, len(flat)))
        check_shape(gb, typ, A, Ad, f"1000 x 1300 {typ}", 2.25 if typ == "FP64" else 9)


def test_column_indices_beyond_2_to_the_31(gb, gpu):
    """As wide as the device layout allows: entries in column 0, column 2^31 and the last column; j must reach the predicate unsigned and whole."""
    nc = DIM_DEVICE_MAX
    cols = [0, 5, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, nc - 1]
    I = [0, 0, 0, 1, 2, 2]
    A, Ad = mat_of(gb, "FP64", 3, nc, I, cols, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    got = got_dict(A.select(sel(gb, right_half, "FP64")))
    assert got == {(1, 1 << 31): 4.0, (2, (1 << 31) + 1): 5.0, (2, nc - 1): 6.0}
    assert got == model_select(right_half, "FP64", "FP64", Ad, None)
    assert got_dict(A.select(sel(gb, u_tril, "FP64", "INT64"), 5)) == {(0, 0): 1.0, (0, 5): 2.0}


# ---- 5. vector shapes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", ["FP64", "FP32", "INT16", "BOOL"])
def test_vector_sizes_and_absent_positions(gb, gpu, typ):
    rng = np.random.default_rng(41)
    for n, k in ((1, 1), (1, 0), (5, 3), (1027, 700), (1027, 1027)):
        if k:
            u, ud = rand_vec(gb, rng, typ, n, k)
        else:
            u, ud = gb.Vector.sparse(getattr(gb, typ), n), {}
        got = u.select(sel(gb, always, typ))
        assert gb.last_kernel_plan().startswith(plan_of(gb, always, typ, typ, "vector"))
        assert_same(got_dict(got), ud, f"{typ} vector of {n} with {k} entries, always true")        # absent positions stay absent
        assert got_dict(u.select(sel(gb, never, typ))) == {}
        if typ != "BOOL":
            thunk = 1 if not typ.startswith("FP") else 1.0
            assert_same(got_dict(u.select(sel(gb, u_gt, typ), thunk)), model_select(u_gt, typ, typ, ud, thunk), f"{typ} vector of {n}: x > v")


# ---- 6. non-blocking mode ---------------------------------------------------------------------------------------------------------------------------------------
_MODE_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import pygraphblas_amd as gb
import test_userselect_gpu as t
n = 100000
rng = np.random.default_rng(1)
u = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), rng.integers(-16, 17, n) / 8.0, n, gb.FP64)
v = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), rng.integers(-16, 17, n) / 8.0, n, gb.FP64)
op = gb.select_op(gb.FP64)(t.mixed)
w = u.eadd(v, gb.FP64.PLUS)            # deferred in non-blocking mode
w = w.apply(gb.FP64.AINV)              # ... and chained
r = w.select(op, 2.25)                 # the user operator: the pending chain is completed, then this runs eagerly
plan = gb.last_kernel_plan()
r2 = r.apply(gb.FP64.ABS)              # built-in work queued after a user result reads it correctly too
I, X = r2.to_arrays()
print(plan.split(">")[0])
print(len(I), int(I.sum()), float(X.sum()), I[:5].tolist(), X[:5].tolist())
"""


def test_nonblocking_chain_then_user_select_equals_blocking(gb, gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _MODE_CHILD.format(root=root, tests=os.path.join(root, "tests"))
    outs = []
    for blocking in ("0", "1"):
        env = dict(os.environ, GRB_MI355X_BLOCKING=blocking)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.strip().splitlines()[-2:])
    assert outs[0] == outs[1], outs
    assert outs[0][0] == "userselect<name=mixed,xtype=GrB_FP64,ttype=GrB_FP64,on=vector"
    rng = np.random.default_rng(1)                                                   # and against the model
    a = rng.integers(-16, 17, 100000) / 8.0
    b = rng.integers(-16, 17, 100000) / 8.0
    w = -(a + b)
    idx = np.nonzero((np.arange(100000) % 3 == 0) & (w * w > 2.25))[0]
    assert outs[0][1].startswith(f"{len(idx)} {int(idx.sum())} {float(np.abs(w[idx]).sum())!r} ")


# ---- 7. compile failure and caching -------------------------------------------------------------------------------------------------------------------------
def test_a_definition_that_does_not_compile_is_an_error_with_the_log(gb, gpu):
    h = new_selectop(gb, "FP64", None, "broken_pred", "bool broken_pred (GrB_Index i, GrB_Index j, const double *x, const double *thunk) { return (*x) >* ; }")
    A = gb.Matrix.from_lists([0, 1], [1, 0], [1.0, 2.0])
    out = gb.Matrix.from_lists([0], [0], [5.0], 2, 2)
    info = select_raw(gb, A, h, None, out)
    assert info == gb._capi.constants["GrB_INVALID_VALUE"]
    with pytest.raises(gb.InvalidValue):
        gb.base.check(info, out)
    s = C.c_char_p()
    assert gb.lib.GrB_Matrix_error(C.byref(s), out._h) == 0
    msg = s.value.decode()
    assert "broken_pred" in msg and "error" in msg and "expected expression" in msg, msg
    assert got_dict(out) == {(0, 0): 5.0}
    before = stats(gb)
    assert select_raw(gb, A, h, None, out) == info                                   # remembered: not compiled again, the same answer
    assert stats(gb) == before and got_dict(out) == {(0, 0): 5.0}
    v, w = gb.Vector.from_lists([0, 1], [1.0, 2.0]), gb.Vector.from_lists([1], [6.0], 2)
    assert select_raw(gb, v, h, None, w) == info and got_dict(w) == {1: 6.0}
    gb.lib.GxB_SelectOp_free(C.byref(h))


def test_a_second_operator_with_the_same_text_compiles_nothing(gb, gpu, monkeypatch, tmp_path):
    monkeypatch.setenv("GRB_MI355X_CACHE_DIR", str(tmp_path))                        # (an empty cache: the first use really compiles)
    defn = "bool cache_probe_7 (GrB_Index i, GrB_Index j, const double *x, const double *thunk) { return i + j > 1 && (*x) > (*thunk) ; }"
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    c0, d0, l0 = stats(gb)
    h1 = new_selectop(gb, "FP64", "FP64", "cache_probe_7", defn)
    out = gb.Matrix.sparse(gb.FP64, 3, 3)
    assert select_raw(gb, A, h1, None, out) == 0 and got_dict(out) == {(1, 2): 2.0, (2, 0): 3.0}
    assert stats(gb) == (c0 + 1, d0, l0 + 1)
    h2 = new_selectop(gb, "FP64", None, "cache_probe_7", defn)                       # another object, the same text (a NULL thunk type is the value type)
    assert h2.value != h1.value
    out2 = gb.Matrix.sparse(gb.FP64, 3, 3)
    assert select_raw(gb, A, h2, None, out2) == 0 and got_dict(out2) == got_dict(out)
    assert stats(gb) == (c0 + 1, d0, l0 + 2)
    assert len([f for f in os.listdir(tmp_path) if f.startswith("userselect-") and f.endswith(".co")]) == 1
    for h in (h1, h2):
        gb.lib.GxB_SelectOp_free(C.byref(h))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_hypersparse_and_complex_operands_are_refused_and_leave_the_output_alone(gb, gpu):
    DM = gb.DomainMismatch
    op = sel(gb, mixed, "FP64")
    H = gb.Matrix.sparse(gb.FP64)
    H[3, 1 << 40] = 2.0
    H2 = gb.Matrix.sparse(gb.FP64)
    H2[7, 7] = 1.0
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    for fn in (lambda: H.select(op, 1.0, out=H2), lambda: H.select(op, out=H2)):
        with pytest.raises(DM, match="mixed.*hypersparse"):
            fn()
        assert got_dict(H2) == {(7, 7): 1.0}
    hv, hv2 = gb.Vector.sparse(gb.FP64), gb.Vector.sparse(gb.FP64)
    hv[1 << 40] = 2.0
    hv2[5] = 1.0
    with pytest.raises(DM, match="mixed.*hypersparse"):
        hv.select(op, 1.0, out=hv2)
    assert got_dict(hv2) == {5: 1.0}
    # complex containers: made through the C ABI (the Python layer has no complex type classes)
    lib = gb.lib
    fc64 = C.c_void_p(gb._capi.handle("GxB_FC64"))
    cm, cv = C.c_void_p(), C.c_void_p()
    assert lib.GrB_Matrix_new(C.byref(cm), fc64, C.c_uint64(3), C.c_uint64(3)) == 0
    assert lib.GrB_Vector_new(C.byref(cv), fc64, C.c_uint64(3)) == 0
    oph = C.c_void_p(op.get_op())
    out = gb.Matrix.from_lists([0], [0], [5.0], 3, 3)
    w = gb.Vector.from_lists([1], [6.0], 3)
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    dm = gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    for info, holder, err in ((lib.GxB_Matrix_select(out._h, None, None, oph, cm, None, None), out, lib.GrB_Matrix_error),
                              (lib.GxB_Matrix_select(cm, None, None, oph, A._h, None, None), None, None),
                              (lib.GxB_Vector_select(w._h, None, None, oph, cv, None, None), w, lib.GrB_Vector_error),
                              (lib.GxB_Vector_select(cv, None, None, oph, v._h, None, None), None, None)):
        assert info == dm
        if holder is not None:
            s = C.c_char_p()
            assert err(C.byref(s), holder._h) == 0
            assert "mixed" in s.value.decode() and "complex" in s.value.decode(), s.value
    assert got_dict(out) == {(0, 0): 5.0} and got_dict(w) == {1: 6.0}
    n = C.c_uint64(9)
    assert lib.GrB_Matrix_nvals(C.byref(n), cm) == 0 and n.value == 0
    lib.GrB_Matrix_free(C.byref(cm))
    lib.GrB_Vector_free(C.byref(cv))
    # a user-defined binary operator is no accumulator here either
    with pytest.raises(DM, match="f_arith"):
        A.select(op, 1.0, out=out, accum=U.user_op(gb, U.f_arith, "FP64", 2))
    assert got_dict(out) == {(0, 0): 5.0}
