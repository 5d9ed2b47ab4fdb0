"""The parts of sort and top-k that need no device: the five entry points and the threshold getter, the refusals, the host route of GxB_Matrix_sort /
GxB_Vector_sort / GrBX_*_select_topk against the numpy model (tests/sort_model.py, exact), and the key functions of grb_sort_keys.hpp under the address and
undefined-behaviour sanitizers (a stand-alone host program, tests/sort_keys_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import sort_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, DOMAIN_MISMATCH, DIMENSION_MISMATCH = 4, 7, 8
TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
NROWS, NCOLS = 40, 50


@pytest.fixture()
def host_route():
    """GRB_MI355X_SORT=0 (and every call on a machine without a device) is the host route."""
    os.environ["GRB_MI355X_SORT"] = "0"
    try:
        yield
    finally:
        os.environ.pop("GRB_MI355X_SORT", None)


def op_of(gb, name, gt=False):
    return C.c_void_p((getattr(gb, name).GT if gt else getattr(gb, name).LT).get_op())


def values(rng, gb, name, n):
    """Few distinct values (ties everywhere) with the type's extremes among them; floats carry NaN, both zeros and both infinities."""
    dt = getattr(gb, name)._np
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    if name in ("FP32", "FP64"):
        pool = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 3.0, 1e-40], dt)
    else:
        info = np.iinfo(dt)
        pool = np.array([info.min, info.max, 0, 1, 2, info.max // 2 + 1], dt)
    return pool[rng.integers(0, len(pool), n)]


def the_matrix(rng, gb, name):
    """40 x 50 with rows of 0, 1, 2 and 50 entries."""
    lens = np.zeros(NROWS, np.int64)
    lens[[3, 17]] = 1
    lens[[4, 30]] = 2
    lens[[5, 39]] = NCOLS
    I = np.repeat(np.arange(NROWS), lens).astype(np.uint64)
    J = np.concatenate([np.sort(rng.choice(NCOLS, size=k, replace=False)) for k in lens]).astype(np.uint64)
    return I, J, values(rng, gb, name, len(I))


def same(got, want):
    return got.dtype == want.dtype and np.array_equal(M.bits(got), M.bits(want))


def test_the_five_symbols_are_exported(gb):
    for f in ("GxB_Matrix_sort", "GxB_Vector_sort", "GrBX_Matrix_select_topk", "GrBX_Vector_select_topk", "GrBX_sort_thresholds"):
        assert f in gb._capi.functions and f not in gb._capi.missing and hasattr(gb.lib, f)


def test_sort_thresholds_getter(gb):
    """wave_max == 64 and a power-of-two lds_max > 64: the edges the default route uses (the LDS kernel's capacity is 4096; its edge is the largest at which it
    did not measure slower than the segmented radix sort)."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert gb.lib.GrBX_sort_thresholds(C.byref(a), C.byref(b)) == 0
    assert a.value == 64 and b.value > 64 and b.value & (b.value - 1) == 0 and b.value <= 4096
    assert gb.lib.GrBX_sort_thresholds(None, C.byref(b)) == NULL_POINTER and gb.lib.GrBX_sort_thresholds(C.byref(a), None) == NULL_POINTER


def test_refusals(gb):
    A = gb.Matrix.from_lists([0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0], 3, 4, gb.FP32)
    C34, P34, C33, P34f = gb.Matrix.sparse(gb.FP32, 3, 4), gb.Matrix.sparse(gb.INT64, 3, 4), gb.Matrix.sparse(gb.FP32, 3, 3), gb.Matrix.sparse(gb.FP64, 3, 4)
    lt = op_of(gb, "FP32")
    sort, topk = gb.lib.GxB_Matrix_sort, gb.lib.GrBX_Matrix_select_topk
    assert sort(None, None, lt, A._h, None) == NULL_POINTER
    assert sort(C34._h, P34._h, None, A._h, None) == NULL_POINTER and sort(C34._h, P34._h, lt, None, None) == NULL_POINTER
    assert sort(C34._h, P34f._h, lt, A._h, None) == DOMAIN_MISMATCH, "P must be INT64"
    assert sort(C33._h, None, lt, A._h, None) == DIMENSION_MISMATCH and sort(None, gb.Matrix.sparse(gb.INT64, 4, 3)._h, lt, A._h, None) == DIMENSION_MISMATCH
    assert sort(C34._h, None, C.c_void_p(gb.FP32.LE.get_op()), A._h, None) == DOMAIN_MISMATCH, "LE is not strict"
    with pytest.raises(gb.base.DomainMismatch, match="GrB_LE_FP32"):
        A.sort(op=gb.FP32.LE)
    assert sort(C34._h, None, C.c_void_p(gb.FP32.PLUS.get_op()), A._h, None) == DOMAIN_MISMATCH
    assert topk(C34._h, C.c_void_p(gb.FP32.GE.get_op()), A._h, C.c_uint64(1), None) == DOMAIN_MISMATCH and topk(C33._h, lt, A._h, C.c_uint64(1), None) == DIMENSION_MISMATCH
    assert topk(None, lt, A._h, C.c_uint64(1), None) == NULL_POINTER

    def bigger(x, y):
        return x > y
    user = gb.binary_op(gb.FP32)(bigger)
    assert sort(C34._h, None, C.c_void_p(user.get_op()), A._h, None) == DOMAIN_MISMATCH, "a user-defined operator has no key"
    # an FC64 matrix (the package has no Python class for the complex types: through the C ABI), as operand and as output
    Z, Zc = C.c_void_p(), C.c_void_p()
    fc64 = C.c_void_p(gb._capi.handle("GxB_FC64"))
    assert gb.lib.GrB_Matrix_new(C.byref(Z), fc64, C.c_uint64(3), C.c_uint64(4)) == 0 and gb.lib.GrB_Matrix_new(C.byref(Zc), fc64, C.c_uint64(3), C.c_uint64(4)) == 0
    assert sort(Zc, None, lt, Z, None) == DOMAIN_MISMATCH and sort(None, P34._h, lt, Z, None) == DOMAIN_MISMATCH and sort(Zc, None, lt, A._h, None) == DOMAIN_MISMATCH
    assert topk(Zc, lt, Z, C.c_uint64(1), None) == DOMAIN_MISMATCH
    assert gb.lib.GrB_Matrix_free(C.byref(Z)) == 0 and gb.lib.GrB_Matrix_free(C.byref(Zc)) == 0
    # vectors
    u = gb.Vector.from_lists([0, 2], [3.0, 4.0], 3, gb.FP32)
    w3, p3, w4, p3f = gb.Vector.sparse(gb.FP32, 3), gb.Vector.sparse(gb.INT64, 3), gb.Vector.sparse(gb.FP32, 4), gb.Vector.sparse(gb.INT32, 3)
    vsort, vtopk = gb.lib.GxB_Vector_sort, gb.lib.GrBX_Vector_select_topk
    assert vsort(None, None, lt, u._h, None) == NULL_POINTER and vsort(w3._h, p3f._h, lt, u._h, None) == DOMAIN_MISMATCH
    assert vsort(w4._h, None, lt, u._h, None) == DIMENSION_MISMATCH and vsort(w3._h, p3._h, C.c_void_p(gb.FP32.LE.get_op()), u._h, None) == DOMAIN_MISMATCH
    assert vtopk(w4._h, lt, u._h, C.c_uint64(1), None) == DIMENSION_MISMATCH and vtopk(None, lt, u._h, C.c_uint64(1), None) == NULL_POINTER
    assert sorted(A) == [(0, 0, 1.0), (1, 1, 2.0), (2, 2, 3.0)], "a refused call changes nothing"


@pytest.mark.parametrize("name", TYPES)
def test_host_route_matrix_matches_the_model(gb, host_route, name):
    rng = np.random.default_rng(TYPES.index(name))
    typ = getattr(gb, name)
    I, J, X = the_matrix(rng, gb, name)
    for gt in (False, True):
        for by_col in (False, True):
            desc = gb.descriptor.T0 if by_col else None
            A = gb.Matrix.from_arrays(I, J, X, NROWS, NCOLS, typ)
            wi, wj, wx, wp = M.matrix_sort(I, J, X, gt=gt, by_col=by_col)
            Cm, Pm = A.sort(op=typ.GT if gt else typ.LT, desc=desc)
            assert gb.last_kernel_plan() == "", "the host route leaves the plan empty"
            ci, cj, cx = Cm.to_arrays()
            pi, pj, px = Pm.to_arrays()
            assert np.array_equal(ci, wi) and np.array_equal(cj, wj) and same(cx, wx), (name, gt, by_col)
            assert Pm.type is gb.INT64 and np.array_equal(pi, wi) and np.array_equal(pj, wj) and same(px, wp), (name, gt, by_col)
            # C only, P only
            Conly, none = A.sort(op=typ.GT if gt else typ.LT, desc=desc, perm=False)
            assert none is None and same(Conly.to_arrays()[2], wx) and np.array_equal(Conly.to_arrays()[1], wj)
            none, Ponly = A.sort(op=typ.GT if gt else typ.LT, desc=desc, values=False)
            assert none is None and same(Ponly.to_arrays()[2], wp) and np.array_equal(Ponly.to_arrays()[0], wi)
            # C is A: earlier content gone, a pending edit included
            A[0, 0] = X[0]
            Iq, Jq, Xq = A.to_arrays()
            A[1, 1] = X[0]
            del A[1, 1]
            P2 = gb.Matrix.sparse(gb.INT64, NROWS, NCOLS)
            P2[7, 7] = 5
            assert gb.lib.GxB_Matrix_sort(A._h, P2._h, op_of(gb, name, gt), A._h, C.c_void_p(desc.get_desc()) if desc else None) == 0
            qi, qj, qx, qp = M.matrix_sort(Iq, Jq, Xq, gt=gt, by_col=by_col)
            ai, aj, ax = A.to_arrays()
            assert np.array_equal(ai, qi) and np.array_equal(aj, qj) and same(ax, qx) and same(P2.to_arrays()[2], qp), (name, gt, by_col)
            # top-k
            for k in (0, 1, 3, NCOLS + 5):
                A = gb.Matrix.from_arrays(I, J, X, NROWS, NCOLS, typ)
                ti, tj, tx = M.matrix_topk(I, J, X, k, gt=gt, by_col=by_col)
                out = gb.Matrix.sparse(typ, NROWS, NCOLS)
                assert gb.lib.GrBX_Matrix_select_topk(out._h, op_of(gb, name, gt), A._h, C.c_uint64(k), C.c_void_p(desc.get_desc()) if desc else None) == 0
                oi, oj, ox = out.to_arrays()
                assert np.array_equal(oi, ti) and np.array_equal(oj, tj) and same(ox, tx), (name, gt, by_col, k)
                assert gb.lib.GrBX_Matrix_select_topk(A._h, op_of(gb, name, gt), A._h, C.c_uint64(k), C.c_void_p(desc.get_desc()) if desc else None) == 0      # C is A
                oi, oj, ox = A.to_arrays()
                assert np.array_equal(oi, ti) and np.array_equal(oj, tj) and same(ox, tx), (name, gt, by_col, k)


@pytest.mark.parametrize("name", TYPES)
def test_host_route_vector_matches_the_model(gb, host_route, name):
    rng = np.random.default_rng(100 + TYPES.index(name))
    typ = getattr(gb, name)
    for n, nv in ((1, 0), (1, 1), (50, 2), (50, 50), (300, 120)):
        idx = np.sort(rng.choice(n, size=nv, replace=False)).astype(np.uint64)
        x = values(rng, gb, name, nv)
        for gt in (False, True):
            u = gb.Vector.from_arrays(idx, x, n, typ)
            wx, px = M.vector_sort(idx, x, gt=gt)
            w, p = u.sort(op=typ.GT if gt else typ.LT)
            assert gb.last_kernel_plan() == ""
            gi, gx = w.to_arrays()
            hi, hx = p.to_arrays()
            assert np.array_equal(gi, np.arange(nv, dtype=np.uint64)) and same(gx, wx) and np.array_equal(hi, gi) and same(hx, px) and p.type is gb.INT64, (name, n, nv, gt)
            w1, none = u.sort(op=typ.GT if gt else typ.LT, perm=False)
            none2, p1 = u.sort(op=typ.GT if gt else typ.LT, values=False)
            assert none is None and none2 is None and same(w1.to_arrays()[1], wx) and same(p1.to_arrays()[1], px)
            for k in (0, 1, 3, n + 5):
                ti, tx = M.vector_topk(idx, x, k, gt=gt)
                t = u.topk(k, largest=gt)
                oi, ox = t.to_arrays()
                assert np.array_equal(oi, ti) and same(ox, tx), (name, n, nv, gt, k)
            assert gb.lib.GxB_Vector_sort(u._h, None, op_of(gb, name, gt), u._h, None) == 0      # w is u
            assert same(u.to_arrays()[1], wx)


def test_host_route_casts(gb, host_route):
    """The operator's type decides the comparison, C's type the stored values: FP64 values under GrB_LT_INT32 into an INT32 C."""
    rng = np.random.default_rng(7)
    I, J, _ = the_matrix(rng, gb, "FP64")
    X = (rng.integers(-40, 40, len(I)) / 4.0).astype(np.float64)
    A = gb.Matrix.from_arrays(I, J, X, NROWS, NCOLS, gb.FP64)
    wi, wj, wx, wp = M.matrix_sort(I, J, X, gt=False, key_dtype=np.int32)
    Cm, Pm = gb.Matrix.sparse(gb.INT32, NROWS, NCOLS), gb.Matrix.sparse(gb.INT64, NROWS, NCOLS)
    assert gb.lib.GxB_Matrix_sort(Cm._h, Pm._h, op_of(gb, "INT32"), A._h, None) == 0
    assert same(Cm.to_arrays()[2], M.cast(wx, np.int32)) and same(Pm.to_arrays()[2], wp)
    assert not np.array_equal(wp, M.matrix_sort(I, J, X, gt=False)[3]), "the case must tell the two comparison types apart"


def test_python_surface_defaults(gb, host_route):
    A = gb.Matrix.from_lists([0, 0, 0, 1], [0, 1, 2, 2], [3, 1, 2, 9], 2, 3, gb.INT64)
    Cm, Pm = A.sort()
    assert sorted(Cm) == [(0, 0, 1), (0, 1, 2), (0, 2, 3), (1, 0, 9)] and sorted(Pm) == [(0, 0, 1), (0, 1, 2), (0, 2, 0), (1, 0, 2)]
    assert sorted(A.topk(1)) == [(0, 0, 3), (1, 2, 9)] and sorted(A.topk(2, largest=False)) == [(0, 1, 1), (0, 2, 2), (1, 2, 9)]
    assert sorted(A.topk(1, desc=gb.descriptor.T0)) == [(0, 0, 3), (0, 1, 1), (1, 2, 9)]
    v = gb.Vector.from_lists([1, 3, 4], [5, 7, 5], 6, gb.INT64)
    w, p = v.sort()
    assert sorted(w) == [(0, 5), (1, 5), (2, 7)] and sorted(p) == [(0, 1), (1, 4), (2, 3)]
    assert sorted(v.topk(2)) == [(1, 5), (3, 7)] and sorted(v.topk(1, largest=False)) == [(1, 5)]


def test_sort_keys_under_the_sanitizers(tmp_path):
    """key(a) < key(b) exactly when a precedes b, for all pairs of every type's edge values under LT and GT: a host program of its own, host code only, built
    with the address and undefined-behaviour sanitizers; no device code, nothing loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "sort_keys_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sort_keys_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sort keys ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
