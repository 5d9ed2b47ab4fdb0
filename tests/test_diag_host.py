"""The parts of the diagonal operations that need no device: the Python surface (Matrix.diag, Matrix.identity below the threshold), the threshold getter, the
host route of GxB_Matrix_diag / GxB_Vector_diag against a numpy restatement of the rule, and the diagonal geometry of grb_diag.hpp under the address and
undefined-behaviour sanitizers (a stand-alone host program, tests/diag_geometry_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMENSION_MISMATCH, NULL_POINTER = 8, 4


def outcome(f):
    """The tuples a call gives, or the exception type it raises (select needs a device; the host-only surface does not)."""
    try:
        return sorted(f())
    except Exception as e:       # noqa: BLE001
        return type(e).__name__


def test_matrix_diag_exists_and_is_select(gb):
    assert "diag" in vars(gb.Matrix), "Matrix.diag must be a method of its own, not a name __getattr__ resolves"
    A = gb.Matrix.from_lists([0, 1, 2, 0, 1], [0, 1, 2, 2, 0], [1, 2, 3, 4, 5], 3, 3, gb.INT32)
    for thunk in (None, 2, -1):
        assert outcome(lambda: A.diag(thunk)) == outcome(lambda: A.select("DIAG", thunk))
    assert outcome(lambda: A.diag()) == outcome(lambda: A.select("DIAG"))
    if gb.device_info()["ok"]:
        assert sorted(A.diag()) == [(0, 0, 1), (1, 1, 2), (2, 2, 3)] and sorted(A.diag(2)) == [(0, 2, 4)] and sorted(A.diag(-1)) == [(1, 0, 5)]


def test_diag_thresholds_getter(gb):
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert gb.lib.GrBX_diag_thresholds(C.byref(a), C.byref(b)) == 0
    assert a.value > 0 and b.value > 0
    assert gb.lib.GrBX_diag_thresholds(None, C.byref(b)) == NULL_POINTER and gb.lib.GrBX_diag_thresholds(C.byref(a), None) == NULL_POINTER
    assert "GrBX_diag_thresholds" in gb._capi.functions and "GrBX_diag_thresholds" not in gb._capi.missing


def test_identity_below_the_threshold_is_unchanged(gb):
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert gb.lib.GrBX_diag_thresholds(C.byref(a), C.byref(b)) == 0
    for typ, n, one, want in ((gb.FP32, 5, None, 1.0), (gb.INT64, 7, 3, 3), (gb.BOOL, 2, None, True), (gb.FP64, 0, None, 1.0), (gb.UINT8, min(a.value - 1, 300), None, 1)):
        Id = gb.Matrix.identity(typ, n) if one is None else gb.Matrix.identity(typ, n, one)
        w = C.c_int(-1)
        assert gb.lib.GrBX_Matrix_residency(Id._h, C.byref(w)) == 0 and w.value == 1, "built from tuples on the host, as before"
        assert Id.type is typ and Id.shape == (n, n)
        I, J, X = Id.to_arrays()
        assert np.array_equal(I, np.arange(n, dtype=np.uint64)) and np.array_equal(J, I) and X.dtype == typ._np and np.array_equal(X, np.full(n, want, typ._np))


def test_host_route_matches_the_rule(gb):
    """GRB_MI355X_DIAG=0 (and every call on a machine without a device) is the host route: entry r of v at (r, r + k) or (r + |k|, r), and back."""
    rng = np.random.default_rng(2)
    os.environ["GRB_MI355X_DIAG"] = "0"
    try:
        for n in (0, 1, 5, 64, 257):
            idx = np.sort(rng.choice(n, size=(n + 1) // 2, replace=False)).astype(np.uint64) if n else np.zeros(0, np.uint64)
            x = (rng.standard_normal(len(idx)) * 100).astype(np.float32)
            for k in (0, 1, -1, 5, -5):
                v = gb.Vector.from_arrays(idx, x, n, gb.FP32)
                D = gb.Matrix.sparse(gb.INT32, n + abs(k), n + abs(k))
                if n + abs(k):
                    D[0, 0] = 9                                        # gone afterwards
                assert gb.lib.GxB_Matrix_diag(D._h, v._h, C.c_int64(k), None) == 0
                I, J, X = D.to_arrays()
                assert np.array_equal(I, idx + np.uint64(max(-k, 0))) and np.array_equal(J, idx + np.uint64(max(k, 0))) and np.array_equal(X, x.astype(np.int32))
                back = D.vector_diag(k)
                bi, bx = back.to_arrays()
                assert back.size == n and np.array_equal(bi, idx) and np.array_equal(bx, x.astype(np.int32))
                assert D.vector_diag(k + 1).nvals == 0 and gb.last_kernel_plan() == ""
    finally:
        os.environ.pop("GRB_MI355X_DIAG", None)


def test_host_route_errors(gb):
    v = gb.Vector.from_lists([0, 2], [3, 4], 3, gb.INT64)
    A = gb.Matrix.from_lists([0, 1, 2], [0, 1, 2], [1, 2, 3], 3, 4, gb.INT64)
    C3, C45, v2, v3 = gb.Matrix.sparse(gb.INT64, 3, 3), gb.Matrix.sparse(gb.INT64, 4, 5), gb.Vector.sparse(gb.INT64, 2), gb.Vector.sparse(gb.INT64, 3)
    assert gb.lib.GxB_Matrix_diag(C3._h, v._h, C.c_int64(-1), None) == DIMENSION_MISMATCH
    assert gb.lib.GxB_Matrix_diag(C45._h, v._h, C.c_int64(1), None) == DIMENSION_MISMATCH
    assert gb.lib.GxB_Matrix_diag(C3._h, v._h, C.c_int64(-(1 << 63)), None) == DIMENSION_MISMATCH
    assert gb.lib.GxB_Vector_diag(v2._h, A._h, C.c_int64(0), None) == DIMENSION_MISMATCH
    assert gb.lib.GxB_Vector_diag(v3._h, A._h, C.c_int64(2), None) == DIMENSION_MISMATCH
    assert gb.lib.GxB_Vector_diag(v3._h, A._h, C.c_int64(-(1 << 63)), None) == DIMENSION_MISMATCH
    assert gb.lib.GxB_Matrix_diag(None, v._h, C.c_int64(0), None) == NULL_POINTER and gb.lib.GxB_Matrix_diag(C3._h, None, C.c_int64(0), None) == NULL_POINTER
    assert gb.lib.GxB_Vector_diag(None, A._h, C.c_int64(0), None) == NULL_POINTER and gb.lib.GxB_Vector_diag(v3._h, None, C.c_int64(0), None) == NULL_POINTER


def test_diag_geometry_under_the_sanitizers(tmp_path):
    """diag_len, the row / column offsets, the matrix dimension and the flat ends of the row pointer for k over INT64_MIN .. INT64_MAX, compared with 128-bit
    arithmetic: a host program of its own, host code only, built with the address and undefined-behaviour sanitizers; no device code, nothing loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "diag_geometry_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "diag_geometry_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "diag geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
