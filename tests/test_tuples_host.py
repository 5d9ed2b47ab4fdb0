"""The parts of extractTuples-into-HBM that need no device: the three new entry points, GrBX_*_extractTuples_at with location 0 against GrB_*_extractTuples_<T> for
the 11 real types and FC64, every info code of the new calls, Matrix.to_tensors / Vector.to_tensors on the CPU path, and the tile arithmetic of
grb_tuples_geom.hpp under the address and undefined-behaviour sanitizers (a stand-alone host program, tests/tuples_geometry_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, INVALID_VALUE, INSUFFICIENT_SPACE = 4, 5, 11
REAL = ("BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _matrix(gb, typ, seed=3):
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(40 * 30, 200, replace=False))
    I, J = (flat // 30).astype(np.uint64), (flat % 30).astype(np.uint64)
    X = rng.standard_normal(200) * 50
    X = (X if typ._np in (np.float32, np.float64) else X.astype(np.int64)).astype(typ._np)      # (integers wrap, BOOL: non-zero)
    return gb.Matrix.from_arrays(I, J, X, 40, 30, typ), (I, J, X)


def test_symbols_header_and_geometry(gb):
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    for name in ("GrBX_Matrix_extractTuples_at", "GrBX_Vector_extractTuples_at", "GrBX_tuples_geometry"):
        assert name in gb._capi.functions and name not in gb._capi.missing, name
        assert "GrB_Info " + name + "(" in header
    out = (C.c_uint64 * 3)()
    assert gb.lib.GrBX_tuples_geometry(out) == 0
    tile, vtile, cap = (int(v) for v in out)
    assert tile >= 512 and tile % 512 == 0 and vtile >= 256 and vtile % 256 == 0 and cap >= 1
    assert gb.lib.GrBX_tuples_geometry(None) == NULL_POINTER
    for cls in (gb.Matrix, gb.Vector):
        assert hasattr(cls, "to_tensors")
    assert hasattr(gb.Matrix, "to_csr_tensors") and hasattr(gb.Vector, "to_dense_tensors")


@pytest.mark.parametrize("tname", REAL)
def test_location0_is_the_typed_call(gb, tname):
    typ = getattr(gb, tname)
    A, (I0, J0, X0) = _matrix(gb, typ)
    n = len(I0)
    want = A.to_arrays()                                             # GrB_Matrix_extractTuples_<T>
    I, J, X = np.full(n + 2, 77, np.uint64), np.full(n + 2, 77, np.uint64), np.zeros(n + 2, typ._np)
    nn = C.c_uint64(n + 2)
    assert gb.lib.GrBX_Matrix_extractTuples_at(_p(I), _p(J), _p(X), C.byref(nn), A._h, 0) == 0 and nn.value == n
    assert np.array_equal(I[:n], want[0]) and np.array_equal(J[:n], want[1]) and np.array_equal(_bits(X[:n]), _bits(want[2]))
    assert np.array_equal(I[:n], I0) and np.array_equal(J[:n], J0) and I[n] == 77 and J[n + 1] == 77
    assert "tuples<" not in gb.last_kernel_plan()
    v = gb.Vector.from_arrays(I0 * np.uint64(30) + J0, X0, 1200, typ)
    wantv = v.to_arrays()
    K, Y = np.zeros(n, np.uint64), np.zeros(n, typ._np)
    nn = C.c_uint64(n)
    assert gb.lib.GrBX_Vector_extractTuples_at(_p(K), _p(Y), C.byref(nn), v._h, 0) == 0 and nn.value == n
    assert np.array_equal(K, wantv[0]) and np.array_equal(_bits(Y), _bits(wantv[1]))


def test_location0_fc64(gb):
    """A complex container (the C ABI has them, the Python mirror does not): built, read by the typed call and read by the new one."""
    lib, vp = gb.lib, C.c_void_p
    I0 = np.array([0, 2, 2], np.uint64); J0 = np.array([1, 0, 3], np.uint64); X0 = np.array([1 + 2j, -0.0 + 3j, 4 - 1j], np.complex128)
    fc64 = vp(gb._capi.handle("GxB_FC64"))
    A = vp()
    assert lib.GrB_Matrix_new(C.byref(A), fc64, C.c_uint64(3), C.c_uint64(4)) == 0
    assert lib.GxB_Matrix_build_FC64(A, _p(I0), _p(J0), _p(X0), C.c_uint64(3), None) == 0
    wI, wJ, wX = np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(3, np.complex128)
    nn = C.c_uint64(3)
    assert lib.GxB_Matrix_extractTuples_FC64(_p(wI), _p(wJ), _p(wX), C.byref(nn), A) == 0 and nn.value == 3
    I, J, X = np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(3, np.complex128)
    nn = C.c_uint64(3)
    assert lib.GrBX_Matrix_extractTuples_at(_p(I), _p(J), _p(X), C.byref(nn), A, 0) == 0 and nn.value == 3
    assert np.array_equal(I, wI) and np.array_equal(J, wJ) and np.array_equal(_bits(X), _bits(wX)) and np.array_equal(_bits(X), _bits(X0))
    v = vp()
    assert lib.GrB_Vector_new(C.byref(v), fc64, C.c_uint64(12)) == 0
    K0 = I0 * np.uint64(4) + J0
    assert lib.GxB_Vector_build_FC64(v, _p(K0), _p(X0), C.c_uint64(3), None) == 0
    wK, wY = np.zeros(3, np.uint64), np.zeros(3, np.complex128)
    nn = C.c_uint64(3)
    assert lib.GxB_Vector_extractTuples_FC64(_p(wK), _p(wY), C.byref(nn), v) == 0 and nn.value == 3
    K, Y = np.zeros(3, np.uint64), np.zeros(3, np.complex128)
    nn = C.c_uint64(3)
    assert lib.GrBX_Vector_extractTuples_at(_p(K), _p(Y), C.byref(nn), v, 0) == 0 and nn.value == 3
    assert np.array_equal(K, wK) and np.array_equal(K, K0) and np.array_equal(_bits(Y), _bits(wY)) and np.array_equal(_bits(Y), _bits(X0))
    lib.GrB_Matrix_free(C.byref(A)); lib.GrB_Vector_free(C.byref(v))


def test_info_codes(gb):
    A, (I0, J0, X0) = _matrix(gb, gb.FP64)
    n = len(I0)
    v = gb.Vector.from_arrays(I0 * np.uint64(30) + J0, X0, 1200, gb.FP64)
    I, J, X = np.full(n, 77, np.uint64), np.full(n, 77, np.uint64), np.full(n, 77.0)
    at, vat = gb.lib.GrBX_Matrix_extractTuples_at, gb.lib.GrBX_Vector_extractTuples_at
    # the capacity is too small: refused before anything is written, and *n keeps the capacity
    for args in ((_p(I), _p(J), _p(X)), (_p(I), None, None), (None, _p(J), None), (None, None, _p(X))):
        nn = C.c_uint64(n - 1)
        assert at(*args, C.byref(nn), A._h, 0) == INSUFFICIENT_SPACE and nn.value == n - 1
    nn = C.c_uint64(n - 1)
    assert vat(_p(I), _p(X), C.byref(nn), v._h, 0) == INSUFFICIENT_SPACE and nn.value == n - 1
    assert (I == 77).all() and (J == 77).all() and (X == 77.0).all()
    # all outputs NULL: nvals, whatever the capacity says
    for cap in (0, n, 10 * n):
        nn = C.c_uint64(cap)
        assert at(None, None, None, C.byref(nn), A._h, 0) == 0 and nn.value == n
        nn = C.c_uint64(cap)
        assert vat(None, None, C.byref(nn), v._h, 0) == 0 and nn.value == n
    # one stream NULL: the others are written
    nn = C.c_uint64(n)
    assert at(None, _p(J), None, C.byref(nn), A._h, 0) == 0 and np.array_equal(J, J0) and (I == 77).all() and (X == 77.0).all()
    # a location that is neither 0 nor 1; a NULL n; a NULL container
    for loc in (2, -1, 7):
        nn = C.c_uint64(n)
        assert at(_p(I), _p(J), _p(X), C.byref(nn), A._h, loc) == INVALID_VALUE and vat(_p(I), _p(X), C.byref(nn), v._h, loc) == INVALID_VALUE
    assert (I == 77).all()
    assert at(_p(I), _p(J), _p(X), None, A._h, 0) == NULL_POINTER and vat(_p(I), _p(X), None, v._h, 0) == NULL_POINTER
    assert at(_p(I), _p(J), _p(X), None, A._h, 2) == NULL_POINTER
    nn = C.c_uint64(n)
    assert at(_p(I), _p(J), _p(X), C.byref(nn), None, 0) == NULL_POINTER and vat(_p(I), _p(X), C.byref(nn), None, 0) == NULL_POINTER


def test_to_tensors_cpu_path(gb):
    torch = pytest.importorskip("torch")
    A, (I0, J0, X0) = _matrix(gb, gb.FP32)
    I, J, V = A.to_tensors()
    assert I.dtype == torch.int64 and J.dtype == torch.int64 and V.dtype == torch.float32 and I.is_contiguous() and V.is_contiguous()
    assert np.array_equal(I.cpu().numpy().astype(np.uint64), I0) and np.array_equal(J.cpu().numpy().astype(np.uint64), J0)
    assert np.array_equal(_bits(V.cpu().numpy()), _bits(X0))
    I2, J2 = A.to_tensors(values=False)
    assert torch.equal(I2, I) and torch.equal(J2, J)
    B = gb.Matrix.from_tensors(I, J, V, 40, 30)
    assert B.type is gb.FP32 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(B.to_arrays(), A.to_arrays()))
    v = gb.Vector.from_arrays(I0 * np.uint64(30) + J0, X0.astype(np.int16), 1200, gb.INT16)
    K, W = v.to_tensors()
    assert K.dtype == torch.int64 and W.dtype == torch.int16
    assert np.array_equal(K.cpu().numpy().astype(np.uint64), v.to_arrays()[0]) and np.array_equal(W.cpu().numpy(), v.to_arrays()[1])
    (K2,) = v.to_tensors(values=False)
    assert torch.equal(K2, K)
    u = gb.Vector.from_tensors(K, W, 1200)
    assert u.type is gb.INT16 and all(np.array_equal(a, b) for a, b in zip(u.to_arrays(), v.to_arrays()))
    # empty containers: empty tensors of the right dtypes
    E = gb.Matrix.sparse(gb.UINT8, 5, 5)
    I, J, V = E.to_tensors()
    assert I.numel() == 0 and J.numel() == 0 and V.numel() == 0 and V.dtype == torch.uint8
    (K,) = gb.Vector.sparse(gb.FP64, 9).to_tensors(values=False)
    assert K.numel() == 0 and K.dtype == torch.int64
    # a mismatching request: tensors of one type do not build a container of another, and a type without a torch dtype is named
    I, J, V = A.to_tensors()
    with pytest.raises(TypeError):
        gb.Matrix.from_tensors(I, J, V, 40, 30, gb.FP64)
    from pygraphblas_amd.matrix import _torch_dtype

    class NoSuchDtype:
        pass
    with pytest.raises(TypeError, match="NoSuchDtype"):
        _torch_dtype(NoSuchDtype)
    assert _torch_dtype(gb.FP32) is torch.float32 and _torch_dtype(gb.BOOL) is torch.bool and _torch_dtype(gb.INT64) is torch.int64


def test_tuples_geometry_under_the_sanitizers(tmp_path):
    """Tile and grid counts at their edges, the row of an entry by bisection and gallop over long rows and runs of empty rows, every probe inside the row pointer:
    a host program of its own with the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "tuples_geometry_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "tuples_geometry_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "tuples geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
