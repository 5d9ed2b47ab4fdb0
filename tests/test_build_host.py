"""The parts of build-from-tuples that need no device: the three new entry points, GrBX_*_build_at with host arrays against GrB_*_build_<T>, a build below the
threshold staying on the host mirror, Matrix.from_tensors / Vector.from_tensors with CPU tensors, and the key arithmetic of grb_build_keys.hpp under the address
and undefined-behaviour sanitizers (a stand-alone host program, tests/build_keys_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, INVALID_VALUE, OUTPUT_NOT_EMPTY, INDEX_OUT_OF_BOUNDS = 4, 5, 9, 12


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def thresholds(gb):
    out = (C.c_uint64 * 3)()
    assert gb.lib.GrBX_build_thresholds(out) == 0
    return [int(v) for v in out]


def test_symbols_and_thresholds(gb):
    for name in ("GrBX_Matrix_build_at", "GrBX_Vector_build_at", "GrBX_build_thresholds"):
        assert name in gb._capi.functions and name not in gb._capi.missing, name
    dev_min, serial, serial_max = thresholds(gb)
    assert dev_min > 9, "the 3 x 3 docstring examples keep the host route"
    assert 2 <= serial < 64 and 129 < serial_max
    assert gb.lib.GrBX_build_thresholds(None) == NULL_POINTER
    assert hasattr(gb.Matrix, "from_tensors") and hasattr(gb.Vector, "from_tensors")


def test_build_at_host_arrays_is_build(gb):
    rng = np.random.default_rng(5)
    os.environ["GRB_MI355X_BUILD"] = "0"
    try:
        for typ, op in ((gb.FP64, "PLUS"), (gb.INT16, "PLUS"), (gb.BOOL, "LOR"), (gb.INT64, "MIN"), (gb.FP32, "SECOND"), (gb.UINT8, None)):
            n = 300
            I = rng.integers(0, 40, n).astype(np.uint64); J = rng.integers(0, 30, n).astype(np.uint64)
            if op is None:
                flat = rng.choice(1200, n, replace=False); I, J = (flat // 30).astype(np.uint64), (flat % 30).astype(np.uint64)
            X = (rng.standard_normal(n) * 50).astype(typ._np)
            dup = C.c_void_p(getattr(typ, op).get_op()) if op else None
            want = gb.Matrix.from_arrays(I, J, X, 40, 30, typ, dup=getattr(typ, op) if op else None).to_arrays()
            m = gb.Matrix.sparse(typ, 40, 30)
            assert gb.lib.GrBX_Matrix_build_at(m._h, _p(I), _p(J), _p(X), C.c_uint64(n), dup, 0) == 0
            got = m.to_arrays()
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want)), typ.__name__
            wantv = gb.Vector.from_arrays(I * np.uint64(30) + J, X, 1200, typ, dup=getattr(typ, op) if op else None).to_arrays()
            v = gb.Vector.sparse(typ, 1200)
            K = I * np.uint64(30) + J
            assert gb.lib.GrBX_Vector_build_at(v._h, _p(K), _p(X), C.c_uint64(n), dup, 0) == 0
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(v.to_arrays(), wantv)), typ.__name__
    finally:
        os.environ.pop("GRB_MI355X_BUILD", None)


def test_build_at_outcomes(gb):
    I = np.array([1, 1, (1 << 32) + 3], np.uint64); J = np.zeros(3, np.uint64); X = np.ones(3)
    m = gb.Matrix.sparse(gb.FP64, 10, 10)
    os.environ["GRB_MI355X_BUILD"] = "0"
    try:
        assert gb.lib.GrBX_Matrix_build_at(m._h, _p(I), _p(J), _p(X), C.c_uint64(3), None, 0) == INDEX_OUT_OF_BOUNDS and m.nvals == 0
        assert gb.lib.GrBX_Matrix_build_at(m._h, _p(I), _p(J), _p(X), C.c_uint64(2), None, 0) == INVALID_VALUE and m.nvals == 0
        assert gb.lib.GrBX_Matrix_build_at(m._h, _p(I), _p(J), _p(X), C.c_uint64(2), None, 2) == INVALID_VALUE
        assert gb.lib.GrBX_Matrix_build_at(m._h, None, _p(J), _p(X), C.c_uint64(2), None, 0) == NULL_POINTER
        assert gb.lib.GrBX_Matrix_build_at(None, _p(I), _p(J), _p(X), C.c_uint64(2), None, 0) == NULL_POINTER
        assert gb.lib.GrBX_Vector_build_at(None, _p(I), _p(X), C.c_uint64(2), None, 0) == NULL_POINTER
        assert gb.lib.GrBX_Matrix_build_at(m._h, _p(I), _p(J), _p(X), C.c_uint64(2), C.c_void_p(gb.FP64.PLUS.get_op()), 0) == 0 and sorted(m) == [(1, 0, 2.0)]
        assert gb.lib.GrBX_Matrix_build_at(m._h, _p(I), _p(J), _p(X), C.c_uint64(1), None, 0) == OUTPUT_NOT_EMPTY and sorted(m) == [(1, 0, 2.0)]
    finally:
        os.environ.pop("GRB_MI355X_BUILD", None)


def test_small_default_build_stays_on_the_host_mirror(gb):
    """Below BUILD_DEVICE_MIN_TUPLES nothing changes, with or without a device: the mirror holds the result and no plan word is left."""
    os.environ.pop("GRB_MI355X_BUILD", None)
    n = min(thresholds(gb)[0] - 1, 500)
    I = np.arange(n, dtype=np.uint64); X = np.arange(n, dtype=np.float64)
    A = gb.Matrix.from_arrays(I, I, X, n, n, gb.FP64)
    w = C.c_int(-1)
    assert gb.lib.GrBX_Matrix_residency(A._h, C.byref(w)) == 0 and w.value == 1
    assert "build<" not in gb.last_kernel_plan()
    assert A.nvals == n


def test_from_tensors_cpu(gb):
    torch = pytest.importorskip("torch")
    I = torch.tensor([2, 0, 2, 1], dtype=torch.int64); J = torch.tensor([1, 0, 1, 1], dtype=torch.int64); V = torch.tensor([1.5, 2.0, 0.25, 4.0], dtype=torch.float64)
    A = gb.Matrix.from_tensors(I, J, V, 3, 2, dup=gb.FP64.PLUS)
    assert A.type is gb.FP64 and sorted(A) == [(0, 0, 2.0), (1, 1, 4.0), (2, 1, 1.75)]
    v = gb.Vector.from_tensors(I, V.to(torch.float32), 3, gb.FP32, dup=gb.FP32.SECOND)
    assert sorted(v) == [(0, 2.0), (1, 4.0), (2, 0.25)]
    with pytest.raises(TypeError):
        gb.Matrix.from_tensors(I, J, V, 3, 2, gb.FP32)              # no cast
    with pytest.raises(TypeError):
        gb.Matrix.from_tensors(I.to(torch.int32), J, V, 3, 2)
    with pytest.raises(ValueError):
        gb.Matrix.from_tensors(I[:3], J, V, 3, 2)


def test_build_keys_under_the_sanitizers(tmp_path):
    """Bit counts for dimensions 1, 2, 2^16, 2^16 + 1 and the device maximum, pack / unpack at rbits + cbits = 32 and 33, the bounds test on untruncated
    indices and the route predicate: a host program of its own with the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "build_keys_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "build_keys_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "build keys ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
