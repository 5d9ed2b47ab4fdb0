"""The parts of the full-operand product (the spmm_full route of GrB_mxm) that need no device: the three entry points in the header, the binding and the library;
GrBX_spmm_geometry; the refusals of GrBX_Matrix_import_Full / export_Full that come before a device is asked for; the integer geometry of grb_spmm_geom.hpp under
the address and undefined-behaviour sanitizers (a stand-alone host program, tests/spmm_geometry_check.cpp); and the product model on a full operand, which is
what tests/test_spmm_full_gpu.py compares the route with: a dense numpy product on the non-empty rows of A, no entry elsewhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import matrix_model as MM
import product_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, INVALID_VALUE, DOMAIN_MISMATCH = 4, 5, 7


def test_symbols_header_and_geometry(gb):
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    for name in ("GrBX_Matrix_import_Full", "GrBX_Matrix_export_Full", "GrBX_spmm_geometry"):
        assert name in gb._capi.functions and name not in gb._capi.missing, name
        assert "GrB_Info " + name + "(" in header
    out = (C.c_uint64 * 5)()
    assert gb.lib.GrBX_spmm_geometry(out) == 0
    L, slab, waves, cap, min_products = (int(v) for v in out)
    assert L >= 2 and slab >= 64 and slab % 64 == 0 and 1 <= waves <= 16 and cap >= 1 and min_products >= 1
    assert gb.lib.GrBX_spmm_geometry(None) == NULL_POINTER
    assert hasattr(gb.Matrix, "from_dense") and hasattr(gb.Matrix, "to_dense_tensor") and isinstance(gb.Matrix.is_full, property)


def test_import_full_refusals_before_a_device(gb):
    """A complex type, a shape beyond the 32-bit layout, a bad location and null arguments are refused whether or not a device exists; a zero dimension gives an
    empty matrix without one."""
    x = np.zeros(4, np.float64); p = x.ctypes.data_as(C.c_void_p); u64 = C.c_uint64
    imp = gb.lib.GrBX_Matrix_import_Full
    h = C.c_void_p()
    assert imp(C.byref(h), C.c_void_p(gb._capi.handle("GxB_FC64")), u64(2), u64(2), p, 0) == DOMAIN_MISMATCH
    assert imp(C.byref(h), C.c_void_p(gb._capi.handle("GxB_FC32")), u64(2), u64(2), p, 0) == DOMAIN_MISMATCH
    assert imp(C.byref(h), C.c_void_p(gb.FP64._h), u64(1 << 16), u64(1 << 16), p, 0) == INVALID_VALUE                  # 2^32 positions
    assert imp(C.byref(h), C.c_void_p(gb.FP64._h), u64((1 << 32) - 16), u64(1), p, 0) == INVALID_VALUE
    assert imp(C.byref(h), C.c_void_p(gb.FP64._h), u64(2), u64(2), p, 2) == INVALID_VALUE
    assert imp(None, C.c_void_p(gb.FP64._h), u64(2), u64(2), p, 0) == NULL_POINTER
    assert imp(C.byref(h), None, u64(2), u64(2), p, 0) == NULL_POINTER
    assert imp(C.byref(h), C.c_void_p(gb.FP64._h), u64(2), u64(2), None, 0) == NULL_POINTER
    assert h.value is None
    for nr, nc in ((0, 5), (5, 0), (0, 0)):
        m = gb.Matrix.from_dense(np.zeros((nr, nc), np.float32))
        assert m.type is gb.FP32 and (m.nrows, m.ncols, m.nvals) == (nr, nc, 0)
        assert m.is_full                                                         # (no position is without an entry)
        t = m.to_dense_tensor()
        assert tuple(t.shape) == (nr, nc)
    assert gb.lib.GrBX_Matrix_export_Full(None, p, 0) == NULL_POINTER


def test_from_dense_argument_checks(gb):
    import pytest
    with pytest.raises(ValueError, match="two-dimensional"):
        gb.Matrix.from_dense(np.zeros(4))
    with pytest.raises(TypeError, match="no GraphBLAS type"):
        gb.Matrix.from_dense(np.zeros((2, 2), np.complex128))
    import torch
    with pytest.raises(TypeError, match="does not cast"):
        gb.Matrix.from_dense(torch.zeros((2, 2), dtype=torch.float32), gb.FP64)
    m = gb.Matrix.from_lists([0, 1], [0, 1], [1.0, 2.0], 2, 2, gb.FP64)          # a position without an entry: the library's own refusal
    assert not m.is_full
    with pytest.raises(gb.InvalidValue):
        m.to_dense_tensor()


def test_spmm_geometry_under_the_sanitizers(tmp_path):
    """Group widths for k = 1 .. 130, slab and chunk counts at their edges, the chunks covering a row once, the long rows' scratch slots disjoint and inside the
    allocation, T's row pointer against a loop, the overflow test around 2^32 - 16: a host program of its own with the address and undefined-behaviour
    sanitizers; nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "spmm_geometry_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "spmm_geometry_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "spmm geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_product_model_on_a_full_operand():
    """3 x 4 times a full 4 x 3: the model's product is the dense numpy product on the rows of A that hold an entry — all three columns there — and has no entry
    in the row that holds none.  Absent entries of A contribute nothing (they are not zeros: MIN_PLUS shows it)."""
    I = np.array([0, 0, 2, 2, 2]); J = np.array([1, 3, 0, 1, 2])
    X = np.array([2.0, -1.5, 0.5, 4.0, 1.0])
    A = MM.from_coo(3, 4, I, J, X)
    Bd = np.arange(1, 13, dtype=np.float64).reshape(4, 3) / 4
    B = MM.Mat(4, 3, np.arange(12), Bd.ravel())
    t = PM.mxm(MM.empty(3, 3, "FP64"), A, B, "PLUS", "TIMES", "FP64")
    Ad = np.zeros((3, 4)); Ad[I, J] = X
    dense = Ad @ Bd
    assert t.keys.tolist() == [0, 1, 2, 6, 7, 8]                                  # rows 0 and 2 full, row 1 absent
    assert np.array_equal(t.vals, dense[[0, 2]].ravel())
    rp, ci, _ = MM.to_csr(t)
    assert rp.tolist() == [0, 3, 3, 6] and ci.tolist() == [0, 1, 2, 0, 1, 2]
    t = PM.mxm(MM.empty(3, 3, "FP64"), A, B, "MIN", "PLUS", "FP64")
    exp = np.array([[min(X[e] + Bd[J[e], j] for e in range(5) if I[e] == i) for j in range(3)] for i in (0, 2)])
    assert t.keys.tolist() == [0, 1, 2, 6, 7, 8] and np.array_equal(t.vals, exp.ravel())
