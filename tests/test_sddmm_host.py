"""The parts of the masked product of two full matrices (the sddmm route of GrB_mxm) that need no device: GrBX_sddmm_geometry in the header, the binding and the
library; Matrix.sddmm; the integer geometry of grb_sddmm_geom.hpp under the address and undefined-behaviour sanitizers (a stand-alone host program,
tests/sddmm_geometry_check.cpp, built with g++); the default rule as pure arithmetic; and the product model on the call the route serves, which is what
tests/test_sddmm_gpu.py compares the route with: dense numpy dot products at the mask's entries, no entry elsewhere."""
import ctypes as C
import os
import subprocess

import numpy as np

import matrix_model as MM
import product_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER = 4


def default_rule_shapes(min_work):
    """(m, k, n) just below and just above the default rule's threshold m k n >= min_work, with m = n: what test_sddmm_gpu.py runs with the hook unset."""
    k = 4
    n = 2
    while n * n * k < min_work:
        n += 1
    return (n - 1, k, n - 1), (n, k, n)


def test_symbol_header_geometry_and_method(gb):
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    name = "GrBX_sddmm_geometry"
    assert name in gb._capi.functions and name not in gb._capi.missing
    assert "GrB_Info " + name + "(" in header
    out = (C.c_uint64 * 4)()
    assert gb.lib.GrBX_sddmm_geometry(out) == 0
    tile, waves, cap, min_work = (int(v) for v in out)
    assert tile >= 2 and tile % (waves * 64) == 0 and 1 <= waves <= 16 and cap >= 1 and min_work >= 1
    assert gb.lib.GrBX_sddmm_geometry(None) == NULL_POINTER
    assert callable(getattr(gb.Matrix, "sddmm", None))


def test_default_rule_is_arithmetic(gb):
    """The rule is m k n >= SDDMM_MIN_WORK, nothing else: the two shapes the GPU test runs straddle it by one row and one column."""
    out = (C.c_uint64 * 4)()
    assert gb.lib.GrBX_sddmm_geometry(out) == 0
    W = int(out[3])
    (m0, k0, n0), (m1, k1, n1) = default_rule_shapes(W)
    assert m0 * k0 * n0 < W <= m1 * k1 * n1 and (m1 - m0, k1 - k0, n1 - n0) == (1, 0, 1)
    for w in (1, 7, 1 << 18, (1 << 18) + 1, 10 ** 9):
        lo, hi = default_rule_shapes(w)
        assert (lo[0] * lo[1] * lo[2] < w or lo[0] < 2) and hi[0] * hi[1] * hi[2] >= w


def test_sddmm_geometry_under_the_sanitizers(tmp_path):
    """Group widths, live lanes and loop trips for k = 1 .. 300, the butterfly's lanes per step (lane 0 ends with every product exactly once and never meets a lane
    without one), tiles to entry ranges around the tile size and the grid cap, the row bisection against a walk, the overflow guards: a host program of its own
    with the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
    exe = str(tmp_path / "sddmm_geometry_check")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "sddmm_geometry_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sddmm geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_product_model_on_the_sddmm_call():
    """X 3 x 2 and Y 4 x 2 full, a mask of four entries (one row without any): the model's masked product with INP1 transposed is the dense X Y' at the mask's
    entries and nothing elsewhere; a valued mask drops its false entry; MIN_PLUS shows the fold is the semiring's."""
    Xd = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 0.25]]); Yd = np.array([[2.0, 1.0], [-1.0, 4.0], [0.5, 0.5], [8.0, -2.0]])
    X = MM.Mat(3, 2, np.arange(6), Xd.ravel()); Y = MM.Mat(4, 2, np.arange(8), Yd.ravel())
    keys = np.array([0 * 4 + 1, 0 * 4 + 3, 2 * 4 + 0, 2 * 4 + 2])
    M = MM.Mat(3, 4, keys, np.array([1, 0, 2, 1], np.int8))
    dense = Xd @ Yd.T
    t = PM.mxm(MM.empty(3, 4, "FP64"), X, Y, "PLUS", "TIMES", "FP64", mask=M, struct=True, tran_b=True)
    assert t.keys.tolist() == keys.tolist() and np.array_equal(t.vals, dense.ravel()[keys])
    t = PM.mxm(MM.empty(3, 4, "FP64"), X, Y, "PLUS", "TIMES", "FP64", mask=M, tran_b=True)
    assert t.keys.tolist() == keys[[0, 2, 3]].tolist() and np.array_equal(t.vals, dense.ravel()[keys[[0, 2, 3]]])
    t = PM.mxm(MM.empty(3, 4, "FP64"), X, Y, "MIN", "PLUS", "FP64", mask=M, struct=True, tran_b=True)
    exp = [min(Xd[i, l] + Yd[j, l] for l in range(2)) for i, j in zip(keys // 4, keys % 4)]
    assert t.keys.tolist() == keys.tolist() and np.array_equal(t.vals, exp)
