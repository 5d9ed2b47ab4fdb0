"""The parts of the product of two full matrices (the gemm_full route of GrB_mxm) that need no device: GrBX_gemm_geometry in the header, the binding and the
library, and what its numbers must satisfy for the kernel's thread layout; the integer geometry of grb_gemm_geom.hpp under the address and undefined-behaviour
sanitizers (a stand-alone host program, tests/gemm_geometry_check.cpp, built with g++); the default rule as pure arithmetic; and the product model on the call
the route serves, which is what tests/test_gemm_full_gpu.py compares the route with: a dense numpy product, every position an entry."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import matrix_model as MM
import product_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER = 4


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/gemm_geometry_check.cpp built once with the address and undefined-behaviour sanitizers: a host program of its own, nothing is loaded into Python."""
    exe = str(tmp_path_factory.mktemp("gemm") / "gemm_geometry_check")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_geometry_check.cpp"), "-o", exe])
    return exe


def library_rule(exe, m, k, n, plain_mask):
    """(what gemm_by_default of grb_gemm_geom.hpp says of the call with GEMM_FULL_MIN_WORK of grb_route.hpp, that constant): the text the library compiles."""
    run = subprocess.run([exe, str(m), str(k), str(n), str(int(plain_mask))], capture_output=True, text=True, timeout=60)
    word = run.stdout.split()
    assert run.returncode == 0 and word[0] == "rule" and word[2] == "min_work", run.stdout + run.stderr
    return bool(int(word[1])), int(word[3])


def default_rule_shapes(min_work):
    """(m, k, n) just below and just above the default rule's threshold m k n >= min_work, with m = n: what test_gemm_full_gpu.py runs with the hooks unset."""
    k = 4
    n = 2
    while n * n * k < min_work:
        n += 1
    return (n - 1, k, n - 1), (n, k, n)


def geometry(gb):
    out = (C.c_uint64 * 9)()
    assert gb.lib.GrBX_gemm_geometry(out) == 0
    return tuple(int(v) for v in out)


def test_symbol_header_and_geometry(gb):
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    name = "GrBX_gemm_geometry"
    assert name in gb._capi.functions and name not in gb._capi.missing
    assert "GrB_Info " + name + "(" in header
    tm, tn, ttm, ttn, kt, waves, cap, min_work, talln = geometry(gb)
    threads = waves * 64
    for a, b in ((tm, tn), (ttm, ttn)):
        assert a * b == threads * 16 and a % 4 == 0 and b % 4 == 0               # one 4 x 4 register block per thread
        assert (a * kt) % threads == 0 and (b * kt) % threads == 0               # the staging loops: whole rounds of the workgroup
    assert (tm * tn) % (waves * 64 * 16) == 0 and kt in (16, 32) and 1 <= waves <= 16 and cap >= 1 and min_work >= 1
    assert 1 <= talln <= ttn and ttn < tn and ttm > tm                           # a narrow result is one tall tile wide
    assert gb.lib.GrBX_gemm_geometry(None) == NULL_POINTER


def test_default_rule_is_arithmetic(gb, check_exe):
    """The rule is m k n >= GEMM_FULL_MIN_WORK without a plain mask, from two columns and from a minimum of tiles of T, nothing else — asked of the library's own gemm_by_default through the
    stand-alone program: the two shapes the GPU test runs straddle the threshold by one row and one column, and one column is off whatever the work."""
    W = geometry(gb)[7]
    (m0, k0, n0), (m1, k1, n1) = default_rule_shapes(W)
    assert m0 * k0 * n0 < W <= m1 * k1 * n1 and (m1 - m0, k1 - k0, n1 - n0) == (1, 0, 1)
    assert library_rule(check_exe, m1, k1, n1, False) == (True, W) and library_rule(check_exe, m0, k0, n0, False) == (False, W)      # (and the entry point reports the constant the rule uses)
    assert library_rule(check_exe, m1, k1, n1, True)[0] is False                  # a plain mask is the sddmm route's
    assert library_rule(check_exe, W, 4, 1, False)[0] is False and library_rule(check_exe, W, 4, 2, False)[0] is True      # n = 1
    assert library_rule(check_exe, W, 1, 2, False)[0] is True and library_rule(check_exe, W // 2, 1, 2, False)[0] is True and library_rule(check_exe, W // 2 - 1, 1, 2, False)[0] is False
    assert library_rule(check_exe, 1 << 31, 1 << 31, 1 << 31, False)[0] is True   # the work count saturates
    ttm, ttn = geometry(gb)[2:4]
    assert library_rule(check_exe, ttm, -(-W // (ttm * ttn)), ttn, False)[0] is False      # enough work in one tile of T: too few tiles (the condition the measurements added)
    for w in (1, 7, 1 << 18, (1 << 18) + 1, 10 ** 9):
        lo, hi = default_rule_shapes(w)
        assert (lo[0] * lo[1] * lo[2] < w or lo[0] < 2) and hi[0] * hi[1] * hi[2] >= w and hi[2] >= 2


def test_gemm_geometry_under_the_sanitizers(check_exe):
    """Tile maps that cover [0, m) x [0, n) exactly once around the tile sizes and the switch between the two shapes, the grid-stride walk under the cap, the k
    steps for k = 1 .. 3 KT + 1, the route's overflow guard and the default rule: a host program of its own with the address and undefined-behaviour sanitizers;
    nothing is loaded into Python."""
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "gemm geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_product_model_on_the_gemm_call():
    """X 3 x 2 and W 2 x 4 full: the model's product is the dense X W with every position an entry, under each of the four layouts; MIN_PLUS shows the fold is the
    semiring's; a complemented mask leaves the other entries."""
    Xd = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 0.25]]); Wd = np.array([[2.0, 1.0, -1.0, 4.0], [0.5, 0.5, 8.0, -2.0]])
    X = MM.Mat(3, 2, np.arange(6), Xd.ravel()); W = MM.Mat(2, 4, np.arange(8), Wd.ravel())
    Xt = MM.Mat(2, 3, np.arange(6), np.ascontiguousarray(Xd.T).ravel()); Wt = MM.Mat(4, 2, np.arange(8), np.ascontiguousarray(Wd.T).ravel())
    dense = Xd @ Wd
    for a, b, ta, tb in ((X, W, False, False), (X, Wt, False, True), (Xt, W, True, False), (Xt, Wt, True, True)):
        t = PM.mxm(MM.empty(3, 4, "FP64"), a, b, "PLUS", "TIMES", "FP64", tran_a=ta, tran_b=tb)
        assert t.keys.tolist() == list(range(12)) and np.array_equal(t.vals, dense.ravel())
    t = PM.mxm(MM.empty(3, 4, "FP64"), X, W, "MIN", "PLUS", "FP64")
    assert np.array_equal(t.vals, [min(Xd[i, l] + Wd[l, j] for l in range(2)) for i in range(3) for j in range(4)])
    M = MM.Mat(3, 4, np.array([1, 6]), np.array([1, 0], np.int8))
    t = PM.mxm(MM.empty(3, 4, "FP64"), X, W, "PLUS", "TIMES", "FP64", mask=M, comp=True)
    assert t.keys.tolist() == [p for p in range(12) if p != 1] and np.array_equal(t.vals, np.delete(dense.ravel(), 1))
