"""The parts of a full matrix times a vector (the gemv_full route of GrB_mxv / GrB_vxm) that need no device: GrBX_gemv_geometry in the header, the binding and the
library, and what its numbers must satisfy for the kernels' thread layout; the integer geometry of grb_gemv_geom.hpp under the address and undefined-behaviour
sanitizers (a stand-alone host program, tests/gemv_geometry_check.cpp, built with g++); the default rule as pure arithmetic; and the product model on the call
the route serves, which is what tests/test_gemv_full_gpu.py compares the route with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import matrix_model as MM
import vector_model as VM
import product_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER = 4
MIN_INNER = 1 << 16          # GEMV_DEFAULT_MIN_INNER of grb_gemv_geom.hpp (GrBX_gemv_geometry does not report it)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/gemv_geometry_check.cpp built once with the address and undefined-behaviour sanitizers: a host program of its own, nothing is loaded into Python."""
    exe = str(tmp_path_factory.mktemp("gemv") / "gemv_geometry_check")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "gemv_geometry_check.cpp"), "-o", exe])
    return exe


def library_rule(exe, rows, cols, transposed=False):
    """(what gemv_by_default of grb_gemv_geom.hpp says of a rows x cols matrix, read as it lies or transposed, with GEMV_FULL_MIN_WORK of grb_route.hpp, that constant): the text the library compiles."""
    run = subprocess.run([exe, str(rows), str(cols), str(int(transposed))], capture_output=True, text=True, timeout=60)
    word = run.stdout.split()
    assert run.returncode == 0 and word[0] == "rule" and word[2] == "min_work", run.stdout + run.stderr
    return bool(int(word[1])), int(word[3])


def default_rule_shapes(min_work):
    """(rows, cols) just below and just above the default rule's threshold rows cols >= min_work, with the shortest rows the rule admits (MIN_INNER = 2^16 of
    grb_gemv_geom.hpp): what test_gemv_full_gpu.py runs with the hooks unset."""
    cols = MIN_INNER
    rows = -(-min_work // cols)
    return (rows - 1, cols), (rows, cols)


def geometry(gb):
    out = (C.c_uint64 * 10)()
    assert gb.lib.GrBX_gemv_geometry(out) == 0
    return tuple(int(v) for v in out)


def test_symbol_header_and_geometry(gb):
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    name = "GrBX_gemv_geometry"
    assert name in gb._capi.functions and name not in gb._capi.missing
    assert "GrB_Info " + name + "(" in header
    load, gmax, L, waves, cap, rt, maxch, min_work, unroll, pack = geometry(gb)
    assert load == 16 and gmax == 64                                              # the widest global load; a row that shares a wave fits one
    assert L % (64 * load) == 0 and L > gmax                                      # a chunk is whole rounds of a wave's packets, for one-byte values too
    assert 1 <= waves <= 16 and rt % waves == 0 and rt & (rt - 1) == 0 and maxch >= 2 and cap >= 1 and min_work >= 1 and unroll >= 1 and 1 <= pack <= load
    assert gb.lib.GrBX_gemv_geometry(None) == NULL_POINTER


def test_default_rule_is_arithmetic(gb, check_exe):
    """The rule is: not transposed, rows of at least MIN_INNER values, rows cols >= GEMV_FULL_MIN_WORK — asked of the library's own gemv_by_default through the
    stand-alone program, on both sides of the threshold and of each shape condition, and where the product passes 2^64."""
    W = geometry(gb)[7]
    (r0, c0), (r1, c1) = default_rule_shapes(W)
    assert r0 * c0 < W <= r1 * c1 and (r1 - r0, c1 - c0) == (1, 0)
    assert library_rule(check_exe, r1, c1) == (True, W) and library_rule(check_exe, r0, c0) == (False, W)      # (and the entry point reports the constant the rule uses)
    assert library_rule(check_exe, r1, c1, True)[0] is False                     # layout T lost most of its measured points
    assert library_rule(check_exe, 2 * r1, c1 - 1)[0] is False and library_rule(check_exe, W, 64)[0] is False     # shorter rows: lost as well
    assert library_rule(check_exe, 1, W)[0] is True and library_rule(check_exe, 0, W)[0] is False
    assert library_rule(check_exe, 1 << 40, 1 << 40)[0] is True                   # the work count saturates


def test_gemv_geometry_under_the_sanitizers(check_exe):
    """The chunk, piece, packet and slab maps cover [0, m) x [0, k) exactly once around every edge, the slots never overlap, the grid-stride walks under the cap,
    saturating work counts near 2^64: a host program of its own with the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "gemv geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_product_model_on_the_gemv_call():
    """X 3 x 2 full: X w and y' X in the model — holes in the operand contribute nothing, an empty operand gives an empty T (the write-back's result), a complemented
    mask leaves the other entries, MIN_PLUS shows the fold is the semiring's."""
    Xd = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 0.25]])
    X = MM.Mat(3, 2, np.arange(6), Xd.ravel())
    w = VM.Vec(np.array([2.0, 4.0]), np.array([True, True])); y = VM.Vec(np.array([1.0, 2.0, -1.0]), np.array([True, True, True]))
    t = PM.mxv(VM.empty(3, "FP64"), X, w, "PLUS", "TIMES", "FP64")
    assert t.pres.all() and np.array_equal(t.val, Xd @ w.val)
    t = PM.vxm(VM.empty(2, "FP64"), y, X, "PLUS", "TIMES", "FP64")
    assert t.pres.all() and np.array_equal(t.val, y.val @ Xd)
    t = PM.mxv(VM.empty(2, "FP64"), X, y, "PLUS", "TIMES", "FP64", tran=True)
    assert t.pres.all() and np.array_equal(t.val, Xd.T @ y.val)
    holed = VM.Vec(np.array([2.0, 99.0]), np.array([True, False]))
    t = PM.mxv(VM.empty(3, "FP64"), X, holed, "PLUS", "TIMES", "FP64")
    assert t.pres.all() and np.array_equal(t.val, Xd[:, 0] * 2.0)                 # every row still has an entry: A is full
    t = PM.mxv(VM.Vec(np.array([7.0, 8.0, 9.0]), np.array([True, False, True])), X, VM.empty(2, "FP64"), "PLUS", "TIMES", "FP64")
    assert t.pres.tolist() == [False, False, False]                                # an empty T replaces w where nothing masks it
    t = PM.mxv(VM.Vec(np.array([7.0, 8.0, 9.0]), np.array([True, False, True])), X, VM.empty(2, "FP64"), "PLUS", "TIMES", "FP64", accum=("PLUS", "FP64"))
    assert t.pres.tolist() == [True, False, True] and t.val[0] == 7.0 and t.val[2] == 9.0
    mask = VM.Vec(np.array([1, 0, 1], np.int8), np.array([True, True, False]))
    t = PM.mxv(VM.empty(3, "FP64"), X, w, "PLUS", "TIMES", "FP64", mask=mask, comp=True)
    assert t.pres.tolist() == [False, True, True] and np.array_equal(t.val[1:], (Xd @ w.val)[1:])
    t = PM.vxm(VM.empty(2, "FP64"), y, X, "MIN", "PLUS", "FP64")
    assert np.array_equal(t.val, [min(y.val[l] + Xd[l, j] for l in range(3)) for j in range(2)])
