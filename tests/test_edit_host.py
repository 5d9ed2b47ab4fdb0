"""The parts of the in-place edits that need no device: the edit-list arithmetic of grb_edit_list.hpp against a brute-force replay (a stand-alone host program,
tests/edit_list_check.cpp, built plainly and under the address and undefined-behaviour sanitizers), and Matrix.resize / Vector.resize / element edits on
host-resident containers against a dict model — they keep the host route and stay host-resident."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "edit_list_check.cpp")
INC = "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc")


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def run_check(cmd, exe):
    subprocess.check_call(cmd)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "edit list ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_edit_list_against_a_replay(tmp_path):
    """Host compiler, no HIP: the header is plain C++."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "edit_list_check")
    run_check([cxx, "-std=c++20", "-O1", INC, SRC, "-o", exe], exe)


def test_edit_list_under_the_sanitizers(tmp_path):
    """The same program as the device compiler's host pass sees the header (its functions marked for both sides), with the address and undefined-behaviour
    sanitizers: a host program of its own, no device code, nothing loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "edit_list_check_san")
    run_check([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
               INC, SRC, "-o", exe], exe)


def test_resize_is_part_of_the_mirror(gb):
    assert "resize" in vars(gb.Matrix) and "resize" in vars(gb.Vector) and "__delitem__" in vars(gb.Vector) and "__delitem__" in vars(gb.Matrix)


def matrix_model(rng, nr, nc, n):
    model = {}
    while len(model) < n:
        model[(int(rng.integers(nr)), int(rng.integers(nc)))] = int(rng.integers(1, 100))
    return model


def matrix_of(gb, T, model, nr, nc):
    keys = sorted(model)
    return gb.Matrix.from_lists([k[0] for k in keys], [k[1] for k in keys], [model[k] for k in keys], nr, nc, T)


def check_matrix(gb, A, model, nr, nc):
    assert A.shape == (nr, nc) and A.nvals == len(model)
    I, J, X = A.to_arrays()
    keys = sorted(model)
    assert list(zip(I.tolist(), J.tolist())) == keys and X.tolist() == [model[k] for k in keys]
    assert residency(gb, A) == 1


def test_matrix_resize_on_the_host(gb):
    rng = np.random.default_rng(5)
    for T in (gb.INT16, gb.FP64):
        for nr, nc in ((30, 40), (12, 40), (30, 7), (12, 7), (50, 60), (0, 40), (30, 0), (1 << 40, 3)):
            model = matrix_model(rng, 30, 40, 150)
            A = matrix_of(gb, T, model, 30, 40)
            A.resize(nr, nc)
            check_matrix(gb, A, {k: v for k, v in model.items() if k[0] < nr and k[1] < nc}, nr, nc)
    A = matrix_of(gb, gb.INT64, {(0, 1): 42, (2, 0): 149}, 3, 3)
    A.resize()                                                   # the reference's default: GxB_INDEX_MAX both ways
    check_matrix(gb, A, {(0, 1): 42, (2, 0): 149}, 1 << 60, 1 << 60)


def test_vector_resize_on_the_host(gb):
    rng = np.random.default_rng(6)
    for T in (gb.BOOL, gb.FP32):
        for n in (100, 37, 1, 0, 250, 1 << 40):
            idx = np.sort(rng.choice(100, size=40, replace=False))
            model = {int(i): 1 for i in idx}
            v = gb.Vector.from_lists(list(model), [model[i] for i in model], 100, T)
            v.resize(n)
            want = {i: x for i, x in model.items() if i < n}
            assert v.size == n and v.nvals == len(want)
            I, X = v.to_arrays()
            assert I.tolist() == sorted(want) and X.tolist() == [want[i] for i in sorted(want)]
            assert residency(gb, v) == 1
    v = gb.Vector.from_lists([0, 1], [5, 6], 2, gb.UINT8)
    v.resize()
    assert v.size == 1 << 60 and v.to_lists() == [[0, 1], [5, 6]] and residency(gb, v) == 1


def test_element_edits_on_the_host_keep_their_route(gb):
    model = {(0, 0): 1, (1, 2): 2, (3, 3): 3}
    A = matrix_of(gb, gb.INT32, model, 4, 4)
    A[2, 2] = 7; model[(2, 2)] = 7
    del A[1, 2]; del model[(1, 2)]
    del A[1, 1]
    A[0, 0] = 9; model[(0, 0)] = 9
    assert A[2, 2] == 7 and A.get(1, 2) is None
    check_matrix(gb, A, model, 4, 4)
    v = gb.Vector.from_lists([1, 3], [10, 30], 5, gb.INT64)
    v[0] = 5
    del v[3]
    del v[4]
    assert v.to_lists() == [[0, 1], [5, 10]] and residency(gb, v) == 1
