"""The parts of index lists in HBM that need no device: the new entry points exist, location 0 is the GrB_ call, the refusals that are decided before any list
is read, a vector as an index list through the host mirror, CPU tensors as lists, and the Python surface's argument errors."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["GrBX_Vector_extract_at", "GrBX_Col_extract_at", "GrBX_Matrix_extract_at", "GrBX_Vector_assign_at", "GrBX_Matrix_assign_at", "GrBX_Row_assign_at",
         "GrBX_Col_assign_at", "GrBX_Vector_extract_Vector", "GrBX_Vector_assign_Vector", "GrBX_Matrix_extract_Vector", "GrBX_index_geometry", "GrBX_index_parse"]
GXB_RANGE = 0x7FFFFFFFFFFFFFFF


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def same(a, b):
    for x, y in zip(a.to_arrays(), b.to_arrays()):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_entry_points_exist(gb):
    for name in NAMES:
        assert name in gb._capi.functions and hasattr(gb.lib, name), name
    out = (C.c_uint64 * 2)()
    assert gb.lib.GrBX_index_geometry(out) == 0 and out[0] > 0 and out[0] % 128 == 0 and out[1] > 0      # whole waves of index pairs, a positive grid cap
    assert gb.lib.GrBX_index_geometry(None) == gb._capi.constants["GrB_NULL_POINTER"]


def test_location0_is_the_grb_call_and_refusals(gb):
    rng = np.random.default_rng(0)
    k = gb._capi.constants
    u = gb.Vector.from_arrays(np.arange(0, 40, 2, dtype=np.uint64), rng.random(20), 40, gb.FP64)
    L = np.array([4, 2, 2, 39, 0], np.uint64)
    w = gb.Vector.sparse(gb.FP64, 5)
    assert gb.lib.GrBX_Vector_extract_at(w._h, None, None, u._h, _p(L), C.c_uint64(5), None, C.c_int(0)) == 0
    same(w, u.extract(L))
    A = gb.Matrix.from_arrays(np.array([0, 1, 3], np.uint64), np.array([1, 1, 2], np.uint64), np.array([1.0, 2.0, 3.0]), 4, 4, gb.FP64)
    Cm = gb.Matrix.sparse(gb.FP64, 2, 2)
    I, J = np.array([3, 1], np.uint64), np.array([2, 1], np.uint64)
    assert gb.lib.GrBX_Matrix_extract_at(Cm._h, None, None, A._h, _p(I), C.c_uint64(2), _p(J), C.c_uint64(2), None, C.c_int(0), C.c_int(0)) == 0
    same(Cm, A.extract_matrix(I, J))
    w2 = u.dup()
    src = gb.Vector.from_arrays(np.arange(2, dtype=np.uint64), np.array([7.0, 8.0]), 2, gb.FP64)
    assert gb.lib.GrBX_Vector_assign_at(w2._h, None, None, src._h, _p(I), C.c_uint64(2), None, C.c_int(0)) == 0
    w3 = u.dup()
    w3.assign(src, I)
    same(w2, w3)
    for loc in (2, -1):
        assert gb.lib.GrBX_Vector_extract_at(w._h, None, None, u._h, _p(L), C.c_uint64(5), None, C.c_int(loc)) == k["GrB_INVALID_VALUE"]
        assert gb.lib.GrBX_Matrix_assign_at(Cm._h, None, None, A._h, _p(I), C.c_uint64(2), _p(J), C.c_uint64(2), None, C.c_int(0), C.c_int(loc)) == k["GrB_INVALID_VALUE"]
    for code in (GXB_RANGE, GXB_RANGE - 1, GXB_RANGE - 2):          # a range triple is a host form: refused before the list is looked at
        assert gb.lib.GrBX_Vector_extract_at(w._h, None, None, u._h, _p(L), C.c_uint64(code), None, C.c_int(1)) == k["GrB_INVALID_VALUE"]
    assert gb.lib.GrBX_Vector_extract_at(None, None, None, u._h, _p(L), C.c_uint64(5), None, C.c_int(0)) == k["GrB_NULL_POINTER"]
    same(w, u.extract(L))                                          # none of the refused calls wrote


def test_vector_as_index_list(gb):
    rng = np.random.default_rng(1)
    u = gb.Vector.from_arrays(np.arange(50, dtype=np.uint64), rng.random(50), 50, gb.FP64)
    iv = gb.Vector.from_arrays(np.array([1, 5, 9], np.uint64), np.array([40, 3, 3], np.int16), 12, gb.INT16)
    same(u.extract(iv), u.extract(np.array([40, 3, 3], np.uint64)))
    same(u[iv], u.extract(np.array([40, 3, 3], np.uint64)))
    A = gb.Matrix.from_arrays(np.array([3, 3, 40], np.uint64), np.array([3, 40, 1], np.uint64), np.array([1.0, 2.0, 3.0]), 50, 50, gb.FP64)
    same(A.extract_matrix(iv, iv), A.extract_matrix([40, 3, 3], [40, 3, 3]))
    same(A.extract_matrix(iv, None), A.extract_matrix([40, 3, 3], None))
    neg = gb.Vector.from_arrays(np.array([0], np.uint64), np.array([-1], np.int32), 1, gb.INT32)
    with pytest.raises(gb.base.IndexOutOfBound):
        u.extract(neg)
    for bad in (gb.FP32, gb.BOOL):
        with pytest.raises(gb.base.DomainMismatch):
            u.extract(gb.Vector.from_arrays(np.array([0], np.uint64), np.array([1], bad._np), 1, bad))
    out = gb.Vector.from_arrays(np.arange(3, dtype=np.uint64), np.arange(3, dtype=np.int64), 3, gb.INT64)
    with pytest.raises(gb.base.InvalidValue):
        out.extract(out, out=out)
    w = u.dup()
    dst = gb.Vector.from_arrays(np.array([0, 1], np.uint64), np.array([7, 9], np.uint8), 2, gb.UINT8)
    src = gb.Vector.from_arrays(np.arange(2, dtype=np.uint64), np.array([-1.0, -2.0]), 2, gb.FP64)
    w.assign(src, dst)
    w2 = u.dup()
    w2.assign(src, [7, 9])
    same(w, w2)


def test_cpu_tensors_and_argument_errors(gb):
    import torch
    rng = np.random.default_rng(2)
    v = gb.Vector.from_arrays(np.arange(30, dtype=np.uint64), rng.random(30), 30, gb.FP64)
    L = np.array([7, 7, 29, 0], np.int64)
    same(v[torch.from_numpy(L)], v[L.astype(np.uint64)])
    same(v[torch.empty(0, dtype=torch.int64)], v[[]])
    with pytest.raises(TypeError):
        v[torch.from_numpy(L).to(torch.float32)]
    with pytest.raises(ValueError):
        v[torch.arange(20)[::2]]
    with pytest.raises(ValueError):
        v.extract(torch.arange(20).reshape(4, 5))
    with pytest.raises(gb.base.IndexOutOfBound):
        v[torch.tensor([3, -1])]
    A = gb.Matrix.from_arrays(np.array([0], np.uint64), np.array([0], np.uint64), np.array([1.0]), 30, 30, gb.FP64)
    for bad in (lambda: v.__setitem__(torch.from_numpy(L), 2.0), lambda: A.__setitem__((torch.from_numpy(L), torch.from_numpy(L)), 2.0), lambda: v.assign_scalar(2.0, torch.from_numpy(L))):
        with pytest.raises(TypeError, match="scalar assign"):
            bad()
