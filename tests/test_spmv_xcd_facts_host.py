"""The refusals of the read-only view of kernel X's plan (GrBX_Matrix_xcd_plan_facts / GrBX_Matrix_xcd_plan_tiles, grb_spmv.hip) that need no device: the two
entry points in the header, the binding and the library; a null pointer; a matrix that carries no plan (neither call builds one).  What they report for a matrix
that has a plan is what tests/test_spmv_xcd_at_size_gpu.py is built on."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_VALUE, NULL_POINTER = 1, 4
NAMES = ("GrBX_Matrix_xcd_plan_facts", "GrBX_Matrix_xcd_plan_tiles")


def test_symbols_and_header(gb):
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in gb._capi.functions and name not in gb._capi.missing, name
        assert "GrB_Info " + name + "(" in header
    assert gb._capi.constants["GrB_NO_VALUE"] == NO_VALUE and gb._capi.constants["GrB_NULL_POINTER"] == NULL_POINTER


def test_refusals_without_a_plan(gb):
    m = gb.Matrix.from_lists([0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0], 3, 3, gb.FP64)
    out = (C.c_uint64 * 280)(); tiles = (C.c_uint32 * 8)(); bstart = (C.c_uint32 * 8)()
    u64 = C.c_uint64
    facts, per_tile = gb.lib.GrBX_Matrix_xcd_plan_facts, gb.lib.GrBX_Matrix_xcd_plan_tiles
    assert facts(None, 0, out, u64(280)) == NULL_POINTER and facts(m._h, 0, None, u64(280)) == NULL_POINTER
    assert per_tile(None, 0, tiles, u64(4), bstart, u64(8)) == NULL_POINTER and per_tile(m._h, 0, None, u64(4), bstart, u64(8)) == NULL_POINTER
    for transposed in (0, 1):
        assert facts(m._h, transposed, out, u64(280)) == NO_VALUE
        assert per_tile(m._h, transposed, tiles, u64(4), bstart, u64(8)) == NO_VALUE
        assert per_tile(m._h, transposed, tiles, u64(4), None, u64(0)) == NO_VALUE
    assert all(v == 0 for v in out) and all(v == 0 for v in tiles)              # nothing was written
    assert m.nvals == 3                                                          # ... and the matrix is what it was
