"""GxB_Matrix_concat / GxB_Matrix_split without a device: the integer geometry under the sanitizers (a stand-alone host program,
tests/tile_geometry_check.cpp), the forced host route through the library against the numpy model (tests/tile_model.py), and every error code."""
import contextlib
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tile_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
GRIDS = [([4], [5]), ([2, 3], [4, 1]), ([3], [1, 2, 3]), ([1, 2, 3], [4])]            # 1x1, 2x2, 1x3, 3x1
CASTS = [("FP64", "INT32"), ("INT64", "FP32"), ("INT8", "BOOL"), ("BOOL", "FP64"), ("UINT16", "INT64")]
NULL_POINTER, INVALID_VALUE, DIMENSION_MISMATCH = 4, 5, 8
u64 = C.c_uint64


@contextlib.contextmanager
def host_route():
    old = os.environ.get("GRB_MI355X_TILE")
    os.environ["GRB_MI355X_TILE"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GRB_MI355X_TILE", None)
        else:
            os.environ["GRB_MI355X_TILE"] = old


def test_tile_geometry_under_the_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "tile_geometry_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "tile_geometry_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "tile geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def to_gb(gb, name, M):
    T = getattr(gb, name)
    return gb.Matrix.from_arrays(M.I, M.J, np.ascontiguousarray(M.X, T._np), M.nrows, M.ncols, T)


def from_gb(A):
    I, J, X = A.to_arrays()
    return tm.Mat(A.nrows, A.ncols, I, J, X)


def grid_of(gb, rng, name, rows, cols):
    dt = getattr(gb, name)._np
    return [[tm.random_mat(rng, r, c, 0.5, dt) for c in cols] for r in rows]


@pytest.mark.parametrize("rows,cols", GRIDS)
@pytest.mark.parametrize("name", TYPES)
def test_host_route_every_type(gb, name, rows, cols):
    rng = np.random.default_rng(TYPES.index(name) * 8 + len(rows) * 2 + len(cols))
    dt = getattr(gb, name)._np
    tiles = grid_of(gb, rng, name, rows, cols)
    with host_route():
        got = gb.Matrix.concat([[to_gb(gb, name, t) for t in row] for row in tiles])
        want = tm.concat(tiles, dt)
        assert got.type is getattr(gb, name) and tm.same(from_gb(got), want)
        parts = got.split(rows, cols)
    assert len(parts) == len(rows) and all(len(r) == len(cols) for r in parts)
    for a in range(len(rows)):
        for b in range(len(cols)):
            assert parts[a][b].type is getattr(gb, name) and parts[a][b].shape == (rows[a], cols[b])
            assert tm.same(from_gb(parts[a][b]), tiles[a][b])


@pytest.mark.parametrize("src,dst", CASTS)
def test_host_route_casts(gb, src, dst):
    rng = np.random.default_rng(5)
    rows, cols = [2, 3], [3, 2]
    tiles = grid_of(gb, rng, src, rows, cols)
    mixed = [[to_gb(gb, src if (a + b) % 2 == 0 else dst, tm.Mat(t.nrows, t.ncols, t.I, t.J, tm.cast(t.X, getattr(gb, src if (a + b) % 2 == 0 else dst)._np)))
              for b, t in enumerate(row)] for a, row in enumerate(tiles)]
    with host_route():
        got = gb.Matrix.concat(mixed, typ=getattr(gb, dst))
    want = tm.concat([[tm.Mat(t.nrows, t.ncols, t.I, t.J, tm.cast(t.X, getattr(gb, src if (a + b) % 2 == 0 else dst)._np)) for b, t in enumerate(row)]
                      for a, row in enumerate(tiles)], getattr(gb, dst)._np)
    assert tm.same(from_gb(got), want)


def test_host_route_discards_c_and_repeats_a_tile(gb):
    rng = np.random.default_rng(9)
    t = tm.random_mat(rng, 3, 4, 0.6, np.float64)
    T = to_gb(gb, "FP64", t)
    out = to_gb(gb, "FP64", tm.random_mat(rng, 6, 8, 0.9, np.float64))            # holds entries: they are discarded, not merged
    grid = (C.c_void_p * 4)(T._h.value, T._h.value, T._h.value, T._h.value)
    with host_route():
        assert gb.lib.GxB_Matrix_concat(out._h, grid, u64(2), u64(2), None) == 0
        assert tm.same(from_gb(out), tm.concat([[t, t], [t, t]], np.float64))
        assert tm.same(from_gb(gb.Matrix.hstack([T, T])), tm.concat([[t, t]], np.float64))
        assert tm.same(from_gb(gb.Matrix.vstack([T, T])), tm.concat([[t], [t]], np.float64))
    assert tm.same(from_gb(T), t)


def test_error_codes(gb):
    rng = np.random.default_rng(3)
    A = to_gb(gb, "INT32", tm.random_mat(rng, 5, 7, 0.5, np.int32))
    B = to_gb(gb, "INT32", tm.random_mat(rng, 5, 2, 0.5, np.int32))
    D = to_gb(gb, "INT32", tm.random_mat(rng, 4, 7, 0.5, np.int32))
    lib = gb.lib
    out = gb.Matrix.sparse(gb.INT32, 5, 9)
    grid = (C.c_void_p * 2)(A._h.value, B._h.value)
    with host_route():
        assert lib.GxB_Matrix_concat(out._h, grid, u64(1), u64(2), None) == 0 and out.nvals == A.nvals + B.nvals
        assert lib.GxB_Matrix_concat(None, grid, u64(1), u64(2), None) == NULL_POINTER
        assert lib.GxB_Matrix_concat(out._h, None, u64(1), u64(2), None) == NULL_POINTER
        assert lib.GxB_Matrix_concat(out._h, (C.c_void_p * 2)(A._h.value, None), u64(1), u64(2), None) == NULL_POINTER
        assert lib.GxB_Matrix_concat(out._h, grid, u64(0), u64(2), None) == INVALID_VALUE
        assert lib.GxB_Matrix_concat(out._h, grid, u64(1), u64(0), None) == INVALID_VALUE
        assert lib.GxB_Matrix_concat(out._h, (C.c_void_p * 2)(A._h.value, out._h.value), u64(1), u64(2), None) == INVALID_VALUE      # C among the tiles
        assert lib.GxB_Matrix_concat(out._h, grid, u64(2), u64(1), None) == DIMENSION_MISMATCH                                       # widths 7 and 2 in one column
        assert lib.GxB_Matrix_concat(out._h, (C.c_void_p * 2)(A._h.value, D._h.value), u64(1), u64(2), None) == DIMENSION_MISMATCH   # heights 5 and 4 in one row
        assert lib.GxB_Matrix_concat(gb.Matrix.sparse(gb.INT32, 5, 10)._h, grid, u64(1), u64(2), None) == DIMENSION_MISMATCH         # the sums are not C's shape
        assert out.nvals == A.nvals + B.nvals                                                                                        # a refused call leaves C alone

        sentinel = 0x5A5A5A5A
        tiles = (C.c_void_p * 4)(sentinel, sentinel, sentinel, sentinel)

        def split(m, n, rs, cs, handles=tiles, a=A):
            return lib.GxB_Matrix_split(handles, u64(m), u64(n), (u64 * max(len(rs), 1))(*rs) if rs is not None else None,
                                        (u64 * max(len(cs), 1))(*cs) if cs is not None else None, a._h if a is not None else None, None)

        assert split(2, 2, [2, 3], [3, 4], handles=None) == NULL_POINTER
        assert split(2, 2, None, [3, 4]) == NULL_POINTER and split(2, 2, [2, 3], None) == NULL_POINTER and split(2, 2, [2, 3], [3, 4], a=None) == NULL_POINTER
        assert split(0, 2, [], [3, 4]) == INVALID_VALUE and split(2, 0, [2, 3], []) == INVALID_VALUE
        zero_dim = lib.GrB_Matrix_new(C.byref(C.c_void_p()), C.c_void_p(gb.INT32._h), u64(1 << 61), u64(1))      # the code GrB_Matrix_new gives a dimension it refuses
        assert zero_dim == INVALID_VALUE
        assert split(2, 2, [5, 0], [3, 4]) == zero_dim and split(2, 2, [2, 3], [7, 0]) == zero_dim
        assert split(2, 2, [2, 2], [3, 4]) == DIMENSION_MISMATCH and split(2, 2, [2, 3], [3, 5]) == DIMENSION_MISMATCH
        assert split(2, 2, [(1 << 64) - 1, 6], [3, 4]) == DIMENSION_MISMATCH                                      # a sum that wraps to A's height
        assert [tiles[k] for k in range(4)] == [sentinel] * 4                                                      # Tiles[] untouched by every failed split
        assert split(2, 2, [2, 3], [3, 4]) == 0 and all(tiles[k] not in (None, sentinel) for k in range(4))
        parts = [gb.Matrix(C.c_void_p(tiles[k]), gb.INT32) for k in range(4)]
    assert sum(p.nvals for p in parts) == A.nvals and [p.shape for p in parts] == [(2, 3), (2, 4), (3, 3), (3, 4)]


def test_thresholds_and_geometry_are_exported(gb):
    a, b = u64(0), u64(0)
    assert gb.lib.GrBX_tile_thresholds(C.byref(a), C.byref(b)) == 0 and a.value > 0 and b.value > 0
    out = (u64 * 3)()
    assert gb.lib.GrBX_tile_geometry(out) == 0 and out[0] % (256 * out[2]) == 0 and out[1] >= 1
