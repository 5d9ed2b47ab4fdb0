"""GxB_Matrix_concat / GxB_Matrix_split on the device (grb_tile.hip) and on the forced host route, both against the numpy model of tests/tile_model.py, bit for bit.

Both operations move and cast values and sum nothing, so every comparison is exact equality of rowptr, col and the values' bytes.  The references are the model
and, for one case each, the existing operations (a chain of ranged assign_matrix calls, a ranged extract_matrix); the device route is never a reference.
The chunk size and the grid cap of the two fill kernels come from the library (GrBX_tile_geometry)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import tile_model as tm

pytestmark = pytest.mark.gpu

NULL_POINTER, INVALID_VALUE, DIMENSION_MISMATCH = 4, 5, 8
u64 = C.c_uint64
HOOKS = ["0", "1"]


@contextlib.contextmanager
def hook(value):
    old = os.environ.get("GRB_MI355X_TILE")
    os.environ["GRB_MI355X_TILE"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GRB_MI355X_TILE", None)
        else:
            os.environ["GRB_MI355X_TILE"] = old


def residency(gb, A):
    w = C.c_int(-1)
    assert gb.lib.GrBX_Matrix_residency(A._h, C.byref(w)) == 0
    return w.value


def geometry(gb):
    out = (u64 * 3)()
    assert gb.lib.GrBX_tile_geometry(out) == 0
    return int(out[0]), int(out[1])


def hbm(gb, name, M):
    """Imported straight into HBM: no host mirror."""
    T = getattr(gb, name)
    rp, col, val = tm.csr(M)
    A = gb.Matrix.from_csr(T, M.nrows, M.ncols, rp.astype(np.uint32), col.astype(np.uint32), np.ascontiguousarray(val, T._np))
    assert residency(gb, A) == 2
    return A


def read(A):
    """(rowptr, col, values) of the library's own CSR image."""
    try:
        rp, ci, x = A.to_csr_tensors()
        return rp.cpu().numpy().view(np.uint32).astype(np.int64), ci.cpu().numpy().view(np.uint32).astype(np.int64), x.cpu().numpy()
    except TypeError:                                                       # a type the installed torch has no dtype for
        I, J, X = A.to_arrays()
        return tm.csr(tm.Mat(A.nrows, A.ncols, I, J, X))


def check(A, want, what=""):
    rp, col, val = read(A)
    wrp, wcol, wval = tm.csr(want)
    assert A.shape == (want.nrows, want.ncols), what
    assert np.array_equal(rp, wrp), what + ": rowptr"
    assert np.array_equal(col, wcol), what + ": col"
    assert val.dtype == wval.dtype and val.tobytes() == np.ascontiguousarray(wval).tobytes(), what + ": values"
    for r in np.nonzero(np.diff(rp) > 1)[0][:50]:
        assert np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0), what + ": columns strictly increasing"
    if len(col) > 1:                                                        # ... in EVERY row: a decrease may stand only where a row begins
        dec = np.nonzero(np.diff(col) <= 0)[0] + 1
        assert np.all(np.isin(dec, rp)), what + ": columns strictly increasing"


def both_routes(gb, name, cname, tiles, hooks=HOOKS):
    """concat the model grid `tiles` (type `name`) into type `cname` and split it again, under each hook value, against the model."""
    rows, cols = [row[0].nrows for row in tiles], [t.ncols for t in tiles[0]]
    cdt = getattr(gb, cname)._np
    want = tm.concat(tiles, cdt)
    want_parts = tm.split(want, rows, cols)
    for h in hooks:
        with hook(h):
            ops = [[hbm(gb, name, t) for t in row] for row in tiles]
            got = gb.Matrix.concat(ops, typ=getattr(gb, cname))
            if h == "1":
                assert residency(gb, got) == 2 and all(residency(gb, t) == 2 for row in ops for t in row), "concat: operands and result stay in HBM only"
                assert want.nrows == 0 or "k_concat_fill" in gb.last_kernel_plan()
            check(got, want, f"concat hook={h}")
            if 0 in rows or 0 in cols:
                continue
            src = hbm(gb, cname, want)
            parts = src.split(rows, cols)
            if h == "1":
                assert "k_split_scatter" in gb.last_kernel_plan() and residency(gb, src) == 2
                assert all(residency(gb, p) == 2 for row in parts for p in row), "split: the tiles live in HBM only"
            for a in range(len(rows)):
                for b in range(len(cols)):
                    assert parts[a][b].type is getattr(gb, cname)
                    check(parts[a][b], want_parts[a][b], f"split hook={h} tile ({a}, {b})")
            check(src, want, "split only reads A")


def rand_grid(rng, rows, cols, dtype, density=0.3):
    return [[tm.random_mat(rng, r, c, density, dtype) for c in cols] for r in rows]


GRIDS = {
    "1x1": ([300], [70]),
    "2x2": ([130, 129], [33, 64]),
    "1xn": ([257], [5, 1, 64, 3]),
    "mx1": ([5, 1, 300, 3], [65]),
    "3x5 unequal": ([1, 40, 7], [9, 1, 31, 2, 17]),
    "n=9": ([70], [3, 1, 4, 1, 5, 9, 2, 6, 5]),
    "n=65": ([37], [1 + (k * 7) % 3 for k in range(65)]),
    "64x3": ([1 + (k * 5) % 4 for k in range(64)], [6, 1, 30]),
}


@pytest.mark.parametrize("grid", list(GRIDS))
def test_grids(gb, gpu, grid):
    rows, cols = GRIDS[grid]
    both_routes(gb, "FP64", "FP64", rand_grid(np.random.default_rng(len(rows) * 100 + len(cols)), rows, cols, np.float64))


def test_content_edges(gb, gpu):
    rng = np.random.default_rng(11)
    rows, cols = [6, 5, 4], [7, 3, 8]
    empty = lambda r, c: tm.make(r, c, [], [], np.zeros(0, np.float32))
    both_routes(gb, "FP32", "FP32", [[empty(r, c) for c in cols] for r in rows])                                   # an all-empty operand
    g = rand_grid(rng, rows, cols, np.float32, 0.6)
    g[1][1] = empty(5, 3)                                                                                          # an empty tile
    both_routes(gb, "FP32", "FP32", g)
    g = rand_grid(rng, rows, cols, np.float32, 0.6)
    g[1] = [empty(5, c) for c in cols]                                                                             # a whole empty tile-row
    both_routes(gb, "FP32", "FP32", g)
    g = rand_grid(rng, rows, cols, np.float32, 0.6)                                                                # empty rows on both sides of a tile border
    for b in range(3):
        keep = g[0][b].I != 5
        g[0][b] = tm.Mat(6, cols[b], g[0][b].I[keep], g[0][b].J[keep], g[0][b].X[keep])
        keep = g[1][b].I != 0
        g[1][b] = tm.Mat(5, cols[b], g[1][b].I[keep], g[1][b].J[keep], g[1][b].X[keep])
    both_routes(gb, "FP32", "FP32", g)
    # rows that lie entirely in one column block, and entries planted at the last column of block b and the first of b + 1 for every b
    cols = [4, 1, 6, 2, 5]
    g = [[empty(8, c) for c in cols]]
    for b, c in enumerate(cols):
        I = [b, b, 5, 5, 6] if c > 1 else [b, 5, 6]
        J = [0, c - 1, 0, c - 1, c - 1] if c > 1 else [0, 0, 0]
        I, J = np.array(I), np.array(J)
        if b == len(cols) - 1:
            I, J = I[:-1], J[:-1]
        if b == 0:
            I, J = np.append(I, 7), np.append(J, 1)                                                                # row 7 lies in block 0 alone
        key = np.unique(I * 100 + J)
        g[0][b] = tm.make(8, c, key // 100, key % 100, (np.arange(len(key)) + 10 * b + 1).astype(np.float32))
    both_routes(gb, "FP32", "FP32", g)


def test_work_distribution_edges(gb, gpu):
    chunk, cap = geometry(gb)
    ncols = 3 * chunk + 40
    lens = [chunk - 1, 0, chunk, chunk + 1, 0, 0, 2 * chunk + 77, 1, 5]                  # rows of chunk - 1, chunk, chunk + 1 entries; one spanning several chunks
    I = np.concatenate([np.full(n, r) for r, n in enumerate(lens)])
    J = np.concatenate([np.arange(n) + (17 if n > 2 * chunk else 0) for n in lens])      # every long row crosses the column boundaries below
    A = tm.make(len(lens), ncols, I, J, (np.arange(len(I)) % 251).astype(np.int16))
    rows, cols = [4, 5], [chunk - 3, 7, ncols - chunk - 4]
    both_routes(gb, "INT16", "INT16", tm.split(A, rows, cols))


def test_more_chunks_than_one_grid_round(gb, gpu):
    chunk, cap = geometry(gb)
    per_row, ncols = 1500, 3000
    nrows = (chunk * cap) // per_row + 40                                                # chunk * cap entries is one grid round
    I = np.repeat(np.arange(nrows), per_row)
    J = np.tile(np.arange(per_row) * 2, nrows)
    A = tm.Mat(nrows, ncols, I.astype(np.uint64), J.astype(np.uint64), ((I + J) % 2).astype(np.bool_))
    assert len(I) > chunk * cap
    rows, cols = [nrows - 1000, 1000], [1001, ncols - 1001]
    both_routes(gb, "BOOL", "BOOL", tm.split(A, rows, cols), hooks=["1"])                # (the host route is covered at every smaller size)


WIDTHS = [("BOOL", "BOOL"), ("INT16", "INT16"), ("FP32", "FP32"), ("FP64", "FP64"), ("UINT64", "UINT64"),
          ("FP64", "INT32"), ("INT64", "FP32"), ("INT8", "BOOL"), ("BOOL", "FP64")]


@pytest.mark.parametrize("name,cname", WIDTHS)
def test_widths_and_casts(gb, gpu, name, cname):
    rng = np.random.default_rng(WIDTHS.index((name, cname)))
    rows, cols = [70, 1, 200], [31, 64, 5]
    dt = getattr(gb, name)._np
    g = rand_grid(rng, rows, cols, dt)
    if name == "UINT64":                                                                 # values above 2^53: no detour through a double survives
        g = [[tm.Mat(t.nrows, t.ncols, t.I, t.J, (t.X + np.uint64((1 << 63) + 1))) for t in row] for row in g]
    if name == "FP64":                                                                   # fractions; FP64 -> INT32 truncates toward zero, far inside the range
        g = [[tm.Mat(t.nrows, t.ncols, t.I, t.J, t.X * 1000.37) for t in row] for row in g]
    if name == "INT64":                                                                  # FP32 rounds them: round-to-nearest-even in numpy and on the device
        g = [[tm.Mat(t.nrows, t.ncols, t.I, t.J, t.X * np.int64((1 << 33) + 12345)) for t in row] for row in g]
    both_routes(gb, name, cname, g)


def test_mixed_tile_types_cast_once_each(gb, gpu):
    rng = np.random.default_rng(21)
    a, b = tm.random_mat(rng, 40, 30, 0.4, np.float64), tm.random_mat(rng, 40, 20, 0.4, np.int32)
    want = tm.concat([[a, b, a]], np.float32)
    for h in HOOKS:
        with hook(h):
            A, B = hbm(gb, "FP64", a), hbm(gb, "INT32", b)
            got = gb.Matrix.concat([[A, B, A]], typ=gb.FP32)                             # the same tile object at two grid positions
            if h == "1":
                assert "cast=2" in gb.last_kernel_plan()
            check(got, want, f"hook={h}")
            check(A, a, "a tile is only read")


@pytest.mark.parametrize("h", HOOKS)
def test_round_trips(gb, gpu, h):
    rng = np.random.default_rng(5)
    a = tm.random_mat(rng, 500, 400, 0.05, np.float64)
    rows, cols = [100, 1, 399], [64, 65, 1, 270]
    with hook(h):
        A = hbm(gb, "FP64", a)
        parts = A.split(rows, cols)
        back = gb.Matrix.concat(parts)
        check(back, a, "concat(split(A)) is A")
        again = back.split(rows, cols)
        want = tm.split(a, rows, cols)
        for x in range(3):
            for y in range(4):
                check(again[x][y], want[x][y], "split(concat(tiles)) gives the tiles back")


def test_existing_operations_agree(gb, gpu):
    rng = np.random.default_rng(8)
    rows, cols = [300, 200], [150, 250, 100]
    g = rand_grid(rng, rows, cols, np.float64, 0.05)
    rb, cb = tm.bounds(rows), tm.bounds(cols)
    with hook("1"):
        ops = [[hbm(gb, "FP64", t) for t in row] for row in g]
        got = gb.Matrix.concat(ops)
        chain = gb.Matrix.sparse(gb.FP64, sum(rows), sum(cols))
        for a in range(2):
            for b in range(3):
                chain.assign_matrix(ops[a][b], slice(int(rb[a]), int(rb[a + 1]) - 1), slice(int(cb[b]), int(cb[b + 1]) - 1))
        for x, y in zip(read(got), read(chain)):
            assert x.tobytes() == y.tobytes()
        tile = got.split(rows, cols)[1][1]
        ext = got.extract_matrix(slice(int(rb[1]), int(rb[2]) - 1), slice(int(cb[1]), int(cb[2]) - 1))
        for x, y in zip(read(tile), read(ext)):
            assert x.tobytes() == y.tobytes()


def test_reuse_of_c_with_cached_plans(gb, gpu):
    rng = np.random.default_rng(13)
    n = 600
    old = tm.random_mat(rng, n, n, 0.05, np.float64)
    g = rand_grid(rng, [250, 350], [400, 200], np.float64, 0.04)
    want = tm.concat(g, np.float64)
    u = rng.integers(1, 9, n).astype(np.float64)
    V, P = tm.to_dense(want)
    with hook("1"):
        Cm = hbm(gb, "FP64", old)
        v = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), u, n, gb.FP64)
        Cm.mxv(v, semiring=gb.FP64.PLUS_TIMES)                                           # the plans of the old image are cached now
        ops = [[hbm(gb, "FP64", t) for t in row] for row in g]
        assert gb.lib.GxB_Matrix_concat(Cm._h, (C.c_void_p * 4)(*[t._h.value for row in ops for t in row]), u64(2), u64(2), None) == 0
        check(Cm, want, "C's old entries are discarded")
        wi, wx = Cm.mxv(v, semiring=gb.FP64.PLUS_TIMES).to_arrays()
    rows_with = np.nonzero(P.any(axis=1))[0]
    assert np.array_equal(wi.astype(np.int64), rows_with)
    assert np.array_equal(wx, (V @ u)[rows_with])                                        # small integers: every sum is exact


def test_error_codes_on_the_device_route(gb, gpu):
    rng = np.random.default_rng(3)
    a, b, d = tm.random_mat(rng, 5, 7, 0.5, np.int32), tm.random_mat(rng, 5, 2, 0.5, np.int32), tm.random_mat(rng, 4, 7, 0.5, np.int32)
    lib = gb.lib
    with hook("1"):
        A, B, D = hbm(gb, "INT32", a), hbm(gb, "INT32", b), hbm(gb, "INT32", d)
        out = gb.Matrix.sparse(gb.INT32, 5, 9)
        grid = (C.c_void_p * 2)(A._h.value, B._h.value)
        assert lib.GxB_Matrix_concat(out._h, grid, u64(1), u64(2), None) == 0
        check(out, tm.concat([[a, b]], np.int32))
        assert lib.GxB_Matrix_concat(out._h, None, u64(1), u64(2), None) == NULL_POINTER
        assert lib.GxB_Matrix_concat(out._h, (C.c_void_p * 2)(A._h.value, None), u64(1), u64(2), None) == NULL_POINTER
        assert lib.GxB_Matrix_concat(out._h, grid, u64(0), u64(2), None) == INVALID_VALUE and lib.GxB_Matrix_concat(out._h, grid, u64(1), u64(0), None) == INVALID_VALUE
        assert lib.GxB_Matrix_concat(out._h, (C.c_void_p * 2)(A._h.value, out._h.value), u64(1), u64(2), None) == INVALID_VALUE
        assert lib.GxB_Matrix_concat(out._h, grid, u64(2), u64(1), None) == DIMENSION_MISMATCH
        assert lib.GxB_Matrix_concat(out._h, (C.c_void_p * 2)(A._h.value, D._h.value), u64(1), u64(2), None) == DIMENSION_MISMATCH
        assert lib.GxB_Matrix_concat(gb.Matrix.sparse(gb.INT32, 5, 10)._h, grid, u64(1), u64(2), None) == DIMENSION_MISMATCH
        check(out, tm.concat([[a, b]], np.int32), "a refused call leaves C alone")
        sentinel = 0x5A5A5A5A
        tiles = (C.c_void_p * 4)(sentinel, sentinel, sentinel, sentinel)
        split = lambda rs, cs, m=2, n=2: lib.GxB_Matrix_split(tiles, u64(m), u64(n), (u64 * 2)(*rs), (u64 * 2)(*cs), A._h, None)
        assert split([2, 3], [3, 4], m=0) == INVALID_VALUE and split([2, 3], [3, 4], n=0) == INVALID_VALUE
        assert split([5, 0], [3, 4]) == INVALID_VALUE and split([2, 3], [7, 0]) == INVALID_VALUE
        assert split([2, 2], [3, 4]) == DIMENSION_MISMATCH and split([2, 3], [3, 5]) == DIMENSION_MISMATCH
        assert lib.GxB_Matrix_split(tiles, u64(2), u64(2), None, (u64 * 2)(3, 4), A._h, None) == NULL_POINTER
        assert [tiles[k] for k in range(4)] == [sentinel] * 4
        assert split([2, 3], [3, 4]) == 0
        parts = [gb.Matrix(C.c_void_p(tiles[k]), gb.INT32) for k in range(4)]
        want = tm.split(a, [2, 3], [3, 4])
        for k in range(4):
            check(parts[k], want[k // 2][k % 2])
