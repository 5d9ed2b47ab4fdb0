"""tests/tile_model.py against numpy itself: concat is np.block of the tiles' dense value and presence arrays, split is slicing them."""
import numpy as np
import pytest

import tile_model as tm

GRIDS = [([3], [4]), ([2, 3], [4, 1]), ([5], [1, 2, 3]), ([1, 2, 3], [5]), ([1, 4, 2], [3, 1, 5, 2, 4])]


@pytest.mark.parametrize("rows,cols", GRIDS)
@pytest.mark.parametrize("dtype", [np.float64, np.int16, np.bool_])
def test_concat_is_np_block(rows, cols, dtype):
    rng = np.random.default_rng(len(rows) * 16 + len(cols))
    tiles = [[tm.random_mat(rng, r, c, 0.4, np.int32) for c in cols] for r in rows]
    got = tm.concat(tiles, dtype)
    dense = [[tm.to_dense(t) for t in row] for row in tiles]
    V = np.block([[tm.cast(d[0], dtype) for d in row] for row in dense])
    P = np.block([[d[1] for d in row] for row in dense])
    assert tm.same(got, tm.from_dense(V, P))
    assert got.X.dtype == np.dtype(dtype) and got.nrows == sum(rows) and got.ncols == sum(cols)


@pytest.mark.parametrize("rows,cols", GRIDS)
def test_split_is_slicing(rows, cols):
    rng = np.random.default_rng(7)
    A = tm.random_mat(rng, sum(rows), sum(cols), 0.5, np.float32)
    V, P = tm.to_dense(A)
    rb, cb = tm.bounds(rows), tm.bounds(cols)
    tiles = tm.split(A, rows, cols)
    for a in range(len(rows)):
        for b in range(len(cols)):
            assert tm.same(tiles[a][b], tm.from_dense(V[rb[a]:rb[a + 1], cb[b]:cb[b + 1]], P[rb[a]:rb[a + 1], cb[b]:cb[b + 1]]))
    assert tm.same(tm.concat(tiles, np.float32), A)


def test_explicit_zeros_are_entries_and_casts_are_c_casts():
    A = tm.make(2, 3, [0, 1, 1], [2, 0, 2], np.array([0.0, -2.75, 3.5]))
    assert len(tm.split(A, [1, 1], [2, 1])[0][1].X) == 1                       # the stored 0.0 is an entry of tile (0, 1)
    got = tm.concat([[A]], np.int32)
    assert got.X.tolist() == [0, -2, 3]                                       # truncation toward zero
    assert tm.concat([[A]], np.bool_).X.tolist() == [False, True, True]
    rp, col, val = tm.csr(A)
    assert rp.tolist() == [0, 1, 3] and col.tolist() == [2, 0, 2]
