"""Kernel X's 8-byte value plane is lane-interleaved inside every tile (pygraphblas_amd/csrc/grb_spmv_tiles.hpp: xt_vpos — two halves of 1 KB, half j holds at
lane * 16 the lane's entries 2 j and 2 j + 1), written by the plan's scattering sweep and read back in entry order by every other reader of the plane (the
narrowing pass of the int16 plane, the scatter of the lane-per-piece layout).  The products of small matrices whose panels end at every place around a tile's
edge, against the oracle:

  edges       eight lines of u carry 14 500, 513, 512, 511, 257, 256, 255 and 1 entries: the line deal gives every line a panel of its own, so the eight streams
              hold exactly these counts (asserted from the plan's facts) — tiles of 1, 255, 256, 257 = 256 + 1, 511, 512, 513 entries' worth
  one_empty   the same without the line of one entry: a panel without a tile
  long_row    seven lines of 2 305 entries each (nine tiles and ONE entry) and 2 048 light columns that the deal gives the eighth panel together: its stream is
              1 900 entries (seven tiles and 108 entries: the last tile is partial) and holds a row of 1 500 entries that begins before and ends behind the
              first chunk boundary (asserted from the plan's tiles per chunk)

FP64 PLUS_TIMES with integer-valued doubles below 2^20 in A and u (every order of summation is exact: the result must be the oracle's BIT FOR BIT), INT64 MIN_PLUS
with weights beyond 16 bits (the 8-byte plane) and with weights 1 ... 255 (the narrow plane must still engage and the plan string say so), FP32 PLUS_SECOND
(4-byte entry words, no value plane: unaffected).  A second FP64 product with rmat.values_torch values at the project's rtol 1e-6 and exact pattern, and the same
under GRB_MI355X_SELL=1 against the tile pipeline's own result to 1e-12 relative.  Kernel X is forced with GRB_MI355X_SPMV=xcd; every product runs twice."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

XP, WP_ENT = 8, 256
EDGE_COUNTS = (513, 512, 511, 257, 256, 255, 1)
BIG = 14500                                        # kernel X takes no matrix of fewer than 16 384 entries
INTERLEAVED, NARROW = "values=lane-interleaved", "values=int16"


@pytest.fixture
def xcd(gpu, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_SPMV", "xcd")


def csr_of(nrows, rows, cols):
    order = np.lexsort((cols, rows)); rows, cols = rows[order], cols[order]
    assert len(np.unique(rows * (1 << 32) + cols)) == len(rows)
    return np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=nrows)))).astype(np.uint32), cols.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(nrows, ncols, rowptr, col, entries per panel in descending order, (first entry, length) of the long row in its stream or None).  Line k of u = columns
    [32 k, 32 k + 16): a 128-byte line of its own for 8-byte AND for 4-byte operands."""
    rng = np.random.default_rng(len(name))
    if name in ("edges", "one_empty"):
        nrows, ncols = 1000, 256
        counts = (BIG,) + (EDGE_COUNTS if name == "edges" else EDGE_COUNTS[:-1])
        rows, cols = [], []
        for k, c in enumerate(counts):             # c distinct (row, column of the line) pairs
            pick = rng.choice(nrows * 16, c, replace=False)
            rows.append(pick // 16); cols.append(32 * k + pick % 16)
        rp, col = csr_of(nrows, np.concatenate(rows), np.concatenate(cols))
        return nrows, ncols, rp, col, tuple(sorted(counts + (0,) * (XP - len(counts)), reverse=True)), None
    assert name == "long_row"
    nh, light0, nlight = 2305, 256, 2048
    lens = [300, 3, 1500, 1, 17, 79]               # the light rows, in row order: 1 900 entries, the third from entry 303 to 1 803
    nrows, ncols = nh + len(lens), light0 + nlight
    light_at = np.sort(rng.choice(nrows, len(lens), replace=False))
    is_light = np.zeros(nrows, bool); is_light[light_at] = True
    rows = [np.repeat(np.flatnonzero(~is_light), 7)]; cols = [(np.arange(7)[None, :] * 32 + rng.integers(0, 16, (nh, 7))).reshape(-1)]
    for r, L in zip(light_at, lens):
        rows.append(np.full(L, r)); cols.append(light0 + rng.choice(nlight, L, replace=False))
    rp, col = csr_of(nrows, np.concatenate(rows), np.concatenate(cols))
    return nrows, ncols, rp, col, tuple(sorted([nh] * 7 + [sum(lens)], reverse=True)), (sum(lens[:2]), lens[2])


def plan_streams(gb, A):
    """(entries, tiles per chunk) of every stream of the matrix's kernel-X plan."""
    out = (C.c_uint64 * 280)()
    rc = gb.lib.GrBX_Matrix_xcd_plan_facts(A._h, 0, out, C.c_uint64(280))
    assert rc == 0, f"no kernel-X plan on the matrix (GrB_Info {rc})"
    assert int(out[4]) == XP                       # NS: one stream per XCD
    per = np.array(out[24: 24 + 4 * XP], np.int64).reshape(XP, 4)
    return per[:, 0], per[:, 3]


def product(gb, typ, sr, name, vals, u):
    """A (+).(x) u twice on pattern `name`; (w's indices, w's values, the plan string).  The plan's streams must hold the entry counts the pattern was built for."""
    nrows, ncols, rp, col, counts, long_row = pattern(name)
    T = getattr(gb, typ)
    A = gb.Matrix.from_csr(T, nrows, ncols, rp, col, np.asarray(vals, T._np))
    x = gb.Vector.from_dense_array(np.asarray(u, T._np), T)
    for _ in range(2): w = A.mxv(x, semiring=getattr(T, sr))
    plan = gb.last_kernel_plan()
    assert "k_spmv_xcd" in plan, plan
    ne, tpc = plan_streams(gb, A)
    assert tuple(sorted(ne.tolist(), reverse=True)) == counts, (ne, counts)
    if long_row:
        k = int(np.flatnonzero(ne == counts[-1])[0]); chunk = int(tpc[k]) * WP_ENT
        assert long_row[0] < chunk < long_row[0] + long_row[1], (long_row, chunk)          # the row crosses the stream's first chunk boundary
        assert all(n % WP_ENT for n in counts)                                              # every stream's last tile is partial
    I, X = w.to_arrays()
    return I, X, plan


def ints(rng, n, lo, hi):
    return rng.integers(lo, hi, n, endpoint=True)


NAMES = ["edges", "one_empty", "long_row"]


@pytest.mark.parametrize("name", NAMES)
def test_fp64_plus_times_is_the_oracles_bits(gb, xcd, name):
    nrows, ncols, rp, col, _, _ = pattern(name)
    rng = np.random.default_rng(11)
    vals = ints(rng, len(col), 1, (1 << 20) - 1).astype(np.float64); u = ints(rng, ncols, 1, (1 << 20) - 1).astype(np.float64)
    I, X, plan = product(gb, "FP64", "PLUS_TIMES", name, vals, u)
    assert INTERLEAVED in plan and NARROW not in plan, plan
    y, pres = O.fast_spmv(rp, col, vals, u)
    assert np.array_equal(I, np.flatnonzero(pres)), plan
    assert np.array_equal(np.asarray(X, np.float64).view(np.uint64), y[pres != 0].view(np.uint64)), plan


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("wide", [True, False])
def test_int64_min_plus_both_value_planes(gb, xcd, name, wide):
    nrows, ncols, rp, col, _, _ = pattern(name)
    rng = np.random.default_rng(12)
    vals = ints(rng, len(col), 1, (1 << 40) if wide else 255).astype(np.int64); u = ints(rng, ncols, 0, 1000).astype(np.int64)
    if wide: vals[:: 97] = ints(rng, len(vals[:: 97]), -(1 << 40), -40000)       # beyond int16 on both sides
    I, X, plan = product(gb, "INT64", "MIN_PLUS", name, vals, u)
    assert (INTERLEAVED in plan) == wide and (NARROW in plan) == (not wide), plan
    rows = np.repeat(np.arange(nrows, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    exp = O.mxv(O.col_vector("INT64", nrows), O.Tuples("INT64", nrows, ncols, rows, col, vals), O.col_vector("INT64", ncols, np.arange(ncols), u), "MIN", "PLUS", "INT64")
    assert np.array_equal(I, exp.I) and np.array_equal(X, exp.X), plan


@pytest.mark.parametrize("name", NAMES)
def test_fp32_plus_second_is_unaffected(gb, xcd, name):
    nrows, ncols, rp, col, _, _ = pattern(name)
    rng = np.random.default_rng(13)
    u = ints(rng, ncols, 1, 1000).astype(np.float32)                               # sums of <= 1 500 terms below 2^24: exact
    I, X, plan = product(gb, "FP32", "PLUS_SECOND", name, np.ones(len(col), np.float32), u)
    assert INTERLEAVED not in plan and NARROW not in plan, plan
    y, pres = O.fast_spmv(rp, col, None, u, semiring="PLUS_SECOND")
    assert np.array_equal(I, np.flatnonzero(pres)) and np.array_equal(np.asarray(X, np.float32).view(np.uint32), y[pres != 0].view(np.uint32)), plan


def rmat_values(name):
    import torch
    from pygraphblas_amd import rmat
    nrows, ncols, rp, col, _, _ = pattern(name)
    dev = torch.device("cuda", 0)
    return rmat.values_torch(len(col), dev, seed=43).cpu().numpy(), rmat.values_torch(ncols, dev, seed=44).cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_fp64_rmat_values_within_1e6(gb, xcd, name):
    nrows, ncols, rp, col, _, _ = pattern(name)
    vals, u = rmat_values(name)
    I, X, plan = product(gb, "FP64", "PLUS_TIMES", name, vals, u)
    assert INTERLEAVED in plan, plan
    y, pres = O.fast_spmv(rp, col, vals, u)
    assert np.array_equal(I, np.flatnonzero(pres)), plan
    assert np.allclose(X, y[pres != 0], rtol=1e-6, atol=0.0), plan


def test_lane_per_piece_layout_reads_the_plane_in_entry_order(gb, xcd, monkeypatch):
    """GRB_MI355X_SELL=1: the plan's lane-per-piece copy is scattered FROM the tile pipeline's value plane; its product must be the tile pipeline's."""
    vals, u = rmat_values("edges")
    It, Xt, plan_t = product(gb, "FP64", "PLUS_TIMES", "edges", vals, u)
    assert "lane-per-piece" not in plan_t, plan_t
    monkeypatch.setenv("GRB_MI355X_SELL", "1")
    Is, Xs, plan_s = product(gb, "FP64", "PLUS_TIMES", "edges", vals, u)
    assert "lane-per-piece" in plan_s, plan_s
    assert np.array_equal(Is, It) and np.allclose(Xs, Xt, rtol=1e-12, atol=0.0), plan_s
