"""Kernel X (grb_spmv_xcd.hpp: the plan, k_xp_merge, k_xp_combine; grb_spmv_tiles.hpp: k_spmv_tiles) against a plain numpy row reduction in int64 / float64, at the
edges of its plan.  Every case first reads the plan back (GrBX_Matrix_xcd_plan_facts / _tiles: `facts`) and asserts that the plan has the property the case was
built for, then compares indices, presence and values bit for bit.  Kernel X is forced with GRB_MI355X_SPMV=xcd (the store-mode cases run the dispatcher's own
choice: only then does a product ask the merge to fold the store), every product runs twice before it is compared, and the plan string must name k_spmv_xcd.

The edges are the headers' constants, written once below; `test_the_constants_are_the_facts` compares them with what the entry point reports:
  LDS table          xt_hot<T>::HOT = 19 454 columns per panel for 8-byte types (16-bit column plane: codes >= H escape to the extras stream), 39 931 for 4-byte
                     types (32-bit words); eight panels: a column can be cold only when more than 155 632 / 319 448 columns carry entries;
  tile pipeline      tiles of WP_ENT = 256 entries, four per lane; chunks of >= WP_CHUNK = 4 tiles, a sub-row ends at every chunk boundary; 64 staging slots per
                     wave: more than 64 sub-row ends in a tile take a second round;
  merge              blocks of <= XM_ROWS = 1024 rows and about XM_TARGET = 2048 sub-rows in XM_SLOTS = 2560 LDS slots; a row of more than 510 sub-rows grows
                     m_slots; beyond 64 KiB of slots (8-byte type: a row of more than 6142 sub-rows) m_ok is false and k_xp_combine adds the rows (XP_CONT /
                     XP_HEAD chains), with forced sub-panels after the plan was built again at S = 1;
  narrow values      an INT32 / INT64 / UINT32 / UINT64 matrix whose values all lie in [-32768, 32767] keeps them as int16 (vbytes = 2).
The smallest shapes that reach each edge: (a) 4096 columns: seven 128-byte lines of u heavier than all others together get a panel each and the other lines share
the eighth, whose stream is then the test's rows in order; (b) 2^18 (8-byte) / 2^19 (4-byte) columns; (c) 5000 rows, six of them with entries; one row of
600 000 entries (586 and more sub-rows); one row of (8192 - XM_TARGET + 64) * WP_CHUNK * WP_ENT = 6 356 992 entries (6208 and more sub-rows); (d) 4096 columns,
40 000 entries.
Out of reach: (a) a row of 4097 entries in one panel of a matrix of 4096 columns (a row holds a column once: at most 4096 - 7 lines' worth of them) - it runs at
8192 columns, every column still hot (ncold == 0 is asserted); the exact lane of a start in the seven heavy panels (the deal of columns decides it) - there every
entry is a sub-row of its own, 256 ends per tile, and the positions are placed in the eighth panel; a block boundary between two chosen rows of the empty-row
case (the weights decide) - asserted instead: a block without a sub-row.

Store modes on the two large matrices: every mode runs kernel X (the plan string of each is asserted; the MIN accumulate over an operand with holes reaches it
through the filled holes of grb_mxv.cpp).  On the row of 586 sub-rows m_ok holds, so k_xp_merge takes the accumulate (EPI 1), the pending fill (EPI 2) and the MIN
accumulate (EPI 3) into its store, on LDS grown beyond XM_SLOTS.  On the fallback matrix run_xcd launches k_xp_combine, which stores plainly whatever the call
asked for: the accumulator then runs as the separate write-back (and the sums made of fill values alone are removed by the pass behind it) - same product.

Values: integers for the integer types, floating point on the 1/8 grid without zeros, operands small enough for every sum to be exact in the type: the order of
a sum does not show, so no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import pygraphblas_amd as gb
from helpers import TYPE

pytestmark = pytest.mark.gpu

HOT = {8: 19454, 4: 39931}                                            # xt_hot<T>::HOT
H_SLOTS = {8: 19454, 4: 39932}                                        # xt_hot<T>::H
XP, WP_ENT, WP_CHUNK, XM_ROWS, XM_TARGET, XM_SLOTS, LDS_BYTES = 8, 256, 4, 1024, 2048, 2560, 64 * 1024
MIN_ENTRIES = 16384                                                   # kernel X takes no smaller matrix
FALLBACK_ROW = (LDS_BYTES // 8 - XM_TARGET + 64) * WP_CHUNK * WP_ENT  # 6 356 992
WIDE_ROW = 600000                                                     # >= 8 * 64 * 1024: more than 510 sub-rows
FACT_NAMES = ("H", "HOT", "S", "NP", "NS", "own", "F", "ncold", "vbytes", "has_vals", "m_ok", "m_wide", "m_nblocks", "m_slots", "WP_ENT", "WP_CHUNK", "XM_ROWS",
              "XM_TARGET", "XM_SLOTS", "tsize", "ntiles_all", "c16", "XP_RB", "sell")
PAIRS = [("FP64", "PLUS_TIMES"), ("FP32", "PLUS_SECOND"), ("INT64", "MIN_PLUS"), ("INT32", "PLUS_PAIR"), ("UINT32", "MAX_MIN"), ("INT64", "MAX_PLUS")]
STATIC = {"PLUS_TIMES", "MIN_PLUS", "PLUS_PAIR", "PLUS_SECOND", "PLUS_FIRST"}      # with_semiring, for INT32 / INT64 / FP32 / FP64; MAX_PLUS and all of UINT32 are dynamic
NPT = {t: TYPE[t]._np for t in ("BOOL", "INT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64")}


@pytest.fixture
def xcd(gpu, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_SPMV", "xcd")


# ---- the plan, read back --------------------------------------------------------------------------------------------------------------------------------------
class Facts:
    def __init__(self, A):
        out = (C.c_uint64 * 280)()
        rc = gb.lib.GrBX_Matrix_xcd_plan_facts(A._h, 0, out, C.c_uint64(280))
        assert rc == 0, f"no kernel-X plan on the matrix (GrB_Info {rc})"
        for i, name in enumerate(FACT_NAMES): setattr(self, name, int(out[i]))
        per = np.array(out[24: 24 + 4 * self.NS], np.int64).reshape(self.NS, 4)
        self.ne, self.ntiles, self.nhot, self.tpc = per[:, 0], per[:, 1], per[:, 2], per[:, 3]
        assert int(self.ntiles.sum()) == self.ntiles_all and np.array_equal(self.ntiles, (self.ne + WP_ENT - 1) // WP_ENT)
        tiles = np.zeros((self.ntiles_all, 2), np.uint32); self.bstart = np.zeros(self.m_nblocks + 1 if self.m_ok else 0, np.uint32)
        rc = gb.lib.GrBX_Matrix_xcd_plan_tiles(A._h, 0, tiles.ctypes.data_as(C.c_void_p), C.c_uint64(self.ntiles_all),
                                                 self.bstart.ctypes.data_as(C.c_void_p) if self.m_ok else None, C.c_uint64(len(self.bstart)))
        assert rc == 0, rc
        self.tbase = np.concatenate(([0], np.cumsum(self.ntiles)))
        # sub-rows that END in every tile (what the tile pipeline stages: `nends`) and cold entries of every tile: differences of the two per-tile words
        self.ends = np.diff(np.concatenate((tiles[:, 0].astype(np.int64), [self.F])))
        self.cold = np.diff(np.concatenate((tiles[:, 1].astype(np.int64), [self.ncold])))
        self.first_extra = tiles[:, 1].astype(np.int64)
        assert self.ends.min() >= 0 and self.ends.max() <= WP_ENT and self.cold.min() >= 0 and self.cold.max() <= WP_ENT, "the per-tile words are not monotone"

    def stream(self, k):
        return slice(int(self.tbase[k]), int(self.tbase[k + 1]))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------------
def model(typ, sr, nrows, rp, col, vals, u, upres=None):
    """(values, presence) of t = M (+).(x) u: the products in int64 (uint64 for UINT64, float64 for floating point), every row folded by one ufunc.reduceat, the
    result cast into the type (integers wrap).  `upres`: the operand's presence; a row without a contribution has no entry."""
    add, mul = sr.split("_")
    wide = np.float64 if typ.startswith("FP") else (np.uint64 if typ == "UINT64" else np.int64)
    rp = np.asarray(rp, np.int64); col = np.asarray(col, np.int64)
    a = np.asarray(vals).astype(wide); x = np.asarray(u).astype(wide)[col]
    lens = np.diff(rp)
    if upres is not None:
        keep = np.asarray(upres, bool)[col]
        lens = np.bincount(np.repeat(np.arange(nrows), lens)[keep], minlength=nrows)
        a, x = a[keep], x[keep]
    with np.errstate(over="ignore"):
        z = {"TIMES": lambda: a * x, "SECOND": lambda: x, "FIRST": lambda: a, "PLUS": lambda: a + x, "PAIR": lambda: np.ones(len(a), wide),
             "MIN": lambda: np.minimum(a, x), "MAX": lambda: np.maximum(a, x)}[mul]()
        has = lens > 0; starts = (np.cumsum(lens) - lens)[has]
        y = np.zeros(nrows, NPT[typ])
        if len(z): y[has] = {"PLUS": np.add, "MIN": np.minimum, "MAX": np.maximum}[add].reduceat(z, starts).astype(NPT[typ])
    return y, has


def values(rng, typ, n, lo=1, hi=7):
    if typ.startswith("FP"): return (rng.integers(1, 17, n) * rng.choice([-1, 1], n) / 8.0).astype(NPT[typ])
    return rng.integers(lo, hi, n, endpoint=True).astype(NPT[typ])


def upload(typ, nrows, ncols, rp, col, vals):
    return gb.Matrix.from_csr(TYPE[typ], nrows, ncols, np.asarray(rp, np.uint32), np.asarray(col, np.uint32), np.asarray(vals, NPT[typ]))


def same(got, exp, what):
    (gy, gp), (ey, ep) = got, exp
    assert np.array_equal(gp != 0, ep), f"presence differs: {what}: rows {np.flatnonzero((gp != 0) != ep)[:8]}"
    bad = np.flatnonzero(ep & (gy.view(np.uint8).reshape(len(gy), -1) != ey.view(np.uint8).reshape(len(ey), -1)).any(axis=1))
    assert not len(bad), f"values differ: {what}: rows {bad[:8]}: got {gy[bad[:8]]} expected {ey[bad[:8]]}"


def product(A, typ, sr, u, reps=2, want_xcd=True):
    """A (+).(x) u, `reps` times; the plan string of the last one."""
    T = TYPE[typ]; x = gb.Vector.from_dense_array(np.asarray(u, NPT[typ]), T)
    for _ in range(reps): w = A.mxv(x, semiring=getattr(T, sr))
    plan = gb.last_kernel_plan()
    assert ("k_spmv_xcd" in plan) == want_xcd, plan
    if want_xcd and typ != "BOOL": assert ("k_spmv_xcd<static" in plan) == (sr in STATIC and typ in ("INT32", "INT64", "FP32", "FP64")), plan
    return w.to_dense_arrays(), plan


def check(A, typ, sr, nrows, rp, col, vals, u, what):
    got, plan = product(A, typ, sr, u)
    same(got, model(typ, sr, nrows, rp, col, vals, u), f"{what} {typ}.{sr} {plan}")
    return plan


def operand(rng, typ, sr, ncols, small=True):
    """A dense operand.  `small`: values of 1 ... 15.  Else distinct integers for the 8-byte types (MIN_PLUS: descending in the column index, in steps of 64 - the
    last column of a row decides it), for the 4-byte ones 1 + (40503 j mod 2^14): distinct inside every window of 2^14 columns, and a PLUS_SECOND sum over a
    row of <= 600 entries stays below 2^24."""
    if small: return rng.integers(1, 15, ncols, endpoint=True).astype(NPT[typ])
    j = np.arange(ncols, dtype=np.int64)
    if sr == "MIN_PLUS": return (64 * (ncols - j)).astype(NPT[typ])
    if NPT[typ]().itemsize == 8: return (rng.permutation(ncols) + 1).astype(NPT[typ])
    return (1 + (40503 * j) % 16384).astype(NPT[typ])


def test_the_constants_are_the_facts(xcd):
    rng = np.random.default_rng(1)
    for typ, size in (("INT64", 8), ("INT32", 4)):
        nrows, ncols, L = 80, 3000, 250
        col = np.concatenate([np.sort(rng.choice(ncols, L, replace=False)) for _ in range(nrows)]); rp = np.arange(nrows + 1) * L
        A = upload(typ, nrows, ncols, rp, col, np.ones(len(col)))
        product(A, typ, "PLUS_TIMES", np.ones(ncols))
        f = Facts(A)
        assert (f.H, f.HOT, f.tsize, f.c16) == (H_SLOTS[size], HOT[size], size, int(size == 8))
        assert (f.WP_ENT, f.WP_CHUNK, f.XM_ROWS, f.XM_TARGET, f.XM_SLOTS) == (WP_ENT, WP_CHUNK, XM_ROWS, XM_TARGET, XM_SLOTS)
        assert (f.S, f.NP, f.NS, f.own, f.sell) == (1, XP, XP, 0, 0) and f.m_ok and not f.m_wide and f.m_slots == XM_SLOTS and f.has_vals and f.vbytes == 2
        assert int(f.ne.sum()) == len(col) >= MIN_ENTRIES and f.ncold == 0 and f.tpc.min() >= WP_CHUNK and int(f.ends.sum()) == f.F
        assert f.bstart[0] == 0 and f.bstart[-1] == nrows and np.all(np.diff(f.bstart.astype(np.int64)) > 0)
    assert XP * HOT[8] == 155632 and XP * HOT[4] == 319448 and FALLBACK_ROW == 6356992 and WIDE_ROW >= 8 * 64 * 1024
    assert (XM_TARGET + 510 + XM_TARGET // XM_ROWS) == XM_SLOTS                      # a row of 510 sub-rows still fits XM_SLOTS, 511 do not
    assert (LDS_BYTES // 8 - XM_TARGET - XM_TARGET // XM_ROWS) == 6142               # sub-rows of one row an 8-byte merge block can hold


# ---- (a) positions inside a tile ------------------------------------------------------------------------------------------------------------------------------
CYCLE = list(range(1, 10)) + list(range(251, 262))
CROSSINGS = [257, 511, 512, 1023, 1024, 1025, 4097]
STEPS = (7, 13, 17, 19, 23)                                           # coprime to the number of light columns of every geometry below


@functools.lru_cache(maxsize=None)
def positions(size, ncols, tail):
    """The pattern of case (a).  Lines 0 .. 6 of u (16 / 32 columns each) are `heavy`: nh rows hold one entry in each of them and nothing else, and nh exceeds
    the entries of all other (`light`) columns together - the deal gives every heavy line a panel of its own and all light lines the eighth, whose stream is the
    light rows in row order, whole.  Their lengths place the starts: CYCLE repeated until a start has fallen on every one of the 256 positions of a tile, then
    the CROSSINGS that fit the light columns, each begun on a chunk boundary behind a filler row, then a row that makes the stream k * 256 + tail entries long;
    nh = tail mod 256 as well.  Light and heavy rows alternate at random."""
    rng = np.random.default_rng(size * 1000 + tail)
    lw = 128 // size; light0 = 7 * lw; NL = ncols - light0; CE = WP_CHUNK * WP_ENT
    lens = []
    while len(set((np.cumsum([0] + lens)[:-1] % WP_ENT).tolist())) < WP_ENT or not lens: lens += CYCLE
    pos = sum(lens)
    for L in (c for c in CROSSINGS if c <= NL):
        fill = CE - pos % CE
        lens += [fill, L]; pos += fill + L
    last = (tail - pos) % WP_ENT or WP_ENT
    lens.append(last); pos += last
    assert pos % WP_ENT == tail and max(lens) <= NL
    light_rows = []
    for L in lens:
        s, step = int(rng.integers(0, NL)), int(rng.choice(STEPS))
        light_rows.append(light0 + np.sort((s + np.arange(L, dtype=np.int64) * step) % NL))
    assert all(len(np.unique(r)) == len(r) for r in light_rows[:40]) and np.gcd(NL, int(np.prod(STEPS))) == 1
    nh = (pos // WP_ENT + 40) * WP_ENT + tail                          # > pos, = tail mod 256
    heavy = np.arange(7)[None, :] * lw + rng.integers(0, lw, (nh, 7))
    nrows = nh + len(lens)
    is_light = np.zeros(nrows, bool); is_light[np.sort(rng.choice(nrows, len(lens), replace=False))] = True
    rlen = np.where(is_light, 0, 7); rlen[is_light] = lens
    rp = np.concatenate(([0], np.cumsum(rlen)))
    col = np.zeros(rp[-1], np.int64)
    hstart = rp[:-1][~is_light]
    col[(hstart[:, None] + np.arange(7)[None, :]).reshape(-1)] = heavy.reshape(-1)
    for r, c in zip(np.flatnonzero(is_light), light_rows): col[rp[r]: rp[r + 1]] = c
    # the sub-row ends of the light stream, per tile: a row's end, every chunk boundary, the stream's end
    cuts = np.union1d(np.cumsum(lens), np.arange(CE, pos, CE))
    ends = np.bincount((cuts - 1) // WP_ENT, minlength=(pos + WP_ENT - 1) // WP_ENT)
    starts = np.cumsum([0] + lens)[:-1]
    return nrows, rp, col, np.array(lens), pos, nh, ends, starts


@pytest.mark.parametrize("ncols,tail", [(4096, 1), (8192, 255)])
@pytest.mark.parametrize("typ,sr", PAIRS)
def test_positions_inside_a_tile(xcd, typ, sr, ncols, tail):
    """(a) Every column hot.  From the facts: ncold == 0; seven streams of nh = k * 256 + tail entries in which every entry is a sub-row (256 ends in every full
    tile: four staging rounds); one stream of k' * 256 + tail entries whose ends per tile are exactly those of the light rows' lengths: a start at each of the
    256 (lane, entry) positions, rows of 257 ... 1025 (and 4097) entries begun on a chunk boundary (a row that ends on the last entry of a tile, on the last
    entry of a chunk, tiles without an end: the carry runs through up to three whole tiles), a last tile of 1 or of 255 entries; several merge blocks."""
    size = NPT[typ]().itemsize
    nrows, rp, col, lens, light_total, nh, light_ends, starts = positions(size, ncols, tail)
    rng = np.random.default_rng(len(sr) + size)
    vals = values(rng, typ, len(col), -50 if typ == "INT64" else 1, 50 if typ == "INT64" else 1000 if typ == "UINT32" else 7)
    u = rng.integers(1, 1000, ncols).astype(NPT[typ]) if typ == "UINT32" else operand(rng, typ, sr, ncols)
    A = upload(typ, nrows, ncols, rp, col, vals)
    got, plan = product(A, typ, sr, u)
    f = Facts(A)
    assert f.ncold == 0 and f.m_ok and f.m_nblocks > 1 and (f.has_vals == 1) == (sr.split("_")[1] not in ("SECOND", "PAIR")), plan
    k = np.flatnonzero(f.ne == light_total)
    assert len(k) == 1 and sorted(f.ne.tolist()) == sorted([light_total] + [nh] * 7) and np.all(f.ne % WP_ENT == tail), (f.ne, light_total, nh)
    le = f.ends[f.stream(int(k[0]))]
    assert np.array_equal(le, light_ends), np.flatnonzero(le != light_ends)[:8]
    assert len(set((starts % WP_ENT).tolist())) == WP_ENT and (le == 0).sum() >= 6 and {257, 511, 512, 1023, 1024, 1025} <= set(lens.tolist()) and (4097 in lens) == (ncols == 8192)
    run0 = np.flatnonzero(le == 0); assert np.any(run0[2:] - run0[:-2] == 2)          # three tiles in a row without an end
    for s in range(XP):
        if s != int(k[0]): assert np.all(f.ends[f.stream(s)][:-1] == WP_ENT) and f.ends[f.stream(s)][-1] == tail
    assert f.ends.max() > 64 and f.F == int(f.ends.sum())
    same(got, model(typ, sr, nrows, rp, col, vals, u), f"positions {typ}.{sr} {plan}")


# ---- (b) cold columns -----------------------------------------------------------------------------------------------------------------------------------------
def cold_bounds(f, used, nnz, cmin):
    """Pigeonhole: the eight tables serve at most 8 HOT columns, so at least used - 8 HOT columns are cold, each with >= cmin entries; a table serves the most
    frequent columns of its panel: at least min(used, HOT) columns somewhere, 8 HOT of them when every panel holds that many used columns."""
    lo = max(0, used - XP * f.HOT) * cmin
    hi = nnz - cmin * (XP * f.HOT if used == f.ncols_all and np.all(f.nhot == f.HOT) else min(used, f.HOT))
    return lo, hi


@functools.lru_cache(maxsize=None)
def cold_pattern(size):
    """2^18 / 2^19 columns, all used: 12 HOT `heavy` columns with three entries each, the others (the last ones, and 65 535, 65 536, 131 071) with one.  Rows
    0 .. : `single` rows of 300 to 400 single-entry columns, one after the other (their entries are cold and fill whole tiles of every stream); then rows made of
    heavy columns below `low` alone (a panel's table takes the columns of equal count in index order: these are served by it), 500 each; then mixed rows of 50
    to 600 entries: three shuffles of the heavy columns (the first without those below `low`) and the remaining single-entry columns."""
    rng = np.random.default_rng(size)
    ncols = 1 << (18 if size == 8 else 19); nheavy = 12 * HOT[size]; low = ncols // 3
    special = np.array([65535, 65536, 131071, ncols - 1])
    single = np.union1d(special, np.arange(ncols - (ncols - nheavy - 3), ncols))
    assert len(single) == ncols - nheavy
    heavy = np.setdiff1d(np.arange(ncols), single)
    rows = []
    s = rng.permutation(single); s = np.concatenate((special, np.setdiff1d(s[: 20000], special)))      # the special columns lie in single rows
    at = 0
    while at + 300 <= len(s): L = min(int(rng.integers(300, 401)), len(s) - at); rows.append(np.sort(s[at: at + L])); at += L
    n_single_rows = len(rows)
    rest_single = np.setdiff1d(single, np.concatenate(rows))
    hl = rng.permutation(heavy[heavy < low])
    for at in range(0, len(hl), 500): rows.append(np.sort(hl[at: at + 500]))
    n_low_rows = len(rows) - n_single_rows
    for p in range(3):
        pool = rng.permutation(heavy if p else heavy[heavy >= low])
        if p == 2: pool = rng.permutation(np.concatenate((pool, rest_single)))
        at = 0
        while at < len(pool): L = int(rng.integers(50, 601)); rows.append(np.sort(pool[at: at + L])); at += L
    lens = np.array([len(r) for r in rows]); col = np.concatenate(rows)
    cnt = np.bincount(col, minlength=ncols)
    assert np.all(cnt[heavy] == 3) and np.all(cnt[single] == 1) and all(len(np.unique(r)) == len(r) for r in rows)
    return ncols, np.concatenate(([0], np.cumsum(lens))), col, n_single_rows, n_low_rows


@pytest.mark.parametrize("typ,sr", PAIRS)
def test_cold_columns(xcd, typ, sr):
    """(b) More used columns than the eight tables serve.  From the facts: ncold within the pigeonhole bounds; a tile of 256 cold entries (the single rows: every
    lane with four extras) and a tile with none; tiles whose extras begin at an odd and at an even offset (16-bit plane); cold columns 65 535, 65 536, 131 071
    and ncols - 1."""
    size = NPT[typ]().itemsize
    ncols, rp, col, n_single_rows, n_low_rows = cold_pattern(size)
    nrows = len(rp) - 1; rng = np.random.default_rng(30 + len(sr))
    vals = values(rng, typ, len(col), 1, (1 << 20) if typ == "UINT32" else 7)
    u = operand(rng, typ, sr, ncols, small=False)
    assert np.diff(rp).max() <= 600
    A = upload(typ, nrows, ncols, rp, col, vals)
    got, plan = product(A, typ, sr, u)
    f = Facts(A); f.ncols_all = ncols
    lo, hi = cold_bounds(f, ncols, len(col), 1)
    assert ncols > XP * f.HOT and lo == ncols - XP * HOT[size] and lo <= f.ncold <= hi, (lo, f.ncold, hi, plan)
    assert np.all(f.nhot == f.HOT) and (f.cold == WP_ENT).any() and (f.cold == 0).any() and f.ends.max() > 0
    if f.c16: assert (f.first_extra % 2 == 1).any() and (f.first_extra[1:] % 2 == 0).any() and ((f.first_extra % 2 == 1) & (f.cold > 0)).any()
    same(got, model(typ, sr, nrows, rp, col, vals, u), f"cold columns {typ}.{sr} {plan}")


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("typ,sr", [("FP64", "PLUS_TIMES"), ("INT64", "MIN_PLUS"), ("FP32", "PLUS_SECOND"), ("UINT32", "MAX_MIN")])
def test_cold_columns_at_the_table_boundary(xcd, typ, sr, extra):
    """(b) Exactly 8 HOT used columns (no column need be cold; some are where the deal gave a panel more than HOT of them) and 8 HOT + 8 (at least 8 are), one
    entry each, rows of 200 entries: the HOT | HOT + 1 boundary of a panel's table."""
    size = NPT[typ]().itemsize; ncols = 1 << (18 if size == 8 else 19)
    rng = np.random.default_rng(50 + extra + size)
    used = XP * HOT[size] + extra
    col = rng.permutation(ncols)[:used]
    nrows = (used + 199) // 200; rp = np.minimum(np.arange(nrows + 1) * 200, used)
    col = np.concatenate([np.sort(col[rp[r]: rp[r + 1]]) for r in range(nrows)])
    vals = values(rng, typ, used, 1, (1 << 20) if typ == "UINT32" else 7); u = operand(rng, typ, sr, ncols, small=False)
    A = upload(typ, nrows, ncols, rp, col, vals)
    got, plan = product(A, typ, sr, u)
    f = Facts(A); f.ncols_all = ncols
    lo, hi = cold_bounds(f, used, used, 1)
    assert lo == extra and lo <= f.ncold <= hi and used >= MIN_ENTRIES, (lo, f.ncold, hi)
    print(f"table boundary {typ} used={used}: ncold={f.ncold}")
    same(got, model(typ, sr, nrows, rp, col, vals, u), f"table boundary {typ}.{sr} +{extra} ncold={f.ncold} {plan}")


# ---- (c) the merge --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ,sr", [("FP64", "PLUS_TIMES"), ("INT32", "PLUS_PAIR"), ("UINT32", "MAX_MIN"), ("INT64", "MIN_PLUS")])
def test_runs_of_empty_rows(xcd, typ, sr):
    """(c) 5000 rows, rows 0, 1023, 1024, 2047, 2048 and 4999 alone hold entries (3000 each): merge blocks without a sub-row, presence bytes of 4994 empty rows."""
    rng = np.random.default_rng(60); nrows, ncols, L = 5000, 8192, 3000
    full = [0, 1023, 1024, 2047, 2048, 4999]
    lens = np.zeros(nrows, np.int64); lens[full] = L
    rp = np.concatenate(([0], np.cumsum(lens)))
    col = np.concatenate([np.sort(rng.choice(ncols, L, replace=False)) for _ in full])
    vals = values(rng, typ, len(col)); u = operand(rng, typ, sr, ncols)
    A = upload(typ, nrows, ncols, rp, col, vals)
    got, plan = product(A, typ, sr, u)
    f = Facts(A)
    b = f.bstart.astype(np.int64)
    per_block = np.array([sum(b[i] <= r < b[i + 1] for r in full) for i in range(f.m_nblocks)])
    assert f.m_ok and f.m_nblocks >= 4 and (per_block == 0).any() and np.diff(b).max() <= XM_ROWS and len(col) >= MIN_ENTRIES, (b, plan)
    assert got[1].sum() == len(full)
    same(got, model(typ, sr, nrows, rp, col, vals, u), f"empty rows {typ}.{sr} {plan}")


def big_row_pattern(big, ncols, nshort, short_len, seed):
    """`nshort` short rows (ascending columns in random steps: no two neighbours in one 128-byte line) with one row of `big` entries, all columns distinct, in
    the middle."""
    rng = np.random.default_rng(seed)
    gap_hi = max(18, int(1.8 * ncols / short_len) - 17)
    short = np.cumsum(rng.integers(17, gap_hi, (nshort, short_len)), axis=1)
    short = short[short[:, -1] < ncols]; nshort = len(short)
    bigc = np.sort(rng.permutation(ncols)[:big])
    mid = nshort // 2
    lens = np.full(nshort + 1, short_len, np.int64); lens[mid] = big
    col = np.concatenate((short[:mid].reshape(-1), bigc, short[mid:].reshape(-1)))
    return nshort + 1, np.concatenate(([0], np.cumsum(lens))), col, mid


@functools.lru_cache(maxsize=None)
def wide_pattern():
    return big_row_pattern(WIDE_ROW, 1 << 20, 2010, 1800, 70)


@functools.lru_cache(maxsize=None)
def fallback_pattern():
    return big_row_pattern(FALLBACK_ROW, FALLBACK_ROW + 150000, 600, 100, 71)


def store_modes(A, typ, nrows, ncols, rp, col, vals, rng, what):
    """Every store mode of the merge, by the dispatcher's own choice of kernel (kernel X: the matrix has 2^22 entries and more): plain, accumulate into a full
    vector, accumulate into a pending fill, MIN accumulate of a MIN_PLUS product over an operand with holes into a vector with entries."""
    T = TYPE[typ]; npt = NPT[typ]
    u = rng.integers(1, 15, ncols, endpoint=True).astype(npt)
    x = gb.Vector.from_dense_array(u, T)
    plans = {}
    A.mxv(x, semiring=T.PLUS_TIMES); w = A.mxv(x, semiring=T.PLUS_TIMES); plans["plain"] = gb.last_kernel_plan()
    y, pres = model(typ, "PLUS_TIMES", nrows, rp, col, vals, u)
    same(w.to_dense_arrays(), (y, pres), what + " plain " + plans["plain"])
    w0 = rng.integers(1, 5, nrows).astype(npt); r = gb.Vector.from_dense_array(w0, T)
    A.mxv(x, out=r, accum=T.PLUS, semiring=T.PLUS_TIMES); plans["accum"] = gb.last_kernel_plan()
    same(r.to_dense_arrays(), (np.where(pres, w0 + y, w0).astype(npt), np.ones(nrows, bool)), what + " accum " + plans["accum"])
    r2 = gb.Vector.sparse(T, nrows); r2[:] = 3
    A.mxv(x, out=r2, accum=T.PLUS, semiring=T.PLUS_TIMES); plans["fill"] = gb.last_kernel_plan()
    same(r2.to_dense_arrays(), (np.where(pres, 3 + y, 3).astype(npt), np.ones(nrows, bool)), what + " fill " + plans["fill"])
    up = rng.random(ncols) < 0.34; idx = np.flatnonzero(up).astype(np.uint64)
    xh = gb.Vector.from_arrays(idx, u[up], ncols, T)
    wp = rng.random(nrows) < 0.5; wv = rng.integers(1, 40, nrows).astype(npt)
    v = gb.Vector.from_arrays(np.flatnonzero(wp).astype(np.uint64), wv[wp], nrows, T)
    for sweep in range(2):
        A.mxv(xh, out=v, accum=T.MIN, semiring=T.MIN_PLUS); plans[f"min{sweep}"] = gb.last_kernel_plan()
    t, tp = model(typ, "MIN_PLUS", nrows, rp, col, vals, u, upres=up)
    exp = np.where(wp & tp, np.minimum(wv, t), np.where(tp, t, wv)).astype(npt)
    same(v.to_dense_arrays(), (exp, wp | tp), what + " min " + plans["min1"])
    assert all("k_spmv_xcd" in p for p in plans.values()), plans
    print(what, plans)
    return plans


@pytest.mark.parametrize("typ", ["FP64", "INT32"])
def test_row_of_more_than_510_sub_rows(gpu, monkeypatch, typ):
    """(c) One row of 600 000 entries beside 2000 rows of 1800: m_ok with m_slots > XM_SLOTS (the merge's LDS grows with the row), the whole wave adds the row;
    every store mode on the same plan; then the forced kernel with the type's other semirings."""
    nrows, rp, col, mid = wide_pattern(); ncols = 1 << 20; rng = np.random.default_rng(80)
    assert len(col) >= 1 << 22
    vals = values(rng, typ, len(col))
    A = upload(typ, nrows, ncols, rp, col, vals)
    store_modes(A, typ, nrows, ncols, rp, col, vals, rng, f"wide row {typ}")
    f = Facts(A)
    assert f.m_ok and f.m_slots > XM_SLOTS and f.m_slots * f.tsize <= LDS_BYTES and f.S == 1 and not f.m_wide, (f.m_slots, f.m_ok)
    assert f.m_slots - XM_TARGET - 2 - 255 <= WIDE_ROW // (WP_CHUNK * WP_ENT) + 2 * XP + 255               # (the longest row's sub-rows: about one per chunk and panel)
    monkeypatch.setenv("GRB_MI355X_SPMV", "xcd")
    for sr in (("MIN_PLUS", "MAX_PLUS") if typ == "FP64" else ("PLUS_PAIR", "MAX_MIN")):
        check(A, typ, sr, nrows, rp, col, vals, operand(rng, typ, sr, ncols), "wide row")


@pytest.fixture(scope="module")
def fallback(gpu):
    """The fallback matrices, one per type, built once: {typ: (matrix, values)}."""
    nrows, rp, col, mid = fallback_pattern(); ncols = FALLBACK_ROW + 150000
    out = {}
    for typ in ("INT64", "FP64"):
        vals = values(np.random.default_rng(90 + len(out)), typ, len(col))
        out[typ] = (upload(typ, nrows, ncols, rp, col, vals), vals)
    return out


@pytest.mark.parametrize("typ", ["INT64", "FP64"])
def test_fallback_merge_of_a_row_beyond_the_lds(fallback, typ):
    """(c) One row of 6 356 992 entries: more sub-rows than 64 KiB of merge slots hold, m_ok is false and k_xp_combine adds the rows through the XP_CONT / XP_HEAD
    chains.  Every store mode: the fallback folds none of them, the accumulator runs as the write-back."""
    nrows, rp, col, mid = fallback_pattern(); ncols = FALLBACK_ROW + 150000
    A, vals = fallback[typ]
    assert rp[mid + 1] - rp[mid] == FALLBACK_ROW and 0 < mid < nrows - 1
    store_modes(A, typ, nrows, ncols, rp, col, vals, np.random.default_rng(91), f"fallback {typ}")
    f = Facts(A)
    assert not f.m_ok and f.S == 1 and f.m_slots * f.tsize > LDS_BYTES and f.F > 6142, (f.m_ok, f.m_slots, f.F)


@pytest.mark.parametrize("typ", ["INT64", "FP64"])
def test_forced_sub_panels_start_over_on_the_fallback_row(xcd, monkeypatch, typ):
    """(c) The same pattern under GRB_MI355X_XS=2: the plan with sub-panels cannot merge the row and is built again at S = 1."""
    monkeypatch.setenv("GRB_MI355X_XS", "2")
    nrows, rp, col, mid = fallback_pattern(); ncols = FALLBACK_ROW + 150000; rng = np.random.default_rng(92)
    vals = values(rng, typ, len(col))
    A = upload(typ, nrows, ncols, rp, col, vals)
    sr = "MIN_PLUS" if typ == "INT64" else "PLUS_TIMES"
    u = operand(rng, typ, sr, ncols)
    got, plan = product(A, typ, sr, u)
    f = Facts(A)
    assert f.S == 1 and f.NP == XP and not f.m_ok and "subpanels" not in plan, (f.S, f.m_ok, plan)
    same(got, model(typ, sr, nrows, rp, col, vals, u), f"start over {typ} {plan}")


# ---- (d) the narrow value plane -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_pattern():
    rng = np.random.default_rng(100); nrows, ncols = 400, 4096
    lens = rng.integers(60, 141, nrows)
    col = np.concatenate([np.sort(rng.choice(ncols, int(L), replace=False)) for L in lens])
    return nrows, ncols, np.concatenate(([0], np.cumsum(lens))), col


def narrow_case(typ, sr, vals, want_vbytes, what):
    nrows, ncols, rp, col = narrow_pattern()
    u = np.random.default_rng(101).integers(1, 3, ncols, endpoint=True)
    A = upload(typ, nrows, ncols, rp, col, vals)
    plan = check(A, typ, sr, nrows, rp, col, vals, u, what)
    f = Facts(A)
    assert f.vbytes == want_vbytes and ("values=int16" in plan) == (want_vbytes == 2) and f.has_vals and (f.ne % WP_ENT != 0).any(), (what, f.vbytes, plan)
    return A


@pytest.mark.parametrize("typ", ["INT32", "INT64"])
def test_narrow_value_plane_signed_thresholds(xcd, monkeypatch, typ):
    """(d) [-32768, 32767] with both ends -> int16; one 32768 or one -32769 in the first, the last or a middle stored entry -> the type's own width; the panels' last
    tiles are partial (the zero padding behind them takes part in the range check).  GRB_MI355X_XT_NARROW=0 -> wide, the same bits."""
    nrows, ncols, rp, col = narrow_pattern(); n = len(col); size = NPT[typ]().itemsize
    assert 35000 < n < 45000
    base = values(np.random.default_rng(102), typ, n, -32768, 32767); base[7] = -32768; base[n - 9] = 32767
    for sr in ("PLUS_TIMES", "MIN_PLUS"): narrow_case(typ, sr, base, 2, "both ends")
    for bad in (32768, -32769):
        for at in (0, n - 1, n // 2):
            v = base.copy(); v[at] = bad
            narrow_case(typ, "PLUS_TIMES", v, size, f"{bad} at {at}")
    u = np.random.default_rng(101).integers(1, 3, ncols, endpoint=True)
    monkeypatch.setenv("GRB_MI355X_XT_NARROW", "0")
    A = upload(typ, nrows, ncols, rp, col, base)
    got, plan = product(A, typ, "PLUS_TIMES", u)
    assert Facts(A).vbytes == size and "values=int16" not in plan
    same(got, model(typ, "PLUS_TIMES", nrows, rp, col, base, u), "narrow plane switched off")


@pytest.mark.parametrize("typ", ["UINT32", "UINT64"])
def test_narrow_value_plane_unsigned_thresholds(xcd, typ):
    """(d) Unsigned: all values <= 32767 -> int16; one 32768 -> wide; one 2^32 - 1 / 2^64 - 1 (a negative int16 if truncated) -> wide."""
    nrows, ncols, rp, col = narrow_pattern(); n = len(col); size = NPT[typ]().itemsize
    base = values(np.random.default_rng(103), typ, n, 0, 32767); base[3] = 32767; base[n - 2] = 0
    narrow_case(typ, "PLUS_TIMES", base, 2, "unsigned narrow")
    for bad, at in ((32768, n - 1), (np.iinfo(NPT[typ]).max, 0), (np.iinfo(NPT[typ]).max, n // 2)):
        v = base.copy(); v[at] = bad
        narrow_case(typ, "PLUS_TIMES", v, size, f"{bad} at {at}")


def test_plan_without_values_is_rebuilt_with_them(xcd):
    """(d) PLUS_SECOND first (the plan keeps no values), then PLUS_TIMES on the same matrix object: has_vals flips, the values are narrow."""
    nrows, ncols, rp, col = narrow_pattern(); rng = np.random.default_rng(104)
    vals = values(rng, "INT64", len(col), -300, 300); u = rng.integers(1, 9, ncols)
    A = upload("INT64", nrows, ncols, rp, col, vals)
    check(A, "INT64", "PLUS_SECOND", nrows, rp, col, vals, u, "without values")
    f = Facts(A); assert not f.has_vals and f.vbytes == 8
    check(A, "INT64", "PLUS_TIMES", nrows, rp, col, vals, u, "with values")
    g = Facts(A); assert g.has_vals and g.vbytes == 2 and g.F == f.F and np.array_equal(g.ends, f.ends)


# ---- (e) types that must not reach kernel X -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ,sr", [("INT16", "PLUS_TIMES"), ("BOOL", "LOR_LAND")])
def test_small_types_do_not_reach_kernel_x(xcd, typ, sr):
    nrows, ncols, rp, col = narrow_pattern(); rng = np.random.default_rng(105)
    if typ == "BOOL": vals = rng.random(len(col)) < 0.5; u = rng.random(ncols) < 0.1
    else: vals = values(rng, typ, len(col), -9, 9); u = rng.integers(-3, 4, ncols)
    A = upload(typ, nrows, ncols, rp, col, vals)
    got, plan = product(A, typ, sr, u, want_xcd=False)
    out = (C.c_uint64 * 280)()
    assert gb.lib.GrBX_Matrix_xcd_plan_facts(A._h, 0, out, C.c_uint64(280)) == 1, plan                     # GrB_NO_VALUE: no plan was built
    exp = model("INT64", "MAX_MIN" if typ == "BOOL" else sr, nrows, rp, col, vals, u)
    same((got[0].astype(np.int64), got[1]), ((exp[0].astype(NPT[typ])).astype(np.int64), exp[1]), f"{typ} {plan}")


# ---- (f) reproducibility --------------------------------------------------------------------------------------------------------------------------------------
def test_cold_gathers_are_reproducible(xcd):
    """(f) Unstructured FP64 values on the cold-column pattern: three products agree bit for bit (they are not compared with the model: the sums round)."""
    ncols, rp, col, _, _ = cold_pattern(8); rng = np.random.default_rng(110)
    A = upload("FP64", len(rp) - 1, ncols, rp, col, rng.random(len(col)))
    u = rng.random(ncols)
    (ref, pres), plan = product(A, "FP64", "PLUS_TIMES", u)
    assert Facts(A).ncold > 0
    for _ in range(2):
        (y, p), _ = product(A, "FP64", "PLUS_TIMES", u, reps=1)
        assert y.tobytes() == ref.tobytes() and p.tobytes() == pres.tobytes(), plan


def test_fallback_merge_is_reproducible(xcd):
    """(f) The same on the fallback pattern: k_xp_combine adds the chains in a fixed order."""
    nrows, rp, col, mid = fallback_pattern(); ncols = FALLBACK_ROW + 150000; rng = np.random.default_rng(111)
    A = upload("FP64", nrows, ncols, rp, col, rng.random(len(col)))
    u = rng.random(ncols)
    (ref, pres), plan = product(A, "FP64", "PLUS_TIMES", u)
    assert not Facts(A).m_ok
    for _ in range(2):
        (y, p), _ = product(A, "FP64", "PLUS_TIMES", u, reps=1)
        assert y.tobytes() == ref.tobytes() and p.tobytes() == pres.tobytes(), plan
