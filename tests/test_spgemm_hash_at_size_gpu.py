"""The unmasked (or complement-masked) two-pass hash product `T = A (+).(x) B` (run_spgemm_hash in grb_spgemm_hash.hpp: k_hash_bin5, k_hash_bin, the four symbolic
and three numeric k_spgemm_hash instantiations, k_spgemm_dense, k_spgemm_spa_symbolic / k_spa_split / k_spgemm_spa_numeric, k_table_counts, k_hash_total, the
segmented sort, k_hash_place_rows / k_hash_gather) against the numpy model `product_model.mxm`, at the bin, table, team, grid, column-width and block edges of the
kernels.  Every case sets GRB_MI355X_SPGEMM=hash and its mode's variables, runs `A.mxm(B)`, parses
`spgemm_hash<static|dynamic> symbolic bins a/b/c/d/e numeric bins a/b/c/d[ ranked ...][ ordered]` out of `gb.last_kernel_plan()` and requires the route and ALL
NINE counts to be the ones tests/spgemm_hash_cases.py computed from the operands (a case that went down mxm_few_rows, spmm_full, a batch route or into another
bin fails instead of passing), then compares `to_csr()` with the model bit for bit: row pointers, columns strictly ascending inside a row, values.

The edges are the header's constants, written down once in spgemm_hash_cases.py (`test_the_constants_are_the_headers` reads them back out of the header text).
The four modes and their limits (products for the symbolic bins, entries for the numeric ones; a table holds twice its limit):
  ranked    nothing set, <= 2^20 columns                          128 / 1024                   128 / 1024          the rest: the LDS dense path, ranked rows
  blocks    GRB_MI355X_SPA_RANK=0                                 128 / 1024 / 4096            128 / 1024 / 4096   the rest: the LDS dense path, block by block
  hbm       GRB_MI355X_SPGEMM_NO_SPA=1, or > 2^20 columns         128 / 1024 / 4096 / 16384    128 / 1024 / 4096   the rest: k_spgemm_dense
  ordered   GRB_MI355X_DETERMINISTIC=1, FP PLUS                   128                          128                 the rest: the LDS dense path, ordered walk
(under GRB_MI355X_DETERMINISTIC=1 every other type and the MIN / MAX monoids keep the ranked limits: the plan must say so).
The smallest shapes that reach each edge: (a) 80 rows x 40 000 columns; (b) 70 rows x 0xFFFFFFF0 columns (the progression of 4096 columns with stride 2^20 that
falls into one slot), 2^30 columns for the 32 768-slot table; (d) 4 * 32 * CUs + 1 rows for the first bin, 32 * CUs + 1 for the others, 8192 * 256 + 65 rows for
the binning kernels; (e) the largest dimension the device layout has, 0xFFFFFFF0 = GRB_DIM_DEVICE_MAX (construction accepts it); (f) 2^20 + 1 columns.
Out of reach: a result of >= 2^32 entries (the GrB_INSUFFICIENT_SPACE branch), and the GRB_MI355X_SPA_BITMAP_GB cap at its natural value, a quarter of the
device's memory (`test_bitmap_cap` sets it to almost nothing and sees the plan lose ` ranked`).

Values are `values()` of tests/test_spgemm_masked_at_size_gpu.py: small integers (PLUS and TIMES wrap as C does, the narrow types carry their extremes so that
PLUS wraps), floating point on the 1/8 grid without zeros — every sum is exact in any order (`exact_sums`), no product is -0.0.  TIMES over floating point
rounds, so the monoid without a native atomic is TIMES for the integer types and MAX for the floating-point ones (`product_model.mxm_semirings`).  No
tolerance anywhere."""
import os
import re

import numpy as np
import pytest
import torch

import matrix_model as MM
import product_model as PM
import pygraphblas_amd as gb
import spgemm_hash_cases as HC
from helpers import TYPE
from test_matrix_kernels_at_size_gpu import check, desc_of
from test_spgemm_masked_at_size_gpu import STATIC, exact_sums, mask_values, up, values

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pygraphblas_amd", "csrc")
TYPES = PM.MXM_TYPES
MODE_ENV = {"ranked": {}, "blocks": {"GRB_MI355X_SPA_RANK": "0"}, "hbm": {"GRB_MI355X_SPGEMM_NO_SPA": "1"}, "ordered": {"GRB_MI355X_DETERMINISTIC": "1"}}
ALL_ENV = ("GRB_MI355X_SPA_RANK", "GRB_MI355X_SPGEMM_NO_SPA", "GRB_MI355X_DETERMINISTIC", "GRB_MI355X_SPA_BITMAP_GB", "GRB_MI355X_MXM_ROWS", "GRB_MI355X_BATCH", "GRB_MI355X_FULL")
PLAN = re.compile(r"spgemm_hash<(static|dynamic)> symbolic bins (\d+)/(\d+)/(\d+)/(\d+)/(\d+) numeric bins (\d+)/(\d+)/(\d+)/(\d+)( ranked \(row bitmaps \d+ GB\))?( ordered)? ")


def semirings(typ):
    """`product_model.mxm_semirings` (MAX_FIRST is the dynamic instantiation) and the two that leave one value side unread."""
    return PM.mxm_semirings(typ) + ([] if typ == "BOOL" else ["PLUS_SECOND", "PLUS_FIRST"])


def test_the_constants_are_the_headers():
    src = open(os.path.join(CSRC, "grb_spgemm_hash.hpp")).read()
    assert "big_from = ordered ? 128ull : rank_static ? 1024ull : 4096ull, mid_from = ordered ? 128ull : 1024ull;" in src
    assert "128ull, mid_from, big_from, spa ? big_from : 16384ull, counts" in src and "rownnz.as<uint32_t>(), 128ull, mid_from, big_from, counts" in src
    assert "b = w <= l0 ? 0 : (w <= l1 ? 1 : (w <= l2 ? 2 : (w <= l3 ? 3 : 4)))" in src and "b = w <= l0 ? 0 : (w <= l1 ? 1 : (w <= l2 ? 2 : 3))" in src
    for slots, team, groups in zip(HC.SYM_SLOTS, (64, 256, 512, 1024), HC.SYM_GROUPS):
        assert "k_spgemm_hash<T, SR, %d, %d, %d, false>" % (slots, team, max(team, 256)) in src and team // 16 == groups
    for slots, team, groups in zip(HC.NUM_SLOTS, (64, 256, 1024), HC.NUM_GROUPS):
        assert src.count("k_spgemm_hash<T, SR, %d, %d, %d, true>" % (slots, team, max(team, 256))) == 2 and team // 16 == groups
    assert "nblocks(hs[0], 4)" in src and "nblocks(hn[0], 4)" in src and HC.TEAMS_BIN0 == 4 and "if (b > (uint64_t)ncu * 32) b = (uint64_t)ncu * 32" in src and HC.GRID_CAP_PER_CU == 32
    assert "if (b > 8192) b = 8192" in src and HC.BIN_THREADS == 8192 * 256 and "(uint64_t)ncols <= 32ull * SPA_SYM_WORDS" in src and "SPA_SYM_WORDS = 32768;" in src
    assert "#define SPA_WD8_V %d" % HC.WD[8] in src and "#define SPA_WD4_V %d" % HC.WD[4] in src and HC.SPA_MAX_COLS == 32 * 32768
    assert "std::min<uint64_t>(rows, (uint64_t)ncu * 2)" in src                                          # persistent workgroups of k_spgemm_dense
    assert "return (j * %du >> 7) & mask;" % HC.HASH_MUL in open(os.path.join(CSRC, "grb_spgemm_kernels.hpp")).read()
    assert "#define GRB_DIM_DEVICE_MAX 0xFFFFFFF0ULL" in open(os.path.join(CSRC, "grb_internal.hpp")).read() and HC.DIM_MAX == 0xFFFFFFF0
    assert not any(sr in STATIC.get(t, ()) for t in TYPES for sr in ("MAX_FIRST", "TIMES_PLUS", "MAX_PLUS", "LXOR_LAND"))


# ---- one product ----------------------------------------------------------------------------------------------------------------------------------------------------
def set_mode(monkeypatch, mode, route="hash", **more):
    for name in ALL_ENV: monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("GRB_MI355X_SPGEMM", route)
    for name, v in {**MODE_ENV[mode], **more}.items(): monkeypatch.setenv(name, v)


def operands(case, typ, seed):
    rng = np.random.default_rng(seed)
    return case.A.mat(values(rng, typ, len(case.A.keys))), case.B.mat(values(rng, typ, len(case.B.keys)))


def product(dv, case, A, B, sr, typ, mode, exp=None, route="hash", ranked=None, M=None, struct=False, C=None, accum=None, replace=False, t0=False, t1=False, what=""):
    """One product on the device (`dv`: the uploaded operands, and the mask if there is one — complemented) under the mode the caller has set; the plan must
    name the route, the semiring object, the nine counts of `case.bins` under the limits the call runs with, ` ranked` and ` ordered`.  `exp`: the expected T
    where the caller has it in closed form, else the model computes it."""
    add, mul = sr.split("_"); T = TYPE[typ]
    eff = HC.effective_mode(mode, typ, add, case.B.ncols); bins = case.bins(eff)
    c = gb.Matrix.sparse(T, case.A.nrows, case.B.ncols) if C is None else up(C)
    dv[0].mxm(dv[1], semiring=getattr(T, sr), mask=dv[2] if M is not None else None, out=c, accum=getattr(T, accum) if accum else None,
              desc=desc_of(replace, struct, M is not None, t0, t1))
    plan = gb.last_kernel_plan() + " "; what = f"{what} {typ}.{sr} mode={mode}/{eff} plan={plan}"
    static = "static" if sr in STATIC.get(typ, ()) else "dynamic"
    if route == "esc":
        assert "spgemm_esc<%s>" % static in plan and "spgemm_hash" not in plan, what
    else:
        m = PLAN.search(plan)
        assert m and "spgemm_esc" not in plan, what
        assert m.group(1) == static, what
        assert tuple(int(g) for g in m.groups()[1:10]) == bins, (what, bins)
        assert bool(m.group(11)) == (bins[4] > 0 and eff in ("ranked", "ordered") if ranked is None else ranked) and bool(m.group(12)) == (eff == "ordered"), what
    if exp is None:
        exp = PM.mxm(MM.empty(A.nrows, B.ncols, typ) if C is None else C, A, B, add, mul, typ, mask=M, struct=struct, comp=M is not None, replace=replace, accum=(accum, typ) if accum else None)
    check(c, exp, what)
    return exp


def single_entry_product(A, B, mul, typ):
    """T = A (+).(x) B where every row of A holds at most one entry: T(i,:) = mult(A(i,k), B(k,:)), no fold (spgemm_hash_cases.single_entry_rows)."""
    assert np.all(np.diff(A.rows) > 0)
    brp = np.searchsorted(B.keys, np.arange(B.nrows + 1, dtype=np.int64) * B.ncols); k = A.cols; cnt = brp[k + 1] - brp[k]
    pb = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt - brp[k], cnt)
    return MM.Mat(A.nrows, B.ncols, np.repeat(A.rows, cnt) * np.int64(B.ncols) + B.cols[pb], PM.mult(mul, typ, np.repeat(MM.cast(A.vals, typ), cnt), MM.cast(B.vals, typ)[pb]))


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- (a) the ladder ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", HC.MODES)
@pytest.mark.parametrize("typ", TYPES)
def test_ladder(gpu, monkeypatch, typ, mode):
    """(a) Rows of 0, 1, 127 | 128 | 129, 1023 | 1024 | 1025, 4095 | 4096 | 4097, 16 383 | 16 384 | 16 385 and 20 000 products, each on as many columns (every table at
    exactly half load on its limit) and on 1, 128, 129 (1024, 1025, 4096, 4097) columns (a high symbolic bin, a low numeric one, many combines per slot); a row
    that references empty B rows alone joins no bin.  Every semiring in the ranked and hbm modes, three of them in the other two."""
    case = HC.ladder(); A, B = operands(case, typ, 100 + TYPES.index(typ)); dv = (up(A), up(B))
    assert exact_sums(typ, A)
    set_mode(monkeypatch, mode)
    srs = semirings(typ)
    if mode == "blocks": srs = srs[:1] + srs[3:4] + srs[-1:]                            # PLUS_TIMES, the monoid without a native atomic, PLUS_FIRST (BOOL: both)
    if mode == "ordered": srs = ["PLUS_TIMES", "PLUS_PAIR", "MIN_PLUS", "PLUS_SECOND"] if typ.startswith("FP") else srs[:1]      # (MIN_PLUS: the ranked limits)
    for sr in srs:
        exp = product(dv, case, A, B, sr, typ, mode, what="ladder")
        assert np.array_equal(np.bincount(exp.rows, minlength=A.nrows), case.ent)


# ---- (b) clustered and wrapping keys ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("slots", HC.SYM_SLOTS)
@pytest.mark.parametrize("typ", ["UINT16", "FP32", "INT64"])
def test_clustered_and_wrapping_keys(gpu, monkeypatch, typ, slots):
    """(b) Rows of slots / 2 distinct columns, on the limit of the symbolic table of `slots` slots and (256, 2048, 8192) of the numeric one: keys that hash into
    the last 8 slots (the probing wraps), keys that all hash to one slot (the longest chain there is), a run of consecutive columns.  The columns reach
    0xFFFFFFEF, so the HBM mode is the natural one; the rows of 16 384 entries leave through k_spgemm_dense, 2^30 accumulators wide."""
    case = HC.clustered(slots); A, B = operands(case, typ, 200 + slots); dv = (up(A), up(B))
    set_mode(monkeypatch, "ranked")                                                    # (nothing set: > 2^20 columns)
    for sr in (semirings(typ)[0], semirings(typ)[2]):
        product(dv, case, A, B, sr, typ, "ranked", what=f"clustered {slots}")


# ---- (c) team shapes -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ranked", "blocks", "hbm"])
@pytest.mark.parametrize("typ", ["INT8", "INT32", "FP64"])
def test_team_shapes(gpu, monkeypatch, typ, mode):
    """(c) Rows of exactly 128, 1024, 4096 and 16 384 products reached through one A entry and one long B row, as many A entries as products, NG - 1 / NG / NG + 1 A
    entries for the 4, 16, 32 and 64 groups of the kernels' teams, and B rows of 15, 16, 17, 31, 32, 33 entries."""
    case = HC.teams(); A, B = operands(case, typ, 300 + len(typ)); dv = (up(A), up(B))
    assert exact_sums(typ, A)
    set_mode(monkeypatch, mode)
    for sr in semirings(typ)[:3]:
        product(dv, case, A, B, sr, typ, mode, what="teams")


# ---- (d) dead teams, grid rounds, many rows ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_dead_teams_of_the_first_bin(gpu, monkeypatch, n):
    """(d) The first bin holds 1, 3, 4 and 5 rows: workgroups of four one-wave teams of which three, one, none and three have no row."""
    case = HC.dead_teams(n); set_mode(monkeypatch, "ranked")
    for typ in ("BOOL", "INT32", "FP64"):
        A, B = operands(case, typ, 400 + n); dv = (up(A), up(B))
        for sr in semirings(typ)[:2]:
            exp = product(dv, case, A, B, sr, typ, "ranked", what=f"{n} rows in bin 0")
            assert same(exp, single_entry_product(A, B, sr.split("_")[1], typ))


def same(x, y):
    return np.array_equal(x.keys, y.keys) and x.vals.dtype == y.vals.dtype and np.array_equal(x.vals, y.vals)


@pytest.mark.gpu
@pytest.mark.parametrize("b,mode,typ,sr", [(0, "ranked", "INT8", "PLUS_TIMES"), (0, "hbm", "FP32", "MIN_PLUS"), (1, "ranked", "UINT16", "PLUS_TIMES"), (1, "hbm", "FP64", "PLUS_TIMES"),
                                           (2, "blocks", "INT32", "PLUS_TIMES"), (2, "hbm", "INT8", "MAX_FIRST"), (3, "hbm", "FP32", "PLUS_TIMES")])
def test_one_row_more_than_a_grid_round(gpu, monkeypatch, b, mode, typ, sr):
    """(d) Bin b holds 4 * 32 * CUs + 1 (b = 0) or 32 * CUs + 1 rows of 129, 1025 (blocks and hbm modes) and 4097 (hbm mode) products: the last row is alone in a second round
    of its kernel's grid.  Every A row has a single entry, so the expected row is mult(A(i,k), B(k,:)) in closed form (`single_entry_product`) — expanding 3 * 10^7
    products in the model is too slow, and the fold is not what these cases are about; for the first two bins the model confirms the closed form."""
    case = HC.grid_rounds(b, cus()); A, B = operands(case, typ, 420 + b); dv = (up(A), up(B))
    exp = single_entry_product(A, B, sr.split("_")[1], typ)
    if b < 2: assert same(exp, PM.mxm(MM.empty(A.nrows, B.ncols, typ), A, B, *sr.split("_"), typ))
    set_mode(monkeypatch, mode)
    assert case.bins(mode)[b] == (HC.TEAMS_BIN0 if b == 0 else 1) * HC.GRID_CAP_PER_CU * cus() + 1
    product(dv, case, A, B, sr, typ, mode, exp=exp, what=f"grid round of bin {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,typ,sr", [("ranked", "INT64", "PLUS_TIMES"), ("hbm", "UINT16", "MIN_PLUS"), ("blocks", "FP32", "PLUS_TIMES")])
def test_more_rows_than_a_round_of_the_binning_kernels(gpu, monkeypatch, mode, typ, sr):
    """(d) 8192 * 256 + 65 rows: k_hash_bin5, k_hash_bin, k_table_counts and k_hash_total go round twice, the second round a full wave and one lane — the very
    last row of the matrix.  Twenty-one rows have products, in every bin."""
    case = HC.tall(); A, B = operands(case, typ, 440); dv = (up(A), up(B))
    set_mode(monkeypatch, mode)
    exp = product(dv, case, A, B, sr, typ, mode, exp=single_entry_product(A, B, sr.split("_")[1], typ), what="tall")
    assert exp.rows[-1] == HC.TALL_ROWS - 1


# ---- (e) column width ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ncols", HC.WIDTHS)
def test_column_width_and_the_sorts_end_bit(gpu, monkeypatch, ncols):
    """(e) 1, 2, 3, 2^k and 2^k + 1 (k = 8, 16, 20, 31) and 0xFFFFFFF0 columns — GRB_DIM_DEVICE_MAX itself: construction accepts it.  One row holds columns 0,
    2^m - 1 and 2^m up to the top bit of the largest column, and ncols - 1; every row stays in the first table bin (e = 0 symbolic, d = 0 numeric in the plan:
    no accumulator array of ncols words), so the order of its columns is the segmented sort's alone."""
    case = HC.widths(ncols); set_mode(monkeypatch, "ranked")
    assert case.bins("hbm")[1:5] == (0, 0, 0, 0) and case.bins("hbm")[8] == 0
    for typ, sr in (("INT32", "PLUS_TIMES"), ("FP64", "MIN_PLUS"), ("BOOL", "LOR_LAND")):
        A, B = operands(case, typ, 500); dv = (up(A), up(B))
        exp = product(dv, case, A, B, sr, typ, "ranked", what=f"{ncols} columns")
        assert np.array_equal(exp.cols[exp.rows == case.row], case.special)


# ---- (f) k_spgemm_dense ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("typ", ["BOOL", "UINT16", "FP32", "INT64"])
def test_hbm_accumulators_by_themselves(gpu, monkeypatch, typ):
    """(f) 2^20 + 1 columns, nothing set: three rows beyond every limit go through k_spgemm_dense, with entries in column 2^20 (the one bit of the last bitmap
    word), 31, 32 and ncols - 2."""
    case = HC.dense_natural(); A, B = operands(case, typ, 600); dv = (up(A), up(B))
    set_mode(monkeypatch, "ranked")
    for sr in semirings(typ)[:3]:
        exp = product(dv, case, A, B, sr, typ, "ranked", what="natural hbm")
        assert all(np.isin(case.special, exp.cols[exp.rows == r]).all() for r in case.beyond)


@pytest.mark.gpu
@pytest.mark.parametrize("typ,sr", [("FP32", "MIN_PLUS"), ("FP64", "MAX_PLUS"), ("INT8", "MAX_FIRST"), ("INT32", "MIN_PLUS"), ("INT64", "PLUS_PAIR"), ("UINT16", "PLUS_PAIR")])
def test_hbm_accumulators_are_restored_between_rows(gpu, monkeypatch, typ, sr):
    """(f) 2 * CUs + 3 rows of more than 16 384 products for the 2 * CUs persistent workgroups: three of them walk two rows that share thousands of columns with
    other values.  MIN and MAX over the same patterns: whichever of two rows comes first, an accumulator it left behind wins in one of the two at about half
    the shared columns.  PLUS_PAIR: a bit left behind is a missing entry (the column is never claimed), a count left behind a wrong value."""
    case = HC.dense_persist(cus()); A, B = operands(case, typ, 620); dv = (up(A), up(B))
    set_mode(monkeypatch, "hbm")
    assert case.bins("hbm")[4] == case.bins("hbm")[8] == 2 * cus() + 3
    product(dv, case, A, B, sr, typ, "hbm", what="persistent hbm")


# ---- (g) the LDS dense path at its block edges ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ranked", "blocks"])
@pytest.mark.parametrize("typ", ["BOOL", "INT8", "UINT16", "FP32", "FP64"])
def test_lds_dense_path_at_the_block_edges(gpu, monkeypatch, typ, mode):
    """(g) WD, WD + 1, 2 WD and 2 WD - 1 columns (WD = 16 384 for 8-byte accumulator words, 28 672 for 4-byte ones, which the narrow types use too): rows beyond
    the tables with entries at WD - 1 and WD, B rows that end on a block's last column, rows of which one block holds nothing."""
    wd = HC.WD[8 if MM.NP[typ]().itemsize == 8 else 4]
    set_mode(monkeypatch, mode)
    for ncols in HC.block_widths(wd):
        case = HC.lds_blocks(ncols, wd); A, B = operands(case, typ, 700 + ncols % 7); dv = (up(A), up(B))
        for sr in semirings(typ)[:2]:
            exp = product(dv, case, A, B, sr, typ, mode, what=f"{ncols} columns, blocks of {wd}")
            got = exp.cols[exp.rows == case.mixed[0]]
            assert wd - 1 in got and (ncols == wd or wd in got)


# ---- (h) the write-back on the same T -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["valued", "structural", "accumulate", "replace", "tran0", "tran1"])
def test_ladder_write_back(gpu, monkeypatch, kind):
    """(h) The ladder's T under a complemented valued and structural mask, accumulated into a C with entries, with REPLACE, and with either operand handed over
    transposed: the same route and bins, `product_model.mxm(..., comp=True)`."""
    case = HC.ladder(); typ = "INT64"; A, B = operands(case, typ, 800); rng = np.random.default_rng(801)
    set_mode(monkeypatch, "ranked")
    if kind in ("tran0", "tran1"):
        dv = (up(MM.transpose(A)) if kind == "tran0" else up(A), up(MM.transpose(B)) if kind == "tran1" else up(B))
        product(dv, case, A, B, "PLUS_TIMES", typ, "ranked", t0=kind == "tran0", t1=kind == "tran1", what=kind)
        return
    T = PM.mxm(MM.empty(A.nrows, B.ncols, typ), A, B, "PLUS", "TIMES", typ)
    mk = np.union1d(T.keys[rng.random(T.nvals) < 0.5], rng.integers(0, A.nrows * B.ncols, 3000))
    M = MM.Mat(A.nrows, B.ncols, mk, mask_values(rng, "INT8", len(mk)))
    ck = np.union1d(T.keys[rng.random(T.nvals) < 0.3], rng.integers(0, A.nrows * B.ncols, 3000))
    C = MM.Mat(A.nrows, B.ncols, ck, values(rng, typ, len(ck))) if kind in ("accumulate", "replace") else None
    dv = (up(A), up(B), up(M))
    exp = product(dv, case, A, B, "PLUS_TIMES", typ, "ranked", M=M, struct=kind == "structural", C=C, accum="PLUS" if C is not None else None, replace=kind == "replace", what=kind)
    false_hit = np.isin(M.keys[~MM.mask_truth(M.vals)], exp.keys).any()              # a stored false entry lets T through, unless the mask is structural
    assert 0 < exp.nvals and false_hit == (kind != "structural") and (C is not None or not np.isin(M.keys[MM.mask_truth(M.vals)], exp.keys).any())


# ---- (i) spgemm_esc against the model ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("typ", TYPES)
def test_esc_ladder(gpu, monkeypatch, typ):
    """(i) The expand / sort / compress path, the yardstick of the R-MAT tests of tests/test_mxm_gpu.py, on the ladder against the model."""
    case = HC.ladder(); A, B = operands(case, typ, 900 + TYPES.index(typ)); dv = (up(A), up(B))
    set_mode(monkeypatch, "ranked", route="esc")
    for sr in semirings(typ):
        product(dv, case, A, B, sr, typ, "ranked", route="esc", what="esc ladder")


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", HC.WIDTHS)
def test_esc_column_width(gpu, monkeypatch, ncols):
    """(i) ... and on the widths of (e)."""
    case = HC.widths(ncols); set_mode(monkeypatch, "ranked", route="esc")
    for typ, sr in (("INT32", "PLUS_TIMES"), ("FP64", "MIN_PLUS")):
        A, B = operands(case, typ, 500); dv = (up(A), up(B))
        product(dv, case, A, B, sr, typ, "ranked", route="esc", what=f"esc, {ncols} columns")


# ---- the bitmap cap -------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bitmap_cap(gpu, monkeypatch):
    """With GRB_MI355X_SPA_BITMAP_GB at almost nothing the rows beyond the tables keep the ranked limits and go block by block: the plan loses ` ranked`."""
    case = HC.ladder(); A, B = operands(case, "FP32", 950); dv = (up(A), up(B))
    set_mode(monkeypatch, "ranked", GRB_MI355X_SPA_BITMAP_GB="0.000001")
    assert case.bins("ranked")[4] * ((case.B.ncols + 31) // 32) * 4 > 0.000001 * 2 ** 30
    product(dv, case, A, B, "PLUS_TIMES", "FP32", "ranked", ranked=False, what="bitmap cap")
