"""The masked Gustavson product `T<M> = A (+).(x) B` (run_spgemm_masked in grb_spgemm_kernels.hpp: k_bin_rows, the four k_spgemm_masked_lds instantiations,
k_spgemm_masked_map, k_fill_words, k_flags_to_u32, k_rowptr_from_scan, k_scatter_acc) against the numpy model `product_model.masked_mxm` / `mxm`, at the bin,
table, list and slice edges of the kernels.  Every case compares `to_csr()` of the result with the model bit for bit (row pointers, columns strictly ascending
inside a row, values), and parses `bins a/b/c/d/e` out of `gb.last_kernel_plan()`: the route (`k_spgemm_masked<static|dynamic>`) and the five bin counts must
be the ones the case was built for, so a case that went down another route, or whose rows moved to another bin, fails instead of passing.

The edges are the header's constants, written down once below (`test_the_constants_are_the_headers` reads the defaults back out of the header): a later change
of a constant shows up there and as a plan assertion failing, not as a case that quietly stops reaching its edge.
  k_bin_rows                 mask-row length (every stored entry, false ones too) <= 32 / <= 256 / <= 1024 / <= 4096 / more; a row with an empty mask row or
                             an empty A row goes into no bin;
  k_spgemm_masked_lds        tables of KS = 128 / 1024 / 2048 / 8192 keys for at most 32 / 256 / 1024 / 4096 mask entries; work lists of LCAP = 64 / SPG_LIST /
                             SPG_LIST / SPG_LIST_BIG_V entries of A(i,:) per round; B rows of < SPG_LONG_V = 64 entries by 16-lane groups, longer ones by a wave,
                             from 256 entries on (always, when the multiply reads no value) through the filter and the survivor queue (SPG_QCAP = 128, flushed
                             at 64), in blocks of 1024 entries; B rows of >= SPG_HUGE by the whole team, at most HCAP = 64 of them per round;
  k_spgemm_masked_map        the first LCF mask positions accumulate in LDS: 24 576 32-bit counters (PLUS_PAIR on an integer type of >= 4 bytes), 19 660 4-byte
                             words with flag bytes (1- and 2-byte types too: their words start at the identity through k_fill_words), 10 922 8-byte words;
                             A(i,:) in slices of SPG_MAP_SLICE entries; B rows of >= SPG_HUBHUGE_V entries by the whole workgroup; at most 256 position maps;
  grids                      16 384 workgroups for every LDS bin (x 4 one-wave teams in the first), 8192 x 256 threads for the compaction kernels, 16 384 rows
                             per workgroup of k_bin_rows.
The smallest shapes that reach each edge: (a) 72 rows x 2^24 columns (an arithmetic progression of 4096 columns with stride 2^12); (c) 2049 B rows for an A row
of 2 * SPG_LIST_BIG_V + 1 entries; (d) 24 577 mask entries in a row, 4097 B rows for an A row of 2 * SPG_MAP_SLICE + 1 entries, 513 rows for two tasks on
every one of 256 maps; (e) more than 65 536 + 16 384 + 16 384 rows that have entries in A and in M, more than 16 384 x 257 mask entries.  Out of reach: overflow of the hub list of k_spgemm_masked_map (HL = 4096
B rows of >= 32 768 entries referenced by one A row: 4097 distinct B rows, about 1.3e8 entries).

Values are `helpers.rand_values`: small integers (PLUS and TIMES wrap as C does, the narrow types carry their extremes so that PLUS wraps), floating point on
the 1/8 grid without zeros — every sum is exact in any order, and no product is -0.0, whose sum with the +0.0 an accumulator starts from has another sign than
the -0.0 a fold of the products alone gives.  TIMES over floating point rounds (the order would show), so the monoid without a native atomic is TIMES for the
integer types and MAX for the floating-point ones."""
import functools
import os
import re

import numpy as np
import pytest

import matrix_model as MM
import product_model as PM
import pygraphblas_amd as gb
from helpers import TYPE, rand_values
from spgemm_hash_cases import Pattern, hash_col, pick          # (shared with tests/test_spgemm_hash_at_size_gpu.py)
from test_matrix_kernels_at_size_gpu import check, desc_of

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pygraphblas_amd", "csrc", "grb_spgemm_kernels.hpp")
BIN_EDGES = (32, 256, 1024, 4096)                                  # k_bin_rows
TABLE_KEYS = {32: 128, 256: 1024, 1024: 2048, 4096: 8192}           # KS of k_spgemm_masked_lds per bin edge
SPG_LIST, SPG_LIST_BIG, SPG_LONG, SPG_HUGE, SPG_QCAP, HCAP = 512, 1024, 64, 8192, 128, 64
LCAP = (64, SPG_LIST, SPG_LIST, SPG_LIST_BIG)                       # per LDS bin
SPG_MAP_SLICE, SPG_HUBHUGE, MAP_LDS_BYTES, MAX_MAPS = 2048, 32768, 96 * 1024, 256
LCF = {"counters": MAP_LDS_BYTES // 4, "words4": MAP_LDS_BYTES // 5, "words8": MAP_LDS_BYTES // 9}
GRID_CAP, COMPACT_THREADS, BIN_ROWS_PER_BLOCK = 16384, 8192 * 256, 16 * 1024

TYPES, MASK_TYPES, semirings = PM.MXM_TYPES, PM.MXM_MASK_TYPES, PM.mxm_semirings
STATIC = {"BOOL": {"LOR_LAND", "ANY_PAIR", "LOR_PAIR"}, **{t: {"PLUS_TIMES", "MIN_PLUS", "PLUS_PAIR", "PLUS_SECOND", "PLUS_FIRST"} for t in ("INT32", "INT64", "FP32", "FP64")}}
# (semirings(typ): PLUS_TIMES, PLUS_PAIR, MIN_PLUS, a monoid without a native atomic, and MAX_FIRST, which with_semiring instantiates for no type)


def test_the_constants_are_the_headers():
    src = open(HEADER).read()
    for name, v in (("SPG_LIST_V", SPG_LIST), ("SPG_LIST_BIG_V", SPG_LIST_BIG), ("SPG_LONG_V", SPG_LONG), ("SPG_HUGE_V", SPG_HUGE), ("SPG_SLICE_V", SPG_MAP_SLICE),
                    ("SPG_HUBHUGE_V", SPG_HUBHUGE), ("SPG_MAP_LDS_KB_V", MAP_LDS_BYTES // 1024)):
        assert re.search(r"#define %s (\d+)" % name, src).group(1) == str(v), name
    assert "constexpr int SPG_QCAP = %d;" % SPG_QCAP in src and "HCAP = TEAM > 64 ? %d : 1" % HCAP in src and "constexpr uint32_t HL = 4096;" in src
    assert "b = ml <= 32 ? 0 : (ml <= 256 ? 1 : (ml <= 1024 ? 2 : (ml <= lim3 ? 3 : 4)))" in src and re.search(r"lists\.as<uint32_t>\(\),\s+4096u", src)
    assert "if (b > 256u * 64) b = 256u * 64" in src and "if (b > 8192) b = 8192" in src and "constexpr int SPG_BIN_ROWS = 16;" in src
    assert LCF == {"counters": 24576, "words4": 19660, "words8": 10922}
    assert not any(sr in STATIC.get(t, ()) for t in TYPES for sr in ("MAX_FIRST", "TIMES_PLUS", "MAX_PLUS", "LXOR_LAND"))


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------------
def values(rng, typ, n):
    x = rand_values(rng, typ, n)
    if typ.startswith("FP"): x[x == 0] = 0.125
    elif typ in ("INT8", "UINT16") and n:
        at = rng.random(n) < 0.06; i = np.iinfo(MM.NP[typ])
        x[at] = rng.choice(np.array([i.min, i.max, i.max - 1], MM.NP[typ]), size=int(at.sum()))
    return x


def expected_bins(A, M):
    """What k_bin_rows does, from the stored lengths of the two operands."""
    ml = np.bincount(M.rows, minlength=M.nrows); al = np.bincount(A.rows, minlength=A.nrows)
    b = np.searchsorted(np.array(BIN_EDGES), ml[(ml > 0) & (al > 0)], side="left")
    return tuple(int(x) for x in np.bincount(b, minlength=5))


def up(m):
    rp, ci, x = MM.to_csr(m)
    return gb.Matrix.from_csr(TYPE[m.typ], m.nrows, m.ncols, rp, ci, x)


PLAN = re.compile(r"k_spgemm_masked<(static|dynamic)> bins (\d+)/(\d+)/(\d+)/(\d+)/(\d+)( exact)? ")


def product(dv, A, B, M, sr, typ, bins, struct=False, exact=False, C=None, accum=None, replace=False, what=""):
    """One masked product on the device (`dv`: the uploaded A, B, M) and in the model; the plan must name the masked route, the semiring object and `bins`."""
    add, mul = sr.split("_"); T = TYPE[typ]
    assert bins == expected_bins(A, M), (what, bins, expected_bins(A, M))
    c = gb.Matrix.sparse(T, A.nrows, B.ncols) if C is None else up(C)
    dv[0].mxm(dv[1], semiring=getattr(T, sr), mask=dv[2], out=c, accum=getattr(T, accum) if accum else None, desc=desc_of(replace, struct))
    plan = gb.last_kernel_plan() + " "; what = f"{what} {typ}.{sr} mask={M.typ} struct={struct} accum={accum} replace={replace} plan={plan}"
    m = PLAN.search(plan)
    assert m, what
    assert m.group(1) == ("static" if sr in STATIC.get(typ, ()) else "dynamic"), what
    assert tuple(int(g) for g in m.groups()[1:6]) == bins, what
    assert bool(m.group(7)) == exact and ("k_spgemm_masked_ordered" in plan) is False, what
    exp = PM.mxm(MM.empty(A.nrows, B.ncols, typ) if C is None else C, A, B, add, mul, typ, mask=M, struct=struct, replace=replace, accum=(accum, typ) if accum else None)
    check(c, exp, what)
    return exp


def exact_sums(typ, A):
    """A PLUS monoid over floating point is exact in any order: every product is a multiple of 1/64 of size <= 4 (operands on the 1/8 grid, |x| <= 2), and the
    longest A row bounds the terms of a sum."""
    return not typ.startswith("FP") or int(np.bincount(A.rows).max()) * 4 * 64 < 2 ** 24


# ---- (a) the bin ladder -------------------------------------------------------------------------------------------------------------------------------------------
LADDER = [0, 1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 6000]
LADDER_ROWS, LADDER_COLS, LADDER_K = 72, 1 << 24, 40
LADDER_BINS = (3 + 2, 3 + 2, 3 + 2, 3 + 2, 2)                        # per LDS bin: its three ladder rows, and the edge length twice more (progression, crowded)
ROW_MASK_NO_A, ROW_A_NO_MASK = 66, 68


@functools.lru_cache(maxsize=None)
def ladder():
    """The patterns of M, A and B.  M: the ladder lengths in rows 2, 5, 8, ... (random columns; the lengths on a bin edge as a run of consecutive columns), each
    edge length twice more: as an arithmetic progression with the largest power-of-two stride that fits the columns (under hash_col the keys fall into few,
    evenly spaced buckets of the table), and as columns whose hash lies in the last 8 slots of the bin's table, so that the probing wraps round its end.  Row 0 and
    the last rows are empty in A and M, row 66 has mask entries and no A entries, row 68 the reverse.  B row 0 holds nine in ten of all mask columns, the others
    between 0.05 % and 20 % of them plus as many columns outside every mask row; every A row holds k = 0 and eleven more."""
    rng = np.random.default_rng(11); nc = LADDER_COLS
    m = {}; edge_rows = {}
    for q, l in enumerate(LADDER):
        if not l: continue
        if l in BIN_EDGES: start = int(rng.integers(0, nc - l)); m[2 + 3 * q] = np.arange(start, start + l)
        else: m[2 + 3 * q] = pick(rng, nc, l)
    r = 2 + 3 * len(LADDER)
    for l in BIN_EDGES:
        stride = nc // l; ks = TABLE_KEYS[l]
        c0 = max(range(64), key=lambda c: int(hash_col(c + stride * np.arange(l), ks).max()))
        m[r] = c0 + stride * np.arange(l, dtype=np.int64)
        cand = np.arange(nc, dtype=np.int64); cand = cand[hash_col(cand, ks) >= ks - 8]
        m[r + 1] = pick(rng, cand, l)
        edge_rows[l] = (2 + 3 * LADDER.index(l), r, r + 1); r += 2
    assert r <= ROW_MASK_NO_A
    m[ROW_MASK_NO_A] = pick(rng, nc, 50)
    M = Pattern(LADDER_ROWS, nc, m)
    U = np.unique(M.keys % nc)
    a = {i: np.concatenate(([0], pick(rng, np.arange(1, LADDER_K), 11))) for i in m if i != ROW_MASK_NO_A}
    a[ROW_A_NO_MASK] = pick(rng, LADDER_K, 9)
    A = Pattern(LADDER_ROWS, LADDER_K, a)
    b = {}
    for k in range(LADDER_K):
        d = 0.9 if k == 0 else (0.0005, 0.002, 0.01, 0.05, 0.2)[k % 5]
        inside = U[rng.random(len(U)) < d]
        b[k] = np.union1d(inside, rng.integers(0, nc, len(inside) + 5))
    b[7] = np.zeros(0, np.int64)                                                    # an empty B row
    return M, A, Pattern(LADDER_K, nc, b), edge_rows


def ladder_operands(typ, seed):
    Mp, Ap, Bp, _ = ladder(); rng = np.random.default_rng(seed)
    return Ap.mat(values(rng, typ, len(Ap.keys))), Bp.mat(values(rng, typ, len(Bp.keys)))


def test_the_ladder_is_what_the_kernels_need():
    M, A, B, edge_rows = ladder()
    assert sorted(M.lens[M.lens > 0].tolist()) == sorted(LADDER[1:] + [32, 32, 256, 256, 1024, 1024, 4096, 4096, 50])
    assert M.lens[0] == A.lens[0] == 0 and M.lens[-1] == A.lens[-1] == 0 and M.lens[ROW_A_NO_MASK] == 0 < A.lens[ROW_A_NO_MASK] and A.lens[ROW_MASK_NO_A] == 0 < M.lens[ROW_MASK_NO_A]
    ones = np.ones(len(M.keys), bool)
    assert expected_bins(A.mat(np.ones(len(A.keys), bool)), M.mat(ones)) == LADDER_BINS
    assert M.nrows > 64 and len(B.keys) < 1 << 20                                   # (neither the few-rows nor the batch route)
    for l, (run, prog, crowd) in edge_rows.items():
        ks = TABLE_KEYS[l]; assert M.lens[run] == M.lens[prog] == M.lens[crowd] == l
        c = M.cols(run); assert np.all(np.diff(c) == 1)
        c = M.cols(prog); d = np.diff(c); assert np.all(d == d[0]) and d[0] == LADDER_COLS // l and d[0] & (d[0] - 1) == 0
        assert len(np.unique(hash_col(c, ks))) <= max(1, ks >> int(np.log2(d[0]) - 7))       # few buckets
        h = hash_col(M.cols(crowd), ks); assert h.min() >= ks - 8 and l > 8          # a cluster of l keys that starts in the last 8 slots wraps
    assert B.lens[7] == 0 and B.lens[0] >= SPG_HUGE and ((B.lens > 0) & (B.lens < SPG_LONG)).any() and ((B.lens >= 256) & (B.lens < SPG_HUGE)).any()
    assert int(B.lens[A.keys % A.ncols].sum()) < 2e7                                 # products


@pytest.mark.gpu
@pytest.mark.parametrize("typ", [t for t in TYPES if t != "INT32"])
def test_bin_ladder(gpu, typ):
    """(a) Mask rows of 0, 1, 31 | 32 | 33, 255 | 256 | 257, 1023 | 1024 | 1025, 4095 | 4096 | 4097 and 6000 entries under an all-true BOOL mask: every
    semiring of `semirings(typ)`.  An entry of the mask that receives no product is absent from the result.  (INT32 is not among the types here; it runs
    in the list, dense-hit and map cases below.)"""
    Mp, _, _, edge_rows = ladder(); A, B = ladder_operands(typ, 100 + TYPES.index(typ))
    M = Mp.mat(np.ones(len(Mp.keys), bool)); dv = (up(A), up(B), up(M))
    assert exact_sums(typ, A)
    for sr in semirings(typ):
        exp = product(dv, A, B, M, sr, typ, LADDER_BINS, what="ladder")
        got = np.bincount(exp.rows, minlength=M.nrows)
        assert 0 < exp.nvals < M.nvals and all(got[r] > 0 for rows in edge_rows.values() for r in rows) and got[ROW_MASK_NO_A] == 0


# ---- (b) mask values ------------------------------------------------------------------------------------------------------------------------------------------------
def mask_values(rng, mtyp, n):
    """About half false.  True values that a narrower or an integer read would take for false (256, 2^32, 1.5: low bytes / words zero; NaN), false values that
    an integer read of floating point would take for true (-0.0)."""
    t = MM.NP[mtyp]; truth = rng.random(n) < 0.5
    if mtyp == "BOOL": return truth
    if mtyp.startswith("FP"): tv, fv = np.array([1.5, np.nan, -2.0, 2.0 ** -120], t), np.array([0.0, -0.0], t)
    else: tv, fv = np.array({"INT8": [1, -128, 64], "UINT16": [1, 256, 65535], "INT64": [1, 1 << 32, -(1 << 40)]}[mtyp], t), np.array([0], t)
    return np.where(truth, rng.choice(tv, size=n), rng.choice(fv, size=n))


@pytest.mark.gpu
@pytest.mark.parametrize("mtyp", MASK_TYPES)
def test_ladder_under_a_valued_mask(gpu, mtyp):
    """(b) The ladder under a mask of every value width with false entries (the bins count them), the first and the last entry of every row on a bin edge
    false, the rows next to them (31, 33, ...) with a true first and last entry: INT64 PLUS_TIMES and PLUS_PAIR, UINT16 MIN_PLUS; then structural over the same values."""
    Mp, _, _, edge_rows = ladder(); rng = np.random.default_rng(200 + MASK_TYPES.index(mtyp))
    mv = mask_values(rng, mtyp, len(Mp.keys)); zero = np.zeros(1, MM.NP[mtyp])[0]; one = np.ones(1, MM.NP[mtyp])[0]
    for r in np.flatnonzero(Mp.lens > 1):
        on_edge = int(Mp.lens[r]) in BIN_EDGES
        mv[Mp.rp[r]] = mv[Mp.rp[r + 1] - 1] = zero if on_edge else one
    if mtyp.startswith("FP"): mv[Mp.rp[edge_rows[256][0]]] = -0.0; mv[Mp.rp[edge_rows[32][1]] + 1] = np.nan
    M = Mp.mat(mv); truth = MM.mask_truth(mv)
    assert 0.3 < truth.mean() < 0.7
    for typ, srs in (("INT64", ("PLUS_TIMES", "PLUS_PAIR")), ("UINT16", ("MIN_PLUS",))):
        A, B = ladder_operands(typ, 210); dv = (up(A), up(B), up(M))
        for sr in srs:
            exp = product(dv, A, B, M, sr, typ, LADDER_BINS, what="valued mask")
            assert np.isin(exp.keys, M.keys[truth]).all() and exp.nvals < truth.sum()
        if typ == "INT64":
            exp_s = product(dv, A, B, M, "PLUS_TIMES", typ, LADDER_BINS, struct=True, what="structural mask")
            assert exp_s.nvals > exp.nvals and not np.isin(exp_s.keys, M.keys[truth]).all()


# ---- (c) A-row and B-row lengths inside the LDS kernels ---------------------------------------------------------------------------------------------------------------
B_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, SPG_HUGE - 1, SPG_HUGE, SPG_HUGE + 1]
LIST_COLS, LIST_K = 40000, 2200
LIST_MASK_LEN = (20, 200, 800, 3000)                                  # one length inside each LDS bin
N_HUGE = 70                                                           # B rows of >= SPG_HUGE entries, all referenced by one A row: more than HCAP


@functools.lru_cache(maxsize=None)
def lists():
    """Per LDS bin three rows whose A rows hold LCAP, LCAP + 1 and 2 * LCAP + 1 entries (one, two and three staging rounds), each with all of B_LENGTHS among
    its B rows; in the first bin four neighbouring rows with A rows of 1, 200, 3 and 70 entries, seven rows of that bin in all; in the second bin a row whose
    A row references 70 B rows of >= SPG_HUGE entries.  B: rows 0 .. 59 have the lengths of B_LENGTHS three times over, rows 60 .. 129 are huge, the rest
    holds 0 to 40 entries; half of a B row's columns (as far as they reach) come from the union of the mask columns."""
    rng = np.random.default_rng(12); nc = LIST_COLS
    m = {}; a = {}; r = 3
    special = np.arange(len(B_LENGTHS)) + len(B_LENGTHS) * rng.integers(0, 3, len(B_LENGTHS))      # one B row of every length
    rest = np.arange(60 + N_HUGE, LIST_K)
    for b, (ml, cap) in enumerate(zip(LIST_MASK_LEN, LCAP)):
        for al in (cap, cap + 1, 2 * cap + 1):
            m[r] = pick(rng, nc, ml); a[r] = np.union1d(special, pick(rng, rest, al - len(special))); r += 2
    for al in (1, 200, 3, 70):                                                      # neighbours in the first bin's list
        m[r] = pick(rng, nc, int(rng.integers(1, 33))); a[r] = pick(rng, np.concatenate((np.arange(60), rest)), al); r += 1
    r += 1
    m[r] = pick(rng, nc, 200); a[r] = np.union1d(np.arange(60, 60 + N_HUGE), pick(rng, rest, 30)); huge_row = r
    M = Pattern(r + 3, nc, m); A = Pattern(r + 3, LIST_K, a)
    U = np.unique(M.keys % nc); out = np.setdiff1d(np.arange(nc), U)
    lens = np.concatenate((np.tile(B_LENGTHS, 3), SPG_HUGE + rng.integers(0, 600, N_HUGE), rng.integers(0, 41, LIST_K - 60 - N_HUGE)))
    b = {k: np.union1d(pick(rng, U, min(int(l) // 2, len(U))), pick(rng, out, int(l) - min(int(l) // 2, len(U)))) for k, l in enumerate(lens) if l}
    return M, A, Pattern(LIST_K, nc, b), lens, huge_row


LIST_BINS = (3 + 4, 3 + 1, 3, 3, 0)


def test_the_list_shapes_are_what_the_kernels_need():
    M, A, B, lens, huge_row = lists()
    assert np.array_equal(B.lens, lens) and set(B_LENGTHS) <= set(B.lens[:60].tolist()) and (B.lens[60: 60 + N_HUGE] >= SPG_HUGE).all() and N_HUGE > HCAP and len(B.keys) < 1 << 20
    assert expected_bins(A.mat(np.ones(len(A.keys), bool)), M.mat(np.ones(len(M.keys), bool))) == LIST_BINS and LIST_BINS[0] % 4
    al = sorted(A.lens[A.lens > 0].tolist())
    assert all(x in al for cap in LCAP for x in (cap, cap + 1, 2 * cap + 1)) and B.ncols < 65536      # (too few columns for the few-rows route)
    rows0 = np.flatnonzero((M.lens > 0) & (M.lens <= 32))[-4:]
    assert np.all(np.diff(rows0) == 1) and A.lens[rows0].tolist() == [1, 200, 3, 70]
    assert int(np.isin(A.cols(huge_row), np.arange(60, 60 + N_HUGE)).sum()) == N_HUGE and 32 < M.lens[huge_row] <= 256
    assert sum(int(B.lens[A.cols(r)].sum()) for r in np.flatnonzero(A.lens)) < 2e7


@pytest.mark.gpu
@pytest.mark.parametrize("typ", ["BOOL", "UINT16", "INT32", "FP64"])
def test_work_lists_and_b_row_lengths(gpu, typ):
    """(c) The staging rounds of the work lists (A rows of LCAP, LCAP + 1, 2 * LCAP + 1 entries in every LDS bin), B rows of every length at which the walk of
    a row changes (short / long lists, direct lookup / filter and queue, blocks of 1024 and the double-buffered loads, SPG_HUGE - 1 / SPG_HUGE / SPG_HUGE + 1
    for the whole team), and 70 huge B rows under one A row (HCAP = 64: six go to the long list)."""
    Mp, Ap, Bp, _, huge_row = lists(); rng = np.random.default_rng(300 + len(typ))
    A, B = Ap.mat(values(rng, typ, len(Ap.keys))), Bp.mat(values(rng, typ, len(Bp.keys)))
    M = Mp.mat(mask_values(rng, "INT8", len(Mp.keys))); dv = (up(A), up(B), up(M))
    assert exact_sums(typ, A)
    for sr in semirings(typ)[:3]:
        exp = product(dv, A, B, M, sr, typ, LIST_BINS, what="lists")
        assert np.bincount(exp.rows, minlength=M.nrows)[huge_row] > 0
    product(dv, A, B, M, semirings(typ)[0], typ, LIST_BINS, struct=True, what="lists, structural")


DENSE_COLS, DENSE_K = 30000, 48
DENSE_BINS = (4, 4, 4, 4, 0)


@functools.lru_cache(maxsize=None)
def dense():
    """Mask rows of exactly 32, 256, 1024 and 4096 entries (every table at its design load), the first l of one set of 4096 columns; four rows per length with A
    rows of 1, 2, 3 and 24 entries.  B rows hold nine in ten of the 4096 columns and as many others, B rows 0 .. 3 only 60 of the 4096: a mask row of
    >= 256 entries sees more than 128 survivors of the filter in one B row, the rows of 32 collect 64 over consecutive B rows, and an A row of one entry leaves
    fewer than 64 survivors to the flush at the end of the mask row."""
    rng = np.random.default_rng(13); nc = DENSE_COLS
    W = pick(rng, nc, 4096); out = np.setdiff1d(np.arange(nc), W)
    m = {}; a = {}; r = 1
    for l in BIN_EDGES:
        for al in (1, 2, 3, 24):
            m[r] = W[:l]; a[r] = pick(rng, DENSE_K, al) if al > 1 else np.array([int(rng.integers(4, DENSE_K))]); r += 1
        a[r - 4] = np.array([r % 4])                                                # (one of the one-entry A rows meets a B row with few hits)
    b = {k: np.union1d(W[rng.random(4096) < 0.9] if k >= 4 else pick(rng, W[:300], 60), pick(rng, out, 3700)) for k in range(DENSE_K)}
    return Pattern(70, nc, m), Pattern(70, DENSE_K, a), Pattern(DENSE_K, nc, b)


@pytest.mark.gpu
@pytest.mark.parametrize("typ", ["INT32", "FP32", "INT8"])
def test_dense_hits_through_the_survivor_queue(gpu, typ):
    """(c) B rows that lie mostly inside the mask row.  PLUS_PAIR on INT32 / FP32 is pattern-only (the queue is carried from B row to B row and flushed at the end
    of the mask row), PLUS_TIMES reads values (flushed per B row); INT8 runs both through the dynamic semiring object (never pattern-only)."""
    Mp, Ap, Bp = dense(); rng = np.random.default_rng(320 + len(typ))
    assert expected_bins(Ap.mat(np.ones(len(Ap.keys), bool)), Mp.mat(np.ones(len(Mp.keys), bool))) == DENSE_BINS and Bp.lens.min() >= 256
    A, B = Ap.mat(values(rng, typ, len(Ap.keys))), Bp.mat(values(rng, typ, len(Bp.keys)))
    M = Mp.mat(np.ones(len(Mp.keys), bool)); dv = (up(A), up(B), up(M))
    for sr in ("PLUS_PAIR", "PLUS_TIMES", "MIN_PLUS"):
        exp = product(dv, A, B, M, sr, typ, DENSE_BINS, what="dense hits")
        per_row = np.bincount(exp.rows, minlength=M.nrows)
        assert per_row.max() > 0.85 * 4096 and 0 < per_row[Mp.lens == 256].min() < 64 and per_row[Mp.lens == 32].max() == 32


# ---- (d) the HBM-map kernel -------------------------------------------------------------------------------------------------------------------------------------------
MAP_COLS, MAP_LONG, MAP_K = 50000, 64, 64 + 4200
MAP_MASK_LENS = [l + d for l in (LCF["words8"], LCF["words4"], LCF["counters"]) for d in (-1, 0, 1)]
MAP_SLICED = (SPG_MAP_SLICE, SPG_MAP_SLICE + 1, 2 * SPG_MAP_SLICE + 1)


@functools.lru_cache(maxsize=None)
def mapped():
    """Rows 1 .. 9: mask rows of LCF - 1, LCF, LCF + 1 entries for the three accumulator layouts, A rows of 20 of the 64 long B rows (about 5000 entries each)
    plus B rows 0 and 1, which hold the mask row's columns at the positions LCF - 2 .. LCF + 1 of every layout: products land on the last LDS position and on
    the first HBM position.  Rows 12 .. 14: mask rows of 24 577 entries (positions on both sides of every LCF) with A rows of SPG_MAP_SLICE, SPG_MAP_SLICE + 1
    and 2 * SPG_MAP_SLICE + 1 of the 4200 short B rows: two or three workgroups combine into one row's slots, while the short A rows of rows 1 .. 9 skip their
    later slices.  Row 16 references B row 2 of SPG_HUBHUGE_V + 100 entries.  Row 18: a mask row of 4097 entries, the shortest of the bin."""
    rng = np.random.default_rng(14); nc = MAP_COLS
    m = {}; a = {}; must = []
    for q, l in enumerate(MAP_MASK_LENS):
        m[1 + q] = pick(rng, nc, l); a[1 + q] = np.union1d([0, 1], pick(rng, np.arange(3, MAP_LONG), 20))
        must.append(m[1 + q][[p for f in LCF.values() for p in range(f - 2, f + 2) if p < l]])
    short = np.arange(MAP_LONG, MAP_K)
    for q, al in enumerate(MAP_SLICED):
        m[12 + q] = pick(rng, nc, LCF["counters"] + 1); a[12 + q] = pick(rng, short, al)
    m[16] = pick(rng, nc, 12000); a[16] = np.array([2, 5, 70, 80])
    m[18] = pick(rng, nc, 4097); a[18] = pick(rng, MAP_K, 40)
    must = np.unique(np.concatenate(must))
    b = {0: must, 1: np.union1d(must, pick(rng, nc, 300)), 2: pick(rng, nc, SPG_HUBHUGE + 100)}
    for k in range(3, MAP_LONG): b[k] = pick(rng, nc, int(rng.integers(4000, 6000)))
    for k in short: b[int(k)] = pick(rng, nc, int(rng.integers(1, 60)))
    return Pattern(80, nc, m), Pattern(80, MAP_K, a), Pattern(MAP_K, nc, b)


MAP_BINS = (0, 0, 0, 0, 9 + 3 + 2)


def test_the_map_shapes_are_what_the_kernel_needs():
    M, A, B = mapped()
    assert expected_bins(A.mat(np.ones(len(A.keys), bool)), M.mat(np.ones(len(M.keys), bool))) == MAP_BINS
    assert sorted(M.lens[1:10].tolist()) == sorted(MAP_MASK_LENS) and A.lens[12:15].tolist() == list(MAP_SLICED) and A.lens[1:10].max() < SPG_MAP_SLICE
    assert B.lens[2] >= SPG_HUBHUGE and 2 in A.cols(16) and M.lens[18] == BIN_EDGES[3] + 1 and M.nrows > 64
    assert sum(int(B.lens[A.cols(r)].sum()) for r in np.flatnonzero(A.lens)) < 2e7


@pytest.mark.gpu
@pytest.mark.parametrize("typ,sr,layout", [("INT32", "PLUS_PAIR", "counters"), ("INT64", "PLUS_PAIR", "counters"), ("INT32", "PLUS_TIMES", "words4"), ("FP32", "PLUS_TIMES", "words4"),
                                           ("INT64", "PLUS_TIMES", "words8"), ("FP64", "MIN_PLUS", "words8"), ("UINT16", "MIN_PLUS", "words4"), ("INT8", "PLUS_TIMES", "words4"),
                                           ("INT8", "PLUS_PAIR", "words4"), ("INT64", "TIMES_PLUS", "words8"), ("BOOL", "LXOR_LAND", "words4")])
def test_map_kernel_at_the_lds_boundary_and_the_slice_edge(gpu, typ, sr, layout):
    """(d) Every accumulator layout of k_spgemm_masked_map with hits on both sides of its LCF, A rows at the slice edge (`shared_row`: several workgroups combine
    into one row's slots, in LDS and in HBM), the narrow types' 32-bit words (MIN: the HBM words must start at the identity, k_fill_words) and one B row the whole
    workgroup walks.  The mask is UINT16 with false entries."""
    Mp, Ap, Bp = mapped(); rng = np.random.default_rng(400 + len(typ) + len(sr))
    A, B = Ap.mat(values(rng, typ, len(Ap.keys))), Bp.mat(values(rng, typ, len(Bp.keys)))
    mv = mask_values(rng, "UINT16", len(Mp.keys))
    f = LCF[layout]
    for r in range(1, 10): mv[Mp.rp[r] + f - 2: min(Mp.rp[r] + f + 2, Mp.rp[r + 1])] = 256           # (the positions round LCF are allowed)
    M = Mp.mat(mv); dv = (up(A), up(B), up(M))
    assert exact_sums(typ, A)
    exp = product(dv, A, B, M, sr, typ, MAP_BINS, what=f"map {layout}")
    for r in range(1, 10):
        want = np.int64(r) * MAP_COLS + Mp.cols(r)[f - 2: f + 2]
        assert np.isin(want, exp.keys).all(), (r, layout)
    assert all(np.bincount(exp.rows, minlength=80)[r] > 0 for r in (12, 13, 14, 16, 18))


TASK_ROWS, TASK_COLS, TASK_K = 2 * MAX_MAPS + 8, 1 << 20, 300


@functools.lru_cache(maxsize=None)
def tasks():
    """520 rows with mask rows of 4097 entries: 256 maps, so every workgroup runs two or three tasks on its map.  A stale map entry is read only where a
    product of the later row passes the row's bit filter (2^18 bits, a multiplicative hash that no two of the first 2^18 columns share): every column in use
    comes from a pool of 5000 filter bits x 4 columns out of 2^20, so four columns in five have a pool column with their filter bit in a mask row.  The mask
    rows come from the lower or the upper half of the pool in turn (the order of a bin's list is settled by atomics: whichever rows follow one another on a
    map, they share about 40 % of their columns or none), B rows hold about 1000 pool columns, A rows 10 entries."""
    rng = np.random.default_rng(15); nc = TASK_COLS
    cols = np.arange(nc, dtype=np.uint64)
    fbit = (((cols & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779)) & np.uint64(0xFFFFFFFF)) >> np.uint64(14)      # fbit of k_spgemm_masked_map: SPG_FILTER_MUL, 2^18 bits
    order = np.argsort(fbit, kind="stable"); sf = fbit[order]
    start = np.flatnonzero(np.concatenate(([True], sf[1:] != sf[:-1]))); size = np.diff(np.concatenate((start, [nc])))
    start = start[size >= 4][:5000]
    pool = np.sort(order[(start[:, None] + np.arange(4)[None, :]).reshape(-1)]).astype(np.int64)
    assert len(pool) == 20000 and len(np.unique(fbit[pool])) == 5000
    m = {r: pick(rng, pool[: 10000] if rng.integers(0, 2) else pool[10000:], 4097) for r in range(TASK_ROWS)}
    a = {r: pick(rng, TASK_K, 10) for r in range(TASK_ROWS)}
    b = {k: pick(rng, pool, int(rng.integers(800, 1200))) for k in range(TASK_K)}
    return Pattern(TASK_ROWS, nc, m), Pattern(TASK_ROWS, TASK_K, a), Pattern(TASK_K, nc, b)


@pytest.mark.gpu
@pytest.mark.parametrize("typ,sr", [("INT64", "PLUS_PAIR"), ("FP32", "PLUS_TIMES"), ("INT8", "MIN_PLUS")])
def test_map_kernel_runs_several_tasks_on_one_map(gpu, typ, sr):
    """(d) More rows than position maps: the clean-up at the end of a task is what keeps the next row on the map right.  A third of the rows carry false mask
    entries (cleaned up like the true ones)."""
    Mp, Ap, Bp = tasks(); rng = np.random.default_rng(430 + len(typ))
    A, B = Ap.mat(values(rng, typ, len(Ap.keys))), Bp.mat(values(rng, typ, len(Bp.keys)))
    mv = np.ones(len(Mp.keys), np.float32)
    for r in range(0, TASK_ROWS, 3): mv[Mp.rp[r]: Mp.rp[r + 1]] = mask_values(rng, "FP32", 4097)
    M = Mp.mat(mv); dv = (up(A), up(B), up(M))
    assert TASK_ROWS > 2 * MAX_MAPS and len(Bp.keys) < 1 << 20 and len(Ap.keys) * 1200 < 2e7
    product(dv, A, B, M, sr, typ, (0, 0, 0, 0, TASK_ROWS), what="tasks on one map")


# ---- (e) grid rounds ----------------------------------------------------------------------------------------------------------------------------------------------------
ROUNDS_N = (4 * GRID_CAP + 2000, GRID_CAP + 600, GRID_CAP + 600)          # rows with mask rows of the first three bins; one in 50 has no A entries and goes into no bin
ROUNDS_COLS, ROUNDS_K, ROUNDS_TRAIL = 3000, 512, 77


@functools.lru_cache(maxsize=None)
def rounds(last_hit):
    """67 536 rows with mask rows of 1 or 2 entries, 16 984 of 33 to 40, 16 984 of 257, then 77 rows with entries in A and none in M; A rows of 1 to 3 entries
    (every 50th row none), B rows of 0 to 32 entries.  The first mask entry of a row is a column of the B row its first A entry names (a product lands), the
    others are random.  `last_hit`: the very last mask entry receives a product, or is the one column no B row holds."""
    rng = np.random.default_rng(16); nc = ROUNDS_COLS; n = sum(ROUNDS_N) + ROUNDS_TRAIL
    blen = rng.integers(0, 33, ROUNDS_K); blen[:8] = 0
    brp = np.concatenate(([0], np.cumsum(blen)))
    bcol = np.concatenate([pick(rng, nc - 1, int(l)) for l in blen])
    alen = rng.integers(1, 4, n); alen[::50] = 0
    arow = np.repeat(np.arange(n, dtype=np.int64), alen)
    ak = rng.integers(0, ROUNDS_K // 4, len(arow)) * 4 + (np.arange(len(arow)) - np.repeat(np.cumsum(alen) - alen, alen))      # distinct inside a row: k = 4 x + position
    A = MM.Mat(n, ROUNDS_K, np.sort(arow * ROUNDS_K + ak), np.zeros(len(arow), bool))
    mlen = np.concatenate((rng.integers(1, 3, ROUNDS_N[0]), rng.integers(33, 41, ROUNDS_N[1]), np.full(ROUNDS_N[2], 257), np.zeros(ROUNDS_TRAIL, np.int64)))
    mrow = np.repeat(np.arange(n, dtype=np.int64), mlen)
    # columns: a random start and steps of 1 .. 11 (distinct, ascending, inside the columns: 257 x 11 < 3000 - 1)
    step = rng.integers(1, 12, len(mrow)); first = np.cumsum(mlen) - mlen
    step[first[mlen > 0]] = 0
    run = np.cumsum(step); run -= np.repeat(run[first[mlen > 0]], mlen[mlen > 0])
    start = rng.integers(0, nc - 1 - 257 * 11, n)
    # the first entry: a column of B(k0, :) where row i has an A entry and that B row is not empty (then the run starts there, if it fits)
    afirst = np.searchsorted(A.keys, np.arange(n, dtype=np.int64) * ROUNDS_K); has_a = alen > 0
    k0 = np.where(has_a, A.keys[np.minimum(afirst, A.nvals - 1)] % ROUNDS_K, 0)
    ok = has_a & (blen[k0] > 0)
    c0 = bcol[np.minimum(brp[k0] + rng.integers(0, 1 << 30, n) % np.maximum(blen[k0], 1), len(bcol) - 1)]
    start = np.where(ok & (c0 + mlen * 11 < nc - 1), c0, start)
    mcol = np.repeat(start, mlen) + run
    # the very last mask entry: column nc - 2, which the B row of its row's first A entry holds, or column nc - 1, which no B row holds
    last_row = int(mrow[-1]); assert has_a[last_row] and last_row == sum(ROUNDS_N) - 1
    mcol[-1] = nc - 2 if last_hit else nc - 1
    bkeys = np.union1d(np.repeat(np.arange(ROUNDS_K, dtype=np.int64), blen) * nc + bcol, [k0[last_row] * nc + nc - 2])
    M = MM.Mat(n, nc, mrow * nc + mcol, np.zeros(len(mrow), bool))
    return M, A, MM.Mat(ROUNDS_K, nc, bkeys, np.zeros(len(bkeys), bool))


@pytest.mark.gpu
@pytest.mark.parametrize("last_hit", [True, False])
def test_grid_rounds_of_every_kernel(gpu, last_hit):
    """(e) More rows than one round of each LDS bin's grid (16 384 workgroups, four teams in the first bin), more mask entries than one round of the compaction
    kernels (8192 x 256), a second and up to a seventh workgroup of k_bin_rows, trailing rows with an empty mask (`p < mnz ? pos[p] : total`), and the very last
    mask entry with and without a product (`total = lastp + lastf`).  INT32 PLUS_TIMES under an INT8 mask with false entries, UINT16 PLUS_PAIR structural."""
    Mk, Ak, Bk = rounds(last_hit); rng = np.random.default_rng(500)
    ml = np.bincount(Mk.rows, minlength=Mk.nrows); al = np.bincount(Ak.rows, minlength=Ak.nrows)
    bins = expected_bins(Ak, Mk)
    assert bins[0] > 4 * GRID_CAP and bins[1] > GRID_CAP and bins[2] > GRID_CAP and bins[3:] == (0, 0) and all(bins[q] < ROUNDS_N[q] for q in range(3))
    assert Mk.nvals > COMPACT_THREADS and Mk.nrows > 6 * BIN_ROWS_PER_BLOCK
    assert (ml[-ROUNDS_TRAIL:] == 0).all() and (al[-ROUNDS_TRAIL:] > 0).any() and Mk.nvals + Ak.nvals * 32 < 2e7
    mv = mask_values(rng, "INT8", Mk.nvals); mv[-1] = 1
    M = MM.Mat(Mk.nrows, Mk.ncols, Mk.keys, mv)
    for typ, sr, struct in (("INT32", "PLUS_TIMES", False), ("UINT16", "PLUS_PAIR", True)):
        A = MM.Mat(Ak.nrows, Ak.ncols, Ak.keys, values(rng, typ, Ak.nvals)); B = MM.Mat(Bk.nrows, Bk.ncols, Bk.keys, values(rng, typ, Bk.nvals))
        exp = product((up(A), up(B), up(M)), A, B, M, sr, typ, bins, struct=struct, what=f"grid rounds, last entry hit: {last_hit}")
        assert (exp.nvals > 0 and exp.keys[-1] == M.keys[-1]) == last_hit
        got = np.bincount(exp.rows, minlength=M.nrows)
        s1, s2 = ROUNDS_N[0], ROUNDS_N[0] + ROUNDS_N[1]
        assert got[:s1].sum() > 5000 and got[s1:s2].sum() > 5000 and got[s2:].sum() > 5000 and got[-ROUNDS_TRAIL:].sum() == 0


# ---- (f) the write-back -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("replace", [False, True])
def test_ladder_accumulates_into_a_matrix_with_entries(gpu, replace):
    """(f) C<M> += A (+).(x) B, INT64 PLUS_TIMES on the ladder under a valued mask: C holds entries at true, at false and outside of mask positions."""
    Mp, _, _, _ = ladder(); rng = np.random.default_rng(600)
    A, B = ladder_operands("INT64", 601); M = Mp.mat(mask_values(rng, "INT8", len(Mp.keys)))
    ck = np.union1d(Mp.keys[rng.random(len(Mp.keys)) < 0.3], rng.integers(0, LADDER_ROWS * LADDER_COLS, 4000))
    C = MM.Mat(LADDER_ROWS, LADDER_COLS, ck, values(rng, "INT64", len(ck)))
    inside = np.isin(C.keys, M.keys)
    assert inside.any() and (~inside).any() and np.isin(C.keys, M.keys[~MM.mask_truth(M.vals)]).any()
    exp = product((up(A), up(B), up(M)), A, B, M, "PLUS_TIMES", "INT64", LADDER_BINS, C=C, accum="PLUS", replace=replace, what="accumulate")
    assert np.isin(C.keys[~inside], exp.keys).all() != replace


# ---- (g) deterministic mode -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ladder_with_exact_accumulators(gpu, monkeypatch):
    """(g) FP64 PLUS_TIMES under GRB_MI355X_DETERMINISTIC=1: the same bins with 128-bit accumulators (` exact` in the plan; no row is handed to the ordered
    kernel: the values lie within a few binades).  The last LDS bin keeps its 4096 mask entries with 16-byte accumulators, a smaller filter and lists of 512:
    the rows of 4095 and 4096 entries are its edge."""
    monkeypatch.setenv("GRB_MI355X_DETERMINISTIC", "1")
    Mp, _, _, _ = ladder(); A, B = ladder_operands("FP64", 700)
    M = Mp.mat(np.ones(len(Mp.keys), bool))
    product((up(A), up(B), up(M)), A, B, M, "PLUS_TIMES", "FP64", LADDER_BINS, exact=True, what="exact")
