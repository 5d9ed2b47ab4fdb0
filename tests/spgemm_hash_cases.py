"""Operand patterns for tests/test_spgemm_hash_at_size_gpu.py (test infrastructure; numpy only, the library is never imported): the smallest A / B pairs that
put rows of the unmasked product `T = A (+).(x) B` on the constants of pygraphblas_amd/csrc/grb_spgemm_hash.hpp, and what the driver must then report:
  ub(i)  = sum of nnz(B(k,:)) over the entries k of A(i,:)     the product count, by which run_spgemm_hash bins the rows for the symbolic pass;
  ent(i) = the distinct columns among those products            the entry count of T(i,:), by which it bins them again for the numeric pass;
  bins(ub, ent, mode)                                           the nine counts of the plan string, per mode (the limits differ, see SYM_LIMITS / NUM_LIMITS).
Every builder returns a `Case`: the two patterns, ub and ent as the builder knows them BY CONSTRUCTION (`products_of` / `entries_of` recompute them from the
patterns: tests/test_spgemm_hash_cases_host.py holds the two against each other) and the rows the case exists for.  `Pattern`, `pick` and `hash_col` are
those of tests/test_spgemm_masked_at_size_gpu.py, which imports them from here."""
import functools

import numpy as np

# ---- the header's constants -----------------------------------------------------------------------------------------------------------------------------------
MODES = ("ranked", "blocks", "hbm", "ordered")
SYM_LIMITS = {"ranked": (128, 1024, 1024, 1024), "blocks": (128, 1024, 4096, 4096), "hbm": (128, 1024, 4096, 16384), "ordered": (128, 128, 128, 128)}      # k_hash_bin5: l0 .. l3
NUM_LIMITS = {"ranked": (128, 1024, 1024), "blocks": (128, 1024, 4096), "hbm": (128, 1024, 4096), "ordered": (128, 128, 128)}                               # k_hash_bin: l0 .. l2
SYM_SLOTS, NUM_SLOTS = (256, 2048, 8192, 32768), (256, 2048, 8192)         # a table holds twice its bin's limit
SYM_GROUPS, NUM_GROUPS = (4, 16, 32, 64), (4, 16, 64)                      # 16-lane groups per team (TEAM / 16)
TEAMS_BIN0 = 4                                                             # one-wave teams per workgroup of the first bin
GRID_CAP_PER_CU = 32                                                       # workgroups per CU of a table kernel's grid
BIN_THREADS = 8192 * 256                                                   # one round of k_hash_bin / k_hash_bin5 / k_table_counts / k_hash_total
SPA_MAX_COLS = 1 << 20                                                     # the LDS dense path: up to 2^20 columns, else the HBM accumulators
WD = {8: 16384, 4: 28672}                                                  # columns per block of the LDS dense path, by accumulator word (narrow types: 4-byte words)
HASH_MUL = 2654435761
DIM_MAX = 0xFFFFFFF0                                                       # GRB_DIM_DEVICE_MAX


def hash_col(j, keys):
    """hash_col of the header for a table of `keys` slots."""
    return (((np.asarray(j, np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(7)).astype(np.int64) & (keys - 1)


def preimages(slots, keys, ncols, rng, want):
    """At least `want` columns below `ncols` whose hash_col lies in `slots`, ascending: the multiplier is odd, so j = y / HASH_MUL (mod 2^32) for every 32-bit y
    whose bits 7 .. carry the slot."""
    sh = 7 + int(np.log2(keys)); inv = np.uint64(pow(HASH_MUL, -1, 1 << 32)); nhi = 1 << (32 - sh)
    take = min(nhi, max(64, (64 * want * (1 << 32)) // (len(slots) * 128 * ncols)))
    hi = np.sort(rng.choice(nhi, size=take, replace=False)).astype(np.uint64)
    y = (hi[:, None, None] << np.uint64(sh)) | (np.asarray(slots, np.uint64)[None, :, None] << np.uint64(7)) | np.arange(128, dtype=np.uint64)[None, None, :]
    j = np.unique((y.reshape(-1) * inv) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    j = j[j < ncols]
    assert len(j) >= want, (len(j), want)
    return j


class Pattern:
    """Rows as {row: ascending columns}; every other row is empty."""

    def __init__(self, nrows, ncols, rows):
        self.nrows, self.ncols = nrows, ncols
        at = sorted(r for r in rows if len(rows[r]))
        self.lens = np.zeros(nrows, np.int64)
        for r in at:
            c = np.asarray(rows[r], np.int64); self.lens[r] = len(c)
            assert np.all(np.diff(c) > 0) and 0 <= c[0] and c[-1] < ncols, r
        self.keys = np.concatenate([np.int64(r) * ncols + np.asarray(rows[r], np.int64) for r in at]) if at else np.zeros(0, np.int64)
        self.rp = np.concatenate(([0], np.cumsum(self.lens)))

    def mat(self, vals):
        import matrix_model as MM
        return MM.Mat(self.nrows, self.ncols, self.keys, vals)

    def cols(self, r):
        return self.keys[self.rp[r]: self.rp[r + 1]] - np.int64(r) * self.ncols


def pick(rng, pool, n):
    """n distinct members of `pool` (an array, or a range end), ascending."""
    return np.sort(rng.choice(pool, size=n, replace=False)).astype(np.int64)


# ---- what the driver computes from the patterns -------------------------------------------------------------------------------------------------------------------
def products_of(A, B):
    """ub(i) for every row of A."""
    ub = np.zeros(A.nrows, np.int64)
    np.add.at(ub, A.keys // A.ncols, B.lens[A.keys % A.ncols])
    return ub


def entries_of(A, B):
    """ent(i) for every row of A: the products expanded, their distinct (row, column) keys counted."""
    k = A.keys % A.ncols; cnt = B.lens[k]
    first = np.cumsum(cnt) - cnt
    pb = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first - B.rp[k], cnt)
    key = np.unique(np.repeat(A.keys // A.ncols, cnt) * np.int64(B.ncols) + B.keys[pb] % B.ncols)
    return np.bincount(key // B.ncols, minlength=A.nrows).astype(np.int64)


def bins(ub, ent, mode):
    """The nine counts of the plan: symbolic a/b/c/d/e by product count, numeric a/b/c/d by entry count; a row without products joins no bin."""
    ub, ent = np.asarray(ub), np.asarray(ent)
    assert np.array_equal(ub > 0, ent > 0) and np.all(ent <= ub)
    s = np.bincount(np.searchsorted(np.array(SYM_LIMITS[mode]), ub[ub > 0], side="left"), minlength=5)
    n = np.bincount(np.searchsorted(np.array(NUM_LIMITS[mode]), ent[ent > 0], side="left"), minlength=4)
    return tuple(int(x) for x in s) + tuple(int(x) for x in n)


def effective_mode(mode, typ, add, ncols):
    """The limits a call runs under: the HBM accumulators beyond 2^20 columns whatever is set; the ordered bins only for a floating-point monoid whose
    result depends on the order (not MIN / MAX)."""
    if mode == "hbm" or ncols > SPA_MAX_COLS: return "hbm"
    if mode == "ordered": return "ordered" if typ.startswith("FP") and add not in ("MIN", "MAX") else "ranked"
    return mode


class Case:
    def __init__(self, A, B, ub, ent, **facts):
        self.A, self.B, self.ub, self.ent = A, B, np.asarray(ub, np.int64), np.asarray(ent, np.int64)
        self.__dict__.update(facts)

    def bins(self, mode):
        return bins(self.ub, self.ent, mode)


class _Rows:
    """B (or A) under construction: add(columns) -> the new row's number."""

    def __init__(self): self.rows = []

    def add(self, cols):
        self.rows.append(np.asarray(cols, np.int64)); return len(self.rows) - 1

    def pattern(self, ncols, nrows=None):
        return Pattern(len(self.rows) if nrows is None else nrows, ncols, {k: c for k, c in enumerate(self.rows)})


# ---- (a) the ladder -------------------------------------------------------------------------------------------------------------------------------------------------
LADDER = [0, 1, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 20000]
LADDER_ROWS, LADDER_COLS = 80, 40000
CROWD = (1, 128, 129)                                   # few columns for every product count above them ...
CROWD_HIGH = (1024, 1025, 4096, 4097)                   # ... and the numeric limits reached from the highest symbolic bins (16384, 16385, 20000 products)
ROW_ONLY_EMPTY_B, ROW_WITH_EMPTY_B = 76, 77             # an A row that references empty B rows alone (ub = 0); one that references one among full ones


@functools.lru_cache(maxsize=None)
def ladder():
    """Every product count p of LADDER twice.  DISTINCT: the A row references the B `pieces` of its binary digits (piece b: 2^b columns, the pieces pairwise
    disjoint), so its p products fall on p columns.  CROWDED on c columns: p // c B rows that hold the same c columns each (Q[:c]) and one that holds the
    first p % c of them — p products, c entries, p // c or p // c + 1 combines per slot.  Rows 0 and 78, 79 of A are empty, B rows 0 and 1 are empty."""
    rng = np.random.default_rng(21); nc = LADDER_COLS
    B = _Rows(); e0, e1 = B.add([]), B.add([])
    perm = rng.permutation(nc)[:(1 << 15) - 1]
    piece = [B.add(np.sort(perm[(1 << b) - 1: (2 << b) - 1])) for b in range(15)]
    Q = rng.permutation(nc)[:max(CROWD_HIGH)]
    full = {c: [B.add(np.sort(Q[:c])) for _ in range(max(LADDER) // c)] for c in CROWD + CROWD_HIGH}
    a = {}; ub = np.zeros(LADDER_ROWS, np.int64); ent = np.zeros(LADDER_ROWS, np.int64); rows = []; r = 1
    for p in LADDER[1:]:
        a[r] = np.sort([piece[b] for b in range(15) if p >> b & 1]); ub[r] = ent[r] = p; rows.append((r, p, None)); r += 1
        for c in CROWD + (CROWD_HIGH if p >= 16384 else ()):
            if p <= c: continue
            ks = full[c][: p // c] + ([B.add(np.sort(Q[: p % c]))] if p % c else [])
            a[r] = np.sort(ks); ub[r] = p; ent[r] = c; rows.append((r, p, c)); r += 1
    assert r <= ROW_ONLY_EMPTY_B
    a[ROW_ONLY_EMPTY_B] = np.sort([e0, e1])
    a[ROW_WITH_EMPTY_B] = np.sort([e0, piece[0], piece[7]]); ub[ROW_WITH_EMPTY_B] = ent[ROW_WITH_EMPTY_B] = 129
    Bp = B.pattern(nc)
    return Case(Pattern(LADDER_ROWS, Bp.nrows, a), Bp, ub, ent, rows=tuple(rows))


# ---- (b) clustered and wrapping keys -----------------------------------------------------------------------------------------------------------------------------------
CLUSTER_ROWS = 70
CLUSTER_COLS = {256: DIM_MAX, 2048: DIM_MAX, 8192: DIM_MAX, 32768: 1 << 30}


@functools.lru_cache(maxsize=None)
def clustered(slots):
    """Four rows of slots / 2 distinct columns each, on the limit of the table of `slots` slots (symbolic; for 256 / 2048 / 8192 numeric too: entries = products):
    row 3 `wrap`: hash_col in the last 8 slots, so the probing wraps round the table's end; row 5 `slot`: every key hashes to ONE slot, slots - 3 (a probe chain of
    slots / 2 that wraps as well) — an arithmetic progression whose stride is the largest power of two that keeps slots / 2 terms below GRB_DIM_DEVICE_MAX (2^25,
    2^22, 2^20: the stride's multiples leave the hash bits alone), and for 32 768 slots, where that stride (2^17) is below the hash bits' end (2^22), the slot's
    preimages below 2^30; row 7 `run`: consecutive columns; row 9 `any`: random ones.  Three B rows per A row share a row's columns out, position mod 3."""
    rng = np.random.default_rng(22 + slots); nc = CLUSTER_COLS[slots]; n = slots // 2
    cols = {3: pick(rng, preimages(range(slots - 8, slots), slots, nc, rng, n), n)}
    if slots < 32768:
        stride = 1 << int(np.log2((1 << 32) // n)); cand = preimages([slots - 3], slots, min(nc, stride - 16), rng, 1)
        cols[5] = int(cand[0]) + stride * np.arange(n, dtype=np.int64)
    else:
        stride = 0; cols[5] = pick(rng, preimages([slots - 3], slots, nc, rng, n), n)
    start = int(rng.integers(0, 1 << 20)); cols[7] = np.arange(start, start + n, dtype=np.int64)
    cols[9] = pick(rng, 1 << 24, n)
    B = _Rows(); B.add([]); a = {}; ub = np.zeros(CLUSTER_ROWS, np.int64)
    for r, c in cols.items():
        a[r] = np.array([B.add(c[q::3]) for q in range(3)]); ub[r] = n
    for r in range(12, 60, 2):                                                       # company: rows of a few products in the first bin
        a[r] = np.array([B.add(pick(rng, 1 << 24, int(rng.integers(1, 40))))]); ub[r] = len(B.rows[-1])
    Bp = B.pattern(nc)
    return Case(Pattern(CLUSTER_ROWS, Bp.nrows, a), Bp, ub, ub.copy(), wrap=3, slot=5, run=7, stride=stride, n=n)


# ---- (c) team shapes -------------------------------------------------------------------------------------------------------------------------------------------------------
TEAM_LIMITS = (128, 1024, 4096, 16384)
TEAM_A_COUNTS = tuple(ng + d for ng in (4, 16, 32, 64) for d in (-1, 0, 1))
TEAM_B_LENGTHS = (15, 16, 17, 31, 32, 33)
TEAM_COLS = 30000


@functools.lru_cache(maxsize=None)
def teams():
    """Per limit L of TEAM_LIMITS twenty rows of exactly L products: one A entry and a B row of L entries (one 16-lane group does all the work); L A entries and
    B rows of one entry; n A entries for n in TEAM_A_COUNTS (n - 1 B rows of L // n entries and one with the rest: every group count NG = 4, 16, 32, 64 of the
    kernels sees NG - 1, NG and NG + 1 entries); B rows of l entries for l in TEAM_B_LENGTHS (L // l of them and one with the rest: whole and broken rounds of
    16 lanes).  The unit rows have distinct columns; the others are random, so their rows hold fewer entries than products."""
    rng = np.random.default_rng(23); nc = TEAM_COLS
    B = _Rows(); B.add([])
    unit = [B.add([c]) for c in rng.permutation(nc)[:max(TEAM_LIMITS)]]
    pool = {l: [B.add(pick(rng, nc, l)) for _ in range(max(TEAM_LIMITS) // l)] for l in TEAM_B_LENGTHS}
    a = {}; ways = {}; r = 1
    for L in TEAM_LIMITS:
        a[r] = np.array([B.add(pick(rng, nc, L))]); ways[r] = (L, "one long", 1); r += 1
        a[r] = np.sort(unit[:L]); ways[r] = (L, "units", L); r += 1
        for n in TEAM_A_COUNTS:
            a[r] = np.array([B.add(pick(rng, nc, L // n)) for _ in range(n - 1)] + [B.add(pick(rng, nc, L - (n - 1) * (L // n)))]); ways[r] = (L, "entries", n); r += 1
        for l in TEAM_B_LENGTHS:
            a[r] = np.sort(pool[l][: L // l] + ([B.add(pick(rng, nc, L % l))] if L % l else [])); ways[r] = (L, "lengths", l); r += 1
    Bp = B.pattern(nc); Ap = Pattern(r + 3, Bp.nrows, a)
    ub = np.zeros(Ap.nrows, np.int64)
    for q, w in ways.items(): ub[q] = w[0]
    return Case(Ap, Bp, ub, entries_of(Ap, Bp), ways=ways)


# ---- (d) dead teams, grid rounds, many rows ------------------------------------------------------------------------------------------------------------------------------
def single_entry_rows(seed, nrows, live, ncols, lengths, nb=48):
    """A: one entry in each of the rows `live`, naming one of `nb` B rows at random; B row k holds lengths[k % len(lengths)] random columns.  A row's products
    are its entries: ub = ent = the length of its B row, and T(i,:) = mult(A(i,k), B(k,:)) in closed form."""
    rng = np.random.default_rng(seed)
    B = _Rows(); B.add([])
    for k in range(nb): B.add(pick(rng, ncols, int(lengths[k % len(lengths)])))
    Bp = B.pattern(ncols)
    live = np.asarray(live, np.int64); k = rng.integers(1, nb + 1, len(live))
    Ap = Pattern(nrows, Bp.nrows, {int(i): [int(kk)] for i, kk in zip(live, k)})
    ub = np.zeros(nrows, np.int64); ub[live] = Bp.lens[k]
    return Case(Ap, Bp, ub, ub.copy(), live=live)


@functools.lru_cache(maxsize=None)
def dead_teams(n):
    """The first bin holds n rows (1, 3, 4, 5: a workgroup of four one-wave teams with three, one, no and three dead teams), nothing else has products."""
    return single_entry_rows(30 + n, 70, np.arange(n) * 9 + 2, 5000, [1, 7, 128, 40, 127], nb=10)


GRID_KINDS = {0: (TEAMS_BIN0, [1, 2, 3, 17, 128], 3000), 1: (1, [129], 3000), 2: (1, [1025], 3000), 3: (1, [4097], 6000)}      # bin: (rows per workgroup, B row lengths, columns)


@functools.lru_cache(maxsize=None)
def grid_rounds(b, cus):
    """Bin `b` (symbolic) holds one row more than a grid round of its table kernel takes: rows per workgroup x 32 workgroups per CU x `cus` + 1.  The rows sit
    on the bin's lower edge (129, 1025, 4097 products); every 97th row of the matrix is empty."""
    per, lengths, nc = GRID_KINDS[b]; n = per * GRID_CAP_PER_CU * cus + 1
    rows = np.arange(n + n // 96 + 2); live = rows[rows % 97 != 0][:n]
    assert len(live) == n
    return single_entry_rows(40 + b, int(live[-1]) + 4, live, nc, lengths)


TALL_ROWS = BIN_THREADS + 65


@functools.lru_cache(maxsize=None)
def tall():
    """8192 * 256 + 65 rows: the binning and counting kernels go round twice; the second round is one full wave and one lane.  Non-empty rows at the start, in the
    middle, on both sides of the round's end, in the last full wave and the very last row, with B rows of every bin of every mode."""
    T = BIN_THREADS
    live = np.array([0, 1, 63, 64, 255, 256, 65535, 65536, 1 << 20, T - 257, T - 256, T - 65, T - 64, T - 2, T - 1, T, T + 1, T + 31, T + 62, T + 63, T + 64])
    assert live[-1] == TALL_ROWS - 1
    return single_entry_rows(50, TALL_ROWS, live, 30000, [1, 128, 129, 1024, 1025, 4096, 4097, 16384, 16385, 3], nb=20)


# ---- (e) column width --------------------------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3) + tuple((1 << k) + d for k in (8, 16, 20, 31) for d in (0, 1)) + (DIM_MAX,)
WIDTH_ROWS = 70


@functools.lru_cache(maxsize=None)
def widths(ncols):
    """Row 5 of T holds columns 0, ncols - 1 and 2^m - 1, 2^m for every m with 2^m < ncols among 1, 7, 8, 15, 16, 19, 20, 30, 31, from three B rows that share
    them out (and overlap in column 0 and the last one): the segmented sort must look at the top bit of ncols - 1.  Rows 7 and 9 hold one of the B rows each, the
    other rows up to 40 random columns; every row stays inside the first table bin."""
    rng = np.random.default_rng(60 + ncols % 1000)
    special = np.unique([0, ncols - 1] + [c for m in (1, 7, 8, 15, 16, 19, 20, 30, 31) for c in ((1 << m) - 1, 1 << m) if c < ncols])
    B = _Rows(); B.add([])
    three = [B.add(np.unique(np.concatenate((special[q::3], [0, ncols - 1])))) for q in range(3)]
    a = {5: np.array(three), 7: np.array(three[:1]), 9: np.array(three[2:])}
    for r in range(12, 60, 3):
        a[r] = np.array([B.add(pick(rng, ncols, int(rng.integers(1, min(ncols, 40) + 1)))) for _ in range(int(rng.integers(1, 4)))])
    Bp = B.pattern(ncols); Ap = Pattern(WIDTH_ROWS, Bp.nrows, a)
    return Case(Ap, Bp, products_of(Ap, Bp), entries_of(Ap, Bp), special=special, row=5)


# ---- (f) k_spgemm_dense ----------------------------------------------------------------------------------------------------------------------------------------------------------
NATURAL_COLS = (1 << 20) + 1


@functools.lru_cache(maxsize=None)
def dense_natural():
    """2^20 + 1 columns: the HBM accumulators by themselves.  Rows 3, 4 and 40 hold more than 16 384 products and more than 4096 entries (five B rows of 4000 random
    columns each and B row 1: columns 0, 31, 32, 2^20 - 1, 2^20 — the one bit of the last bitmap word — and ncols - 2); the others stay in the tables."""
    rng = np.random.default_rng(70); nc = NATURAL_COLS
    B = _Rows(); B.add([]); sp = B.add(np.unique([0, 31, 32, (1 << 20) - 1, 1 << 20, nc - 2]))
    big = [B.add(np.union1d(pick(rng, nc, 4000), [31, 1 << 20] if k % 2 else [32])) for k in range(8)]
    a = {3: np.sort([sp] + big[:5]), 4: np.sort([sp] + big[2:7]), 40: np.sort([sp] + big[3:8])}
    for r in range(10, 70, 4):
        if r != 40: a[r] = np.array([B.add(pick(rng, nc, int(rng.integers(1, 3000))))])
    Bp = B.pattern(nc); Ap = Pattern(72, Bp.nrows, a)
    return Case(Ap, Bp, products_of(Ap, Bp), entries_of(Ap, Bp), beyond=(3, 4, 40), special=Bp.cols(sp))


PERSIST_COLS = 20000


@functools.lru_cache(maxsize=None)
def dense_persist(cus):
    """2 * cus + 3 rows of more than 16 384 products each for the 2 * cus persistent workgroups of k_spgemm_dense: three of them (whichever the binning's atomics
    choose) walk a second row.  An A row names two of twelve B rows of 8200 to 8400 of the 20 000 columns: any two rows of T share thousands of columns, with
    other values."""
    rng = np.random.default_rng(71); nc = PERSIST_COLS
    B = _Rows(); B.add([])
    big = [B.add(pick(rng, nc, int(rng.integers(8200, 8400)))) for _ in range(12)]
    n = 2 * cus + 3
    a = {2 + r: np.sort(rng.choice(big, size=2, replace=False)) for r in range(n)}
    Bp = B.pattern(nc); Ap = Pattern(n + 4, Bp.nrows, a)
    return Case(Ap, Bp, products_of(Ap, Bp), entries_of(Ap, Bp), n=n)


# ---- (g) the LDS dense path at its block edges ----------------------------------------------------------------------------------------------------------------------------------
def block_widths(wd):
    return (wd, wd + 1, 2 * wd, 2 * wd - 1)


@functools.lru_cache(maxsize=None)
def lds_blocks(ncols, wd):
    """Rows beyond the tables of every mode (more than 4096 products and entries) over blocks of `wd` columns.  B rows: `low` — 2600 columns of block 0 that end
    on its last column wd - 1; `high` — up to 2600 columns of block 1 that begin on its first column wd (none when ncols = wd; the single column wd when ncols =
    wd + 1); `span` — both sides with wd - 1 and wd.  A rows: 3 low-only (block 1 holds nothing of the row), 4 high-only (block 0 holds nothing), 5 and 6 mixed;
    rows 20 .. 60 hold a few products."""
    rng = np.random.default_rng(80 + ncols % 997); hi_n = min(2600, ncols - wd)
    B = _Rows(); B.add([])
    low = [B.add(np.union1d(pick(rng, wd - 1, 2599), [wd - 1])) for _ in range(4)]
    high = [B.add(np.union1d(wd + pick(rng, ncols - wd, hi_n), [wd])) for _ in range(4)] if hi_n else []
    span = [B.add(np.union1d(pick(rng, ncols, 2600), [wd - 1] + ([wd] if hi_n else []))) for _ in range(3)]
    a = {3: np.sort(low[:3]), 5: np.sort(low[1:] + high[:2] + span[:1]), 6: np.sort(span + low[:1])}
    if high: a[4] = np.sort(high)
    for r in range(20, 61, 5): a[r] = np.array([B.add(pick(rng, ncols, int(rng.integers(1, 900))))])
    Bp = B.pattern(ncols); Ap = Pattern(70, Bp.nrows, a)
    return Case(Ap, Bp, products_of(Ap, Bp), entries_of(Ap, Bp), low_only=3, high_only=4 if high else None, mixed=(5, 6))
