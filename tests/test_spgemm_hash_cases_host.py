"""The case builders of tests/spgemm_hash_cases.py (no GPU): every case has the property it exists for — the per-row product and entry counts it claims, the
slots its keys hash to, the group arithmetic of its A rows, the nine bin counts per mode — and the model of the ladder agrees with the oracle."""
import numpy as np
import pytest

from oracle import oracle as O
import matrix_model as MM
import product_model as PM
import spgemm_hash_cases as HC
from test_spgemm_masked_at_size_gpu import values

CUS = 256          # the builders that take a CU count are checked for the MI355X's


def bins_by_hand(ub, ent, mode):
    """k_hash_bin5 and k_hash_bin row by row, as the header writes them."""
    l0, l1, l2, l3 = HC.SYM_LIMITS[mode]; s = [0] * 5; n = [0] * 4
    for w in ub:
        if w: s[0 if w <= l0 else (1 if w <= l1 else (2 if w <= l2 else (3 if w <= l3 else 4)))] += 1
    l0, l1, l2 = HC.NUM_LIMITS[mode]
    for w in ent:
        if w: n[0 if w <= l0 else (1 if w <= l1 else (2 if w <= l2 else 3))] += 1
    return tuple(s) + tuple(n)


def consistent(c, expand=True):
    """What the builder claims is what the patterns give, and `bins` is the header's rule in every mode."""
    assert np.array_equal(c.ub, HC.products_of(c.A, c.B))
    if expand: assert np.array_equal(c.ent, HC.entries_of(c.A, c.B))
    for mode in HC.MODES: assert c.bins(mode) == bins_by_hand(c.ub, c.ent, mode), mode
    assert c.A.ncols == c.B.nrows and c.A.nrows > 64                                 # (more than 64 rows: neither the few-rows nor the batch route)
    assert len(c.B.keys) < c.B.nrows * c.B.ncols and (c.B.lens == 0).any()           # (B is not full: no spmm_full)


def test_the_modes_limits():
    assert HC.SYM_SLOTS == tuple(2 * l for l in HC.SYM_LIMITS["hbm"]) and HC.NUM_SLOTS == tuple(2 * l for l in HC.NUM_LIMITS["hbm"])
    assert HC.bins([0, 1, 128, 129, 1024, 1025, 4096, 4097, 16384, 16385], [0, 1, 128, 129, 1024, 1025, 4096, 4097, 4097, 1], "hbm") == (2, 2, 2, 2, 1, 3, 2, 2, 2)
    assert HC.bins([129, 1025, 4097], [128, 129, 1025], "ranked") == (0, 1, 0, 0, 2, 1, 1, 0, 1)
    assert HC.bins([129, 1025, 4097], [128, 129, 1025], "blocks") == (0, 1, 1, 0, 1, 1, 1, 1, 0)
    assert HC.bins([128, 129, 1025], [128, 129, 1025], "ordered") == (1, 0, 0, 0, 2, 1, 0, 0, 2)
    assert HC.effective_mode("ordered", "FP32", "PLUS", 1000) == "ordered" and HC.effective_mode("ordered", "FP32", "MIN", 1000) == "ranked"
    assert HC.effective_mode("ordered", "INT32", "PLUS", 1000) == "ranked" and HC.effective_mode("ranked", "INT32", "PLUS", (1 << 20) + 1) == "hbm"
    assert HC.effective_mode("blocks", "BOOL", "LOR", 1 << 20) == "blocks"


def test_hash_col_and_its_preimages():
    rng = np.random.default_rng(1)
    for keys in HC.SYM_SLOTS:
        j = rng.integers(0, 1 << 32, 1000)
        assert np.array_equal(HC.hash_col(j, keys), [((int(x) * 2654435761) % (1 << 32) >> 7) & (keys - 1) for x in j])
        p = HC.preimages([5, keys - 1], keys, 1 << 28, rng, 100)
        assert len(p) >= 100 and p.max() < 1 << 28 and np.all(np.diff(p) > 0) and set(HC.hash_col(p, keys).tolist()) == {5, keys - 1}


def test_the_ladder():
    c = HC.ladder(); consistent(c)
    distinct = sorted(p for _, p, k in c.rows if k is None); crowded = {(p, k) for _, p, k in c.rows if k is not None}
    assert distinct == HC.LADDER[1:] and all(c.ub[r] == c.ent[r] == p for r, p, k in c.rows if k is None)
    assert crowded == {(p, k) for p in HC.LADDER for k in HC.CROWD + (HC.CROWD_HIGH if p >= 16384 else ()) if p > k}
    assert all(c.ub[r] == p and c.ent[r] == k for r, p, k in c.rows if k is not None) and {(16384, 1), (16384, 128), (16384, 129)} <= crowded
    assert c.A.lens[0] == 0 and c.A.lens[-1] == 0 and c.B.lens[0] == c.B.lens[1] == 0
    assert c.A.lens[HC.ROW_ONLY_EMPTY_B] == 2 and c.ub[HC.ROW_ONLY_EMPTY_B] == 0 and set(c.A.cols(HC.ROW_ONLY_EMPTY_B)) == {0, 1}
    assert 0 in c.A.cols(HC.ROW_WITH_EMPTY_B) and c.ub[HC.ROW_WITH_EMPTY_B] == 129
    # a row ON every limit of every mode, symbolic and numeric, and the crowded rows in a high symbolic and a low numeric bin
    for lim in (128, 1024, 4096, 16384): assert (c.ub == lim).sum() >= 2 and (c.ub == lim + 1).sum() >= 2 and (c.ub == lim - 1).sum() >= 2
    for lim in (128, 1024, 4096): assert ((c.ent == lim) & (c.ub >= 16384)).any() and ((c.ent == lim + 1) & (c.ub >= 16384)).any()
    assert ((c.ub > 16384) & (c.ent == 1)).any()
    s = c.bins("hbm"); assert all(x > 0 for x in s)
    assert c.bins("ranked")[2:4] == (0, 0) and c.bins("ranked")[7] == 0 and c.bins("ordered")[1:4] == (0, 0, 0) and c.bins("blocks")[3] == 0
    assert int(c.A.lens.max()) * 4 * 64 < 2 ** 24 and c.ub.sum() < 2e6               # exact_sums; the model's cost


def test_the_clustered_keys():
    for slots in HC.SYM_SLOTS:
        c = HC.clustered(slots); consistent(c); n = slots // 2
        assert c.ub[c.wrap] == c.ub[c.slot] == c.ub[c.run] == n == c.n
        h = HC.hash_col(np.concatenate([c.B.cols(k) for k in c.A.cols(c.wrap)]), slots); assert len(h) == n and h.min() >= slots - 8
        cols = np.sort(np.concatenate([c.B.cols(k) for k in c.A.cols(c.slot)]))
        assert len(np.unique(cols)) == n and set(HC.hash_col(cols, slots).tolist()) == {slots - 3}          # one slot: a probe chain of n that wraps
        if slots < 32768:
            d = np.diff(cols); assert np.all(d == c.stride) and c.stride & (c.stride - 1) == 0 and cols[-1] + c.stride > HC.DIM_MAX - 1 and c.stride >= (1 << 7) * slots
        else: assert c.stride == 0 and (1 << 32) // n < (1 << 7) * slots             # (no power-of-two stride reaches 16 384 terms)
        assert np.all(np.diff(np.sort(np.concatenate([c.B.cols(k) for k in c.A.cols(c.run)]))) == 1)
        b = c.bins("hbm"); q = HC.SYM_SLOTS.index(slots)
        assert b[q] >= 4 and b[4] == 0 and (b[5 + q] >= 4 if q < 3 else b[8] == 4)


def test_the_team_shapes():
    c = HC.teams(); consistent(c)
    seen = set()
    for r, (L, way, n) in c.ways.items():
        k = c.A.cols(r); bl = c.B.lens[k]; assert c.ub[r] == L == bl.sum(); seen.add((L, way, n))
        if way == "one long": assert len(k) == 1
        if way == "units": assert len(k) == L and np.all(bl == 1) and c.ent[r] == L
        if way == "entries": assert len(k) == n and np.all(bl > 0)
        if way == "lengths": assert (bl == n).sum() == L // n and len(k) == L // n + (L % n > 0)
    assert seen == {(L, w, n) for L in HC.TEAM_LIMITS for w, ns in (("one long", (1,)), ("units", (L,)), ("entries", HC.TEAM_A_COUNTS), ("lengths", HC.TEAM_B_LENGTHS)) for n in ns}
    assert {g + d for g in set(HC.SYM_GROUPS + HC.NUM_GROUPS) for d in (-1, 0, 1)} == set(HC.TEAM_A_COUNTS)
    assert c.bins("hbm")[:5] == (20, 20, 20, 20, 0)


def test_the_grid_cases():
    for n in (1, 3, 4, 5):
        c = HC.dead_teams(n); consistent(c); assert c.bins("ranked") == (n, 0, 0, 0, 0, n, 0, 0, 0) and n % HC.TEAMS_BIN0 in (0, 1, 3)
    for b, mode in ((0, "ranked"), (1, "ranked"), (2, "blocks"), (3, "hbm")):
        c = HC.grid_rounds(b, CUS); consistent(c, expand=b < 2)
        per = HC.TEAMS_BIN0 if b == 0 else 1
        assert c.bins(mode)[b] == per * HC.GRID_CAP_PER_CU * CUS + 1 and sum(c.bins(mode)[:5]) == c.bins(mode)[b] and c.A.lens.max() == 1
        if b: assert c.ub[c.live].min() == c.ub[c.live].max() == HC.SYM_LIMITS["hbm"][b - 1] + 1
    c = HC.tall(); consistent(c, expand=False)
    T = HC.BIN_THREADS; assert c.A.nrows == T + 65 and c.ub[-1] > 0 and c.ub[T - 1] > 0 and c.ub[T] > 0 and c.ub[T + 63] > 0 and c.ub[0] > 0
    assert all(x > 0 for x in c.bins("hbm")) and len(c.live) < 40


def test_the_widths():
    for nc in HC.WIDTHS:
        c = HC.widths(nc); consistent(c)
        got = np.unique(np.concatenate([c.B.cols(k) for k in c.A.cols(c.row)]))
        assert np.array_equal(got, c.special) and got[0] == 0 and got[-1] == nc - 1
        k = int(np.log2(nc - 1)) if nc > 1 else 0
        if nc > 2: assert (1 << k) - 1 in got and 1 << k in got                       # the top bit of the largest column, and the column below it
        assert c.bins("hbm")[1:5] == (0, 0, 0, 0) and c.bins("hbm")[6:] == (0, 0, 0)
    assert set(HC.WIDTHS) == {1, 2, 3, 256, 257, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 31, (1 << 31) + 1, 0xFFFFFFF0}


def test_the_dense_cases():
    c = HC.dense_natural(); consistent(c)
    assert c.B.ncols == (1 << 20) + 1 and c.bins("hbm")[4] == 3 and c.bins("hbm")[8] == 3 and {31, 32, 1 << 20, c.B.ncols - 2} <= set(c.special.tolist())
    assert all(c.ub[r] > 16384 and c.ent[r] > 4096 for r in c.beyond)
    c = HC.dense_persist(CUS); consistent(c)
    assert c.n == 2 * CUS + 3 and c.bins("hbm")[4] == c.n and c.bins("hbm")[8] == c.n and c.ub.sum() < 1e7
    rows = [np.unique(np.concatenate([c.B.cols(k) for k in c.A.cols(r)])) for r in (2, 3, c.n + 1)]
    assert len(np.intersect1d(rows[0], rows[1])) > 4000 and len(np.intersect1d(rows[1], rows[2])) > 4000


def test_the_block_edges():
    for wd in HC.WD.values():
        for nc in HC.block_widths(wd):
            c = HC.lds_blocks(nc, wd); consistent(c)
            low = np.unique(np.concatenate([c.B.cols(k) for k in c.A.cols(c.low_only)]))
            assert low[-1] == wd - 1 and c.ent[c.low_only] > 4096                   # ends on the block's last column; block 1 holds nothing of it
            assert all(c.B.cols(k)[-1] == wd - 1 for k in c.A.cols(c.low_only))
            if nc > wd:
                high = np.unique(np.concatenate([c.B.cols(k) for k in c.A.cols(c.high_only)])); assert high[0] == wd
                assert all(wd - 1 in np.concatenate([c.B.cols(k) for k in c.A.cols(r)]) and wd in np.concatenate([c.B.cols(k) for k in c.A.cols(r)]) for r in c.mixed)
                if nc > wd + 1: assert c.ent[c.high_only] > 4096
            else: assert c.high_only is None
            assert c.bins("blocks")[4] >= 3 and c.bins("blocks")[8] >= 3 and c.bins("ranked")[4] >= 3


def tuples_of_mat(m):
    return O.Tuples(m.typ, m.nrows, m.ncols, m.rows, m.cols, m.vals)


@pytest.mark.parametrize("typ", ["INT8", "FP32"])
def test_the_ladders_model_agrees_with_the_oracle(typ):
    """product_model.mxm on the ladder against oracle/grb_oracle.c: PLUS_TIMES (INT8 wraps; FP32 sums of up to 20 000 terms are exact), the monoid without a
    native atomic, and PLUS_SECOND."""
    c = HC.ladder(); rng = np.random.default_rng(5)
    A, B = c.A.mat(values(rng, typ, len(c.A.keys))), c.B.mat(values(rng, typ, len(c.B.keys)))
    for sr in ("PLUS_TIMES", PM.mxm_semirings(typ)[3], "PLUS_SECOND"):
        add, mul = sr.split("_")
        got = PM.mxm(MM.empty(A.nrows, B.ncols, typ), A, B, add, mul, typ)
        exp = O.mxm(O.Tuples(typ, A.nrows, B.ncols), tuples_of_mat(A), tuples_of_mat(B), add, mul, typ).sorted()
        assert np.array_equal(got.rows, exp.I.astype(np.int64)) and np.array_equal(got.cols, exp.J.astype(np.int64)), sr
        assert np.array_equal(got.vals, exp.X), sr
        assert np.array_equal(np.bincount(got.rows, minlength=A.nrows), c.ent), sr
