"""Positional semirings on the device (pygraphblas_amd/csrc/grb_possr.hip): GxB_{MIN,MAX,ANY,PLUS,TIMES}_{FIRSTI..SECONDJ1}_{INT32,INT64} in mxv, vxm and mxm.

The oracle has no positional operators: the expected values come from the brute-force model below — dense presence arrays of the operands AFTER the descriptor's
transposes, the term (i, k, j) exists where A(i,k) and B(k,j) do, its value is the coordinate the multiplier names (u is an n x 1 column in mxv, u' a 1 x n row
in vxm), and the monoid folds the terms in numpy integer arithmetic of the type's width (PLUS and TIMES wrap).  An entry exists iff a term does.  For ANY the
pattern must be the model's and every value the coordinate of some contributing term.

Shapes: the rows kernel on 70 x 300 with row lengths 0, 1, 63, 64, 65, 200 (the lane stride and the wave tree) and a row of five odd columns whose product
overflows INT32 without becoming 0; the product kernel on 40 x 130 times 130 x 160 with one output row of > 128 entries (accumulators in global memory) among
shorter ones (LDS) and rows of B whose 20-column supports shift by one from k to k + 1; 4 096 x 4 096 against the POSITIONI workaround, several workgroups per
slot of the grid-stride loop.  Known gap: the INT32 wrap of coordinates >= 2^31 is out of reach at these sizes."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ADDS = ["MIN", "MAX", "ANY", "PLUS", "TIMES"]
MULS = ["FIRSTI", "FIRSTI1", "FIRSTJ", "FIRSTJ1", "SECONDI", "SECONDI1", "SECONDJ", "SECONDJ1"]
NPT = {"INT32": np.int32, "INT64": np.int64, "INT8": np.int8, "FP64": np.float64, "BOOL": np.bool_}
ALL = list(itertools.product(ADDS, MULS, ["INT32", "INT64"]))


# ---- the model --------------------------------------------------------------------------------------------------------------------------------------------------
def term_values(mul, kind, m, kk, n, npt):
    """coord(i, k, j) of every possible term as an (m, kk, n) array of the semiring's type."""
    base, one = mul.rstrip("1"), int(mul.endswith("1"))
    i, k, j = np.arange(m, dtype=np.int64)[:, None, None], np.arange(kk, dtype=np.int64)[None, :, None], np.arange(n, dtype=np.int64)[None, None, :]
    zero = np.zeros((1, 1, 1), np.int64)
    if base == "FIRSTI":
        v = zero if kind == "vxm" else i
    elif base in ("FIRSTJ", "SECONDI"):
        v = k
    else:
        v = zero if kind == "mxv" else j
    return np.broadcast_to((v + one).astype(npt), (m, kk, n))


def model(PA, PB, add, mul, t, kind):
    """(pattern (m, n) bool, values (m, n) of the type — meaningless where the pattern is False; for ANY: the (m, kk, n) terms and their values instead)."""
    npt = NPT[t]
    H = PA[:, :, None] & PB[None, :, :]
    V = term_values(mul, kind, PA.shape[0], PA.shape[1], PB.shape[1], npt)
    pat = H.any(axis=1)
    info = np.iinfo(npt)
    if add == "MIN":
        val = np.where(H, V, info.max).min(axis=1)
    elif add == "MAX":
        val = np.where(H, V, info.min).max(axis=1)
    elif add == "PLUS":
        val = np.where(H, V, 0).sum(axis=1, dtype=npt)              # numpy integer sums wrap at the type's width
    elif add == "TIMES":
        val = np.where(H, V, 1).prod(axis=1, dtype=npt)             # ... and so do products
    else:
        return pat, (H, V)
    return pat, val.astype(npt)


def check(add, got_pat, got_val, pat, val, what):
    """got_pat / got_val: dense (m, n) arrays of the result."""
    assert np.array_equal(got_pat, pat), (what, "pattern")
    if add == "ANY":
        H, V = val
        ok = (H & (V == got_val[:, None, :])).any(axis=1)           # the value is the coordinate of some contributing term
        assert ok[pat].all(), (what, "ANY value is no term's coordinate")
    else:
        assert np.array_equal(got_val[pat], val[pat]), (what, got_val[pat][:8], val[pat][:8])


def dense_vec(w, n, npt):
    idx, x = w.to_arrays()
    p, v = np.zeros(n, bool), np.zeros(n, npt)
    p[idx.astype(np.int64)] = True
    v[idx.astype(np.int64)] = x
    return p, v


def dense_mat(Cm, m, n, npt):
    i, j, x = Cm.to_arrays()
    p, v = np.zeros((m, n), bool), np.zeros((m, n), npt)
    p[i.astype(np.int64), j.astype(np.int64)] = True
    v[i.astype(np.int64), j.astype(np.int64)] = x
    return p, v


def mat_from_pattern(gb, P, typ, rng):
    i, j = np.nonzero(P)
    if typ == "BOOL":
        x = rng.integers(0, 2, len(i)).astype(np.bool_)              # false values are entries too: the values are never read
    elif typ == "FP64":
        x = rng.standard_normal(len(i))
    else:
        x = rng.integers(-100, 100, len(i)).astype(NPT[typ])
    return gb.Matrix.from_arrays(i.astype(np.uint64), j.astype(np.uint64), x, P.shape[0], P.shape[1], getattr(gb, typ))


def vec_from_pattern(gb, p, typ, rng):
    idx = np.nonzero(p)[0]
    x = rng.integers(0, 2, len(idx)).astype(np.bool_) if typ == "BOOL" else rng.integers(-5, 5, len(idx)).astype(NPT[typ])
    return gb.Vector.from_arrays(idx.astype(np.uint64), x, len(p), getattr(gb, typ))


# ---- the rows kernel --------------------------------------------------------------------------------------------------------------------------------------------
ROWS, COLS = 70, 300
LONG_ROW, ODD_ROW = 5, 6


def rows_pattern(rng):
    P = np.zeros((ROWS, COLS), bool)
    lengths = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, LONG_ROW: 200}
    for r in range(ROWS):
        if r == ODD_ROW:
            P[r, [255, 257, 259, 261, 263]] = True                   # 255 * 257 * 259 * 261 * 263 > 2^31 and odd: wraps in INT32, never to 0
            continue
        ln = lengths.get(r, int(rng.integers(2, 120)))
        P[r, rng.choice(COLS, size=ln, replace=False)] = True
    assert P[0].sum() == 0 and P[LONG_ROW].sum() == 200
    return P


@pytest.fixture(scope="module")
def rows_case():
    """The pattern, the operand patterns per orientation and the model's answers: computed once, shared by the three matrix types, never modified."""
    rng = np.random.default_rng(11)
    P = rows_pattern(rng)
    last = int(np.nonzero(P[LONG_ROW])[0][-1])                        # the LAST entry of the 200-entry row
    us = {}
    for n in (ROWS, COLS):
        half = rng.random(n) < 0.5
        single = np.zeros(n, bool)
        single[last if n == COLS else LONG_ROW] = True
        us[n] = {"half": half, "single": single, "full": np.ones(n, bool), "empty": np.zeros(n, bool)}
    # orientation -> (kind, desc name, op(A) as the model's matrix operand, size of u)
    orient = {"mxv": ("mxv", None, P, COLS), "mxv_T0": ("mxv", "T0", P.T, ROWS), "vxm": ("vxm", None, P, ROWS), "vxm_T1": ("vxm", "T1", P.T, COLS)}
    expect = {}
    for oname, (kind, _d, M, un) in orient.items():
        for uname, up in us[un].items():
            for add, mul, t in ALL:
                if kind == "mxv":
                    pat, val = model(M, up[:, None], add, mul, t, kind)
                    expect[(oname, uname, add, mul, t)] = (pat[:, 0], val, 0)
                else:
                    pat, val = model(up[None, :], M, add, mul, t, kind)
                    expect[(oname, uname, add, mul, t)] = (pat[0, :], val, 1)
    return P, us, orient, expect


@pytest.mark.parametrize("atype", ["FP64", "BOOL", "INT8"])
def test_rows_kernel_every_semiring_every_orientation(gb, gpu, rows_case, atype):
    P, us, orient, expect = rows_case
    rng = np.random.default_rng(3)
    A = mat_from_pattern(gb, P, atype, rng)
    D = gb.descriptor
    seen_plans = set()
    for oname, (kind, dname, M, un) in orient.items():
        desc = getattr(D, dname) if dname else None
        nout = M.shape[0] if kind == "mxv" else M.shape[1]
        for uname, up in us[un].items():
            u = vec_from_pattern(gb, up, atype, rng)
            for add, mul, t in ALL:
                sr = getattr(getattr(gb, t), f"{add}_{mul}")
                w = A.mxv(u, sr, desc=desc) if kind == "mxv" else u.vxm(A, sr, desc=desc)
                assert w.type is getattr(gb, t) and w.size == nout
                plan = gb.last_kernel_plan()
                assert plan.startswith(f"possr<add={add},mul={mul},type={t},kind={kind}>") and "k_possr_rows" in plan, plan
                seen_plans.add(plan)
                gp, gv = dense_vec(w, nout, NPT[t])
                pat, val, axis = expect[(oname, uname, add, mul, t)]
                what = (atype, oname, uname, add, mul, t)
                if axis == 0:
                    check(add, gp[:, None], gv[:, None], pat[:, None], val, what)
                else:
                    check(add, gp[None, :], gv[None, :], pat[None, :], val, what)
    assert len(seen_plans) == 80 * 2


def test_rows_kernel_results_do_not_depend_on_the_operands_types(gb, gpu, rows_case):
    """FP64, BOOL and INT8 operands of one pattern: identical results, ANY included (the lowest lane of the first stride with a term: reproducible)."""
    P, us, _orient, _expect = rows_case
    rng = np.random.default_rng(4)
    results = []
    for atype in ("FP64", "BOOL", "INT8"):
        A = mat_from_pattern(gb, P, atype, rng)
        u300, u70 = vec_from_pattern(gb, us[COLS]["half"], atype, rng), vec_from_pattern(gb, us[ROWS]["half"], atype, rng)
        out = []
        for add, mul, t in ALL:
            sr = getattr(getattr(gb, t), f"{add}_{mul}")
            for w in (A.mxv(u300, sr), u70.vxm(A, sr)):
                idx, x = w.to_arrays()
                out.append((idx.tobytes(), x.tobytes()))
        results.append(out)
    assert results[0] == results[1] == results[2]


def test_overflow_row_wraps_in_int32(gb, gpu, rows_case):
    P, _us, _orient, _expect = rows_case
    A = mat_from_pattern(gb, P, "FP64", np.random.default_rng(5))
    u = gb.Vector.from_arrays(np.arange(COLS, dtype=np.uint64), np.ones(COLS), COLS, gb.FP64)
    exact = 255 * 257 * 259 * 261 * 263
    assert exact > 2 ** 31
    w32, w64 = A.mxv(u, gb.INT32.TIMES_SECONDI), A.mxv(u, gb.INT64.TIMES_SECONDI)
    assert w64[ODD_ROW] == exact and w32[ODD_ROW] == int(np.int64(exact).astype(np.int32)) and w32[ODD_ROW] != 0


# ---- masks and the write-back -------------------------------------------------------------------------------------------------------------------------------------
def write_back_model(c_pat, c_val, t_pat, t_val, allow, accum, replace, out_npt):
    """C<M, replace> = accum(C, T) on dense arrays; T in the semiring's type, C and the result in out_npt; accum in out_npt's arithmetic (its operator is of that type)."""
    tc = t_val.astype(out_npt)                                        # the C cast of the write-back
    if accum is None:
        z_pat, z_val = t_pat, tc
    else:
        both = c_pat & t_pat
        with np.errstate(over="ignore"):
            comb = (c_val + tc).astype(out_npt) if accum == "PLUS" else np.minimum(c_val, tc)
        z_pat = c_pat | t_pat
        z_val = np.where(both, comb, np.where(c_pat, c_val, tc))
    keep_pat = np.zeros_like(c_pat) if replace else c_pat
    out_pat = np.where(allow, z_pat, keep_pat)
    out_val = np.where(allow, z_val, c_val)
    return out_pat, out_val


def mask_forms(D):
    # (name, descriptor, uses the mask, structural, complemented, replace)
    return [("none", None, False, False, False, False), ("valued", None, True, False, False, False), ("structural", D.S, True, True, False, False),
            ("complemented", D.C, True, False, True, False), ("complemented_replace", D.RC, True, False, True, True)]


@pytest.mark.parametrize("srname,t", [("MIN_SECONDI1", "INT64"), ("PLUS_FIRSTJ", "INT32")])
@pytest.mark.parametrize("out_t", ["FP64", "INT8"])
def test_masks_accumulators_and_the_cast_of_the_write_back(gb, gpu, rows_case, srname, t, out_t):
    P, us, _orient, _expect = rows_case
    rng = np.random.default_rng(21)
    add, mul = srname.split("_")
    sr = getattr(getattr(gb, t), srname)
    OT, onpt = getattr(gb, out_t), NPT[out_t]
    A = mat_from_pattern(gb, P, "FP64", rng)
    D = gb.descriptor
    for kind, n_out, up in (("mxv", ROWS, us[COLS]["half"]), ("vxm", COLS, us[ROWS]["half"])):
        u = vec_from_pattern(gb, up, "INT8", rng)
        if kind == "mxv":
            t_pat, t_val = model(P, up[:, None], add, mul, t, kind)
            t_pat, t_val = t_pat[:, 0], t_val[:, 0]
        else:
            t_pat, t_val = model(up[None, :], P, add, mul, t, kind)
            t_pat, t_val = t_pat[0], t_val[0]
        m_pat = rng.random(n_out) < 0.6
        m_val = np.where(rng.random(n_out) < 0.5, 0, 3).astype(np.int8)          # present-but-false entries: the valued and the structural mask differ
        c_pat = rng.random(n_out) < 0.4
        c_val = rng.integers(-50, 50, n_out).astype(onpt)
        midx, cidx = np.nonzero(m_pat)[0], np.nonzero(c_pat)[0]
        Mv = gb.Vector.from_arrays(midx.astype(np.uint64), m_val[midx], n_out, gb.INT8)
        for (fname, desc, use_mask, structural, comp, replace), accum in itertools.product(mask_forms(D), (None, "PLUS", "MIN")):
            w = gb.Vector.from_arrays(cidx.astype(np.uint64), c_val[cidx], n_out, OT)
            acc = getattr(OT, accum) if accum else None
            kw = dict(out=w, mask=Mv if use_mask else None, accum=acc, desc=desc)
            if kind == "mxv":
                A.mxv(u, sr, **kw)
            else:
                u.vxm(A, sr, **kw)
            allow = np.ones(n_out, bool)
            if use_mask:
                allow = m_pat if structural else (m_pat & (m_val != 0))
                allow = ~allow if comp else allow
            e_pat, e_val = write_back_model(c_pat, c_val, t_pat, t_val, allow, accum, replace, onpt)
            g_pat, g_val = dense_vec(w, n_out, onpt)
            what = (kind, srname, out_t, fname, accum)
            assert np.array_equal(g_pat, e_pat), what
            assert np.array_equal(g_val[e_pat], e_val[e_pat]), (what, g_val[e_pat][:8], e_val[e_pat][:8])


# ---- the product kernel -------------------------------------------------------------------------------------------------------------------------------------------
PM, PK_, PN = 40, 130, 160
BIG_ROW = 7


def product_patterns(rng):
    """A 40 x 130, B 130 x 160.  Row 7 of A holds columns 5..124; row k of B for those k holds the 20 consecutive columns k .. k + 19, its support shifted by one
    column from one k to the next, so in output row 7 the same column is written by one lane at k and by its neighbour at k + 1; that row has the 139 columns
    5..143 (> 128: accumulators in global memory).  Every other row of A has 0..12 entries and reaches < 128 columns."""
    PA, PB = np.zeros((PM, PK_), bool), np.zeros((PK_, PN), bool)
    for i in range(PM):
        if i == BIG_ROW:
            PA[i, 5:125] = True
        elif i != 9:
            PA[i, rng.choice(PK_, size=int(rng.integers(0, 13)), replace=False)] = True
    for k in range(PK_):
        if 5 <= k < 125:
            PB[k, k:k + 20] = True
        else:
            PB[k, rng.choice(PN, size=int(rng.integers(0, 9)), replace=False)] = True
    return PA, PB


@pytest.fixture(scope="module")
def product_case():
    rng = np.random.default_rng(12)
    PA, PB = product_patterns(rng)
    H = PA[:, :, None] & PB[None, :, :]
    lens = H.any(axis=1).sum(axis=1)
    assert lens[BIG_ROW] > 128 and (np.delete(lens, BIG_ROW) <= 128).all() and (lens == 0).any()
    expect = {(add, mul, t): model(PA, PB, add, mul, t, "mxm") for add, mul, t in ALL}
    m_pat = rng.random((PM, PN)) < 0.5
    m_pat[BIG_ROW, :140] = True                                       # the masked long row stays beyond the LDS capacity
    return PA, PB, expect, m_pat


def test_product_kernel_every_semiring(gb, gpu, product_case):
    PA, PB, expect, m_pat = product_case
    rng = np.random.default_rng(6)
    A, B = mat_from_pattern(gb, PA, "FP64", rng), mat_from_pattern(gb, PB, "INT8", rng)
    At, Bt = mat_from_pattern(gb, PA.T.copy(), "BOOL", rng), mat_from_pattern(gb, PB.T.copy(), "FP64", rng)
    M = mat_from_pattern(gb, m_pat, "FP64", rng)                      # (standard normal values: all true)
    D = gb.descriptor
    variants = [("unmasked", A, B, None, None, None), ("mask", A, B, M, None, m_pat), ("complemented", A, B, M, D.C, ~m_pat),
                ("T0", At, B, None, D.T0, None), ("T1", A, Bt, None, D.T1, None), ("T0T1_mask", At, Bt, M, D.T0T1, m_pat)]
    kernels = set()
    for add, mul, t in ALL:
        sr = getattr(getattr(gb, t), f"{add}_{mul}")
        pat, val = expect[(add, mul, t)]
        for vname, a, b, mask, desc, allow in variants:
            Cm = a.mxm(b, sr, out=gb.Matrix.sparse(getattr(gb, t), PM, PN), mask=mask, desc=desc)
            plan = gb.last_kernel_plan()
            assert plan.startswith(f"possr<add={add},mul={mul},type={t},kind=mxm>"), plan
            kernels.add(plan.split()[1])
            gp, gv = dense_mat(Cm, PM, PN, NPT[t])
            e_pat = pat if allow is None else pat & allow
            what = (vname, add, mul, t)
            check(add, gp, gv, e_pat, val, what)
    assert kernels == {"k_possr_product", "k_possr_fill"}


# ---- against the workaround, several workgroups per slot of the grid-stride loop -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized_case(gb):
    n = 4096
    rng = np.random.default_rng(7)
    i = np.repeat(np.arange(n, dtype=np.uint64), 16)
    j = rng.integers(0, n, len(i)).astype(np.uint64)
    flat = np.unique(i * np.uint64(n) + j)
    i, j = np.divmod(flat, np.uint64(n))
    A = gb.Matrix.from_arrays(i, j, rng.random(len(i)), n, n, gb.FP64)
    bi = rng.integers(0, n, 30000).astype(np.uint64)
    bj = rng.integers(0, 64, 30000).astype(np.uint64)
    bflat = np.unique(bi * np.uint64(64) + bj)
    bi, bj = np.divmod(bflat, np.uint64(64))
    B = gb.Matrix.from_arrays(bi, bj, rng.random(len(bi)), n, 64, gb.FP64)
    uidx = np.nonzero(rng.random(n) < 0.5)[0].astype(np.uint64)
    u = gb.Vector.from_arrays(uidx, rng.random(len(uidx)), n, gb.FP64)
    u_pos = gb.Vector.from_arrays(uidx, uidx.astype(np.int64), n, gb.INT64)              # u with its own positions as values
    pos = lambda X, op: X.apply(op, out=gb.Matrix.sparse(gb.INT64, X.nrows, X.ncols))      # noqa: E731  (the workaround's copy: an 8-byte index per entry)
    return n, A, B, u, u_pos, pos(A, gb.INT64.POSITIONI), pos(A, gb.INT64.POSITIONJ), pos(B, gb.INT64.POSITIONI)


@pytest.mark.parametrize("add", ["MIN", "MAX", "PLUS"])
def test_equals_the_positioni_workaround_bit_for_bit(gb, gpu, sized_case, add):
    n, A, B, u, u_pos, A_i, A_j, B_i = sized_case
    T = gb.INT64
    second, first = getattr(T, add + "_SECOND"), getattr(T, add + "_FIRST")
    # vxm, u(k) A(k,j): SECONDI is the row index k of A's entry; FIRSTJ the column index k of u' — the position of u's entry
    pairs = [(u.vxm(A, getattr(T, add + "_SECONDI")), u.vxm(A_i, second)), (u.vxm(A, getattr(T, add + "_FIRSTJ")), u_pos.vxm(A, first)),
             # mxm, A(i,k) B(k,j): FIRSTJ is the column index of A's entry, SECONDI the row index of B's
             (A.mxm(B, getattr(T, add + "_FIRSTJ")), A_j.mxm(B, first)), (A.mxm(B, getattr(T, add + "_SECONDI")), A.mxm(B_i, second))]
    for got, want in pairs:
        assert got.nvals == want.nvals and got.nvals > n // 2
        for g, w_ in zip(got.to_arrays(), want.to_arrays()):
            assert g.dtype == w_.dtype and np.array_equal(g, w_)


# ---- BFS parents ------------------------------------------------------------------------------------------------------------------------------------------------
def bfs_graph(rng):
    """300 vertices: the path 0 -> 1 -> ... -> 119, random edges among the first 280, and 20 vertices (280..299) nothing reaches."""
    n = 300
    E = np.zeros((n, n), bool)
    E[np.arange(119), np.arange(1, 120)] = True
    src, dst = rng.integers(0, 280, 500), rng.integers(0, 280, 500)
    E[src, dst] = True
    E[280:, :] = False
    E[:, 280:] = False
    return n, E


def numpy_levels(E, s):
    n = E.shape[0]
    level = np.full(n, -1)
    level[s] = 0
    frontier, d = np.array([s]), 0
    while len(frontier):
        d += 1
        nxt = np.nonzero(E[frontier].any(axis=0) & (level < 0))[0]
        level[nxt] = d
        frontier = nxt
    return level


@pytest.mark.parametrize("add", ["ANY", "MIN"])
def test_bfs_parent_tree(gb, gpu, add):
    rng = np.random.default_rng(7)
    n, E = bfs_graph(rng)
    i, j = np.nonzero(E)
    A = gb.Matrix.from_arrays(i.astype(np.uint64), j.astype(np.uint64), np.ones(len(i), np.bool_), n, n, gb.BOOL)
    sr = getattr(gb.INT64, add + "_SECONDI")
    D = gb.descriptor
    for s in (0, 57):
        level = numpy_levels(E, s)
        p = gb.Vector.from_lists([s], [s], n, gb.INT64)
        q = gb.Vector.from_lists([s], [s], n, gb.INT64)
        for _ in range(n):
            q.vxm(A, sr, out=q, mask=p, desc=D.RSC)               # q<!p, structural, replace> = q (+).secondi A: the parent of every newly reached vertex
            if q.nvals == 0:
                break
            p.assign(q, mask=q, desc=D.S)                          # p<q, structural> = q
        idx, par = p.to_arrays()
        idx, par = idx.astype(np.int64), par.astype(np.int64)
        assert np.array_equal(idx, np.nonzero(level >= 0)[0])      # unreached vertices (the 20 isolated ones among them) have no entry
        assert not (idx >= 280).any() and par[idx == s][0] == s    # the source is its own parent
        for v, pv in zip(idx.tolist(), par.tolist()):
            if v == s:
                continue
            assert level[pv] == level[v] - 1 and E[pv, v], (add, s, v, pv)
            if add == "MIN":
                assert pv == np.nonzero(E[:, v] & (level == level[v] - 1))[0].min(), (s, v, pv)


# ---- refusals that need a device-resident container, and non-blocking mode --------------------------------------------------------------------------------------
def last_error(gb):
    buf = C.create_string_buffer(1024)
    gb.lib.GrBX_last_error(buf, C.c_int(1024))
    return buf.value.decode()


def test_refusals_on_device_resident_containers(gb, gpu):
    lib, DM = gb.lib, gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1, 2, 3], 3, 3, gb.INT64)
    u = gb.Vector.from_lists([0, 1, 2], [1, 2, 3], 3, gb.INT64)
    w = A.mxv(u, gb.INT64.PLUS_TIMES)                                  # lives in HBM
    Cm = A.mxm(A, gb.INT64.PLUS_TIMES)
    before_w, before_c = w.to_lists(), Cm.to_lists()
    w = A.mxv(u, gb.INT64.PLUS_TIMES); Cm = A.mxm(A, gb.INT64.PLUS_TIMES)
    sr = C.c_void_p(gb.INT64.MIN_SECONDI.get_op())
    mul = C.c_void_p()
    assert lib.GxB_Semiring_multiply(C.byref(mul), sr) == 0
    calls = [("accum of mxv", lambda: lib.GrB_mxv(w._h, None, mul, sr, A._h, u._h, None), "GxB_SECONDI_INT64"),
             ("accum of a built-in product", lambda: lib.GrB_mxv(w._h, None, mul, C.c_void_p(gb.INT64.PLUS_TIMES.get_op()), A._h, u._h, None), "GxB_SECONDI_INT64"),
             ("accum of mxm", lambda: lib.GrB_mxm(Cm._h, None, mul, sr, A._h, A._h, None), "GxB_SECONDI_INT64"),
             ("eWiseAdd", lambda: lib.GrB_Vector_eWiseAdd_Semiring(w._h, None, None, sr, w._h, u._h, None), "GxB_MIN_SECONDI_INT64"),
             ("eWiseMult", lambda: lib.GrB_Matrix_eWiseMult_Semiring(Cm._h, None, None, sr, Cm._h, A._h, None), "GxB_MIN_SECONDI_INT64"),
             ("multiplier in eWiseMult", lambda: lib.GrB_Vector_eWiseMult_BinaryOp(w._h, None, None, mul, w._h, u._h, None), "GxB_SECONDI_INT64"),
             ("multiplier in apply", lambda: lib.GxB_Vector_apply_BinaryOp2nd_INT64(w._h, None, None, mul, w._h, C.c_int64(1), None), "GxB_SECONDI_INT64")]
    for what, call, name in calls:
        assert call() == DM and name in last_error(gb), (what, last_error(gb))
    assert w.to_lists() == before_w and Cm.to_lists() == before_c
    with pytest.raises(gb.DimensionMismatch):                          # dimensions are checked as for every built-in semiring
        A.mxv(gb.Vector.sparse(gb.INT64, 4), gb.INT64.MIN_SECONDI)
    with pytest.raises(gb.DimensionMismatch):
        A.mxm(gb.Matrix.sparse(gb.INT64, 4, 3), gb.INT64.ANY_FIRSTI)


def test_a_pending_chain_on_the_operand_completes_first(gb, gpu):
    """Non-blocking mode: u is the output of queued element-wise work when the product is called; the product is never queued — the chain runs, then it does —
    and the result is the one of an operand that was complete all along."""
    n = 500
    rng = np.random.default_rng(9)
    P = rng.random((n, n)) < 0.03
    A = mat_from_pattern(gb, P, "FP64", rng)
    ia, ib = np.nonzero(rng.random(n) < 0.3)[0].astype(np.uint64), np.nonzero(rng.random(n) < 0.3)[0].astype(np.uint64)
    a = gb.Vector.from_arrays(ia, np.ones(len(ia)), n, gb.FP64)
    b = gb.Vector.from_arrays(ib, np.ones(len(ib)), n, gb.FP64)
    both = np.union1d(ia, ib)
    plain = gb.Vector.from_arrays(both, np.ones(len(both)), n, gb.FP64)
    for srname in ("MIN_SECONDI", "PLUS_FIRSTJ1", "ANY_SECONDJ"):
        sr = getattr(gb.INT64, srname)
        want_v, want_m = plain.vxm(A, sr).to_arrays(), A.mxv(plain, sr).to_arrays()
        stats = [C.c_uint64() for _ in range(4)]
        assert gb.lib.GrBX_lazy_stats(*[C.byref(x) for x in stats]) == 0
        chains0 = stats[0].value
        u = a.eadd(b, gb.FP64.PLUS)                                   # queued
        u = u.emult(u, gb.FP64.TIMES)                                 # ... and a second node on top
        got_v = u.vxm(A, sr)
        assert gb.last_kernel_plan().startswith("possr<")
        assert gb.lib.GrBX_lazy_stats(*[C.byref(x) for x in stats]) == 0 and stats[0].value > chains0      # the chain ran because of the product
        u2 = a.eadd(b, gb.FP64.PLUS)
        got_m = A.mxv(u2, sr)
        for g, w_ in zip(got_v.to_arrays() + got_m.to_arrays(), want_v + want_m):
            assert np.array_equal(g, w_), srname
