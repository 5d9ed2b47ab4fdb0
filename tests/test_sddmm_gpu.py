"""The masked product of two full matrices (the sddmm route of GrB_mxm: grb_sddmm.hip, grb_sddmm_kernels.hpp) against the numpy model of tests/product_model.py —
`PM.mxm(..., mask=...)`, which is pinned to the oracle — BIT FOR BIT on `to_csr()` (row pointers, columns, values).

Every edge is read from GrBX_sddmm_geometry: TILE = mask entries per workgroup, WAVES and CAP = waves per workgroup and the grid cap, MINW = the work m k n from
which the route is taken by itself.  Floating-point values lie on the 1/8 grid without zeros and are small enough that every summation order is exact (the route's
order is a butterfly, not the oracle's left to right); the narrow integer types carry their extremes (they wrap, in any order alike).  Cases run with
GRB_MI355X_SDDMM=1 unless they are about the default rule, and every routed case asserts the plan string — `sddmm<k=K,group=G,entries=E,...` with the values the
case was built for — so that a case that went another way fails instead of passing.  X is m x k, Y is n x k, the mask m x n; unless a case says otherwise the call
is `X.mxm(Y, mask=M, desc=ST1)`: Y is read as it lies.

The last section is about rounding: normal random values, where the order matters."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import matrix_model as MM
import product_model as PM
import pygraphblas_amd as gb
from helpers import TYPE
from test_matrix_kernels_at_size_gpu import check, desc_of
from test_spmm_full_gpu import values, sparse, full, up, up_full, pow2ceil
from test_sddmm_host import default_rule_shapes

pytestmark = pytest.mark.gpu
NP = MM.NP
REAL = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]


@functools.lru_cache(maxsize=None)
def geometry():
    out = (C.c_uint64 * 4)()
    assert gb.lib.GrBX_sddmm_geometry(out) == 0
    return tuple(int(v) for v in out)              # TILE, WAVES, CAP, MINW


@pytest.fixture(autouse=True)
def route_hook(gpu, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_SDDMM", "1")
    for name in ("GRB_MI355X_FULL", "GRB_MI355X_DETERMINISTIC", "GRB_MI355X_SPGEMM", "GRB_MI355X_MXM_ROWS", "GRB_MI355X_BATCH"):
        monkeypatch.delenv(name, raising=False)


PLAN = re.compile(r"^sddmm<k=(\d+),group=(\d+),entries=(\d+),cast=([01])> ")


def assert_route(k, entries, cast=None, what=""):
    plan = gb.last_kernel_plan() + " "
    m = PLAN.match(plan)
    assert m, f"{what}: not on the sddmm route: {plan}"
    got = tuple(int(v) for v in m.groups())
    assert got[:3] == (k, pow2ceil(min(k, 64)), entries), f"{what}: {plan}"
    assert ("k_sddmm " in plan) == (entries > 0), plan
    if cast is not None:
        assert got[3] == int(cast), plan


def off_route(what):
    plan = gb.last_kernel_plan()
    assert "sddmm<" not in plan, f"{what}: {plan}"


def mask_of(rng, lens, ncols, typ="BOOL", all_true=False):
    M = sparse(rng, lens, ncols, typ)
    if all_true:
        M = MM.Mat(M.nrows, M.ncols, M.keys, np.ones(M.nvals, NP[typ]))
    return M


def product(A, B, M, sr, typ, dA=None, dB=None, dM=None, C=None, dC=None, struct=True, comp=False, replace=False, accum=None, t0=False, t1=True, routed=True, cast=None, what=""):
    """dA.mxm(dB, mask=dM) into dC (a fresh matrix of the semiring's type when not given) against the model; `accum` = (operator, type).  A is op(A)'s operand as
    the call gets it (k x m under t0), B likewise (n x k under t1).  `routed`: assert the route, with the entry count of the mask's whole pattern."""
    add, mul = sr.split("_")
    dA = up_full(A) if dA is None else dA; dB = up_full(B) if dB is None else dB
    opA = MM.transpose(A) if t0 else A; opB = MM.transpose(B) if t1 else B
    if C is None:
        C = MM.empty(opA.nrows, opB.ncols, typ)
    if dC is None:
        dC = up(C)
    if dM is None:
        dM = up(M)
    exp = PM.mxm(C, A, B, add, mul, typ, mask=M, struct=struct, comp=comp, replace=replace, accum=accum, tran_a=t0, tran_b=t1)
    dA.mxm(dB, semiring=getattr(TYPE[typ], sr), mask=dM, out=dC, accum=getattr(TYPE[accum[1]], accum[0]) if accum else None, desc=desc_of(replace, struct, comp, t0, t1))
    what = f"{what} {typ}.{sr} k={opA.ncols}"
    if routed:
        assert_route(opA.ncols, M.nvals, cast, what)
    check(dC, exp, what)
    return dC, exp


# ---- k edges: every group width, the first k with two trips, three trips, a ragged last trip ------------------------------------------------------------------------
K_EDGES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257]
MORE = ["MIN_PLUS", "MAX_MIN", "ANY_PAIR", "PLUS_PAIR", "PLUS_FIRST", "PLUS_SECOND"]


def k_cases():
    out = [(t, "LOR_LAND" if t == "BOOL" else "PLUS_TIMES") for t in REAL]
    return out + [(t, s) for t in ("INT64", "FP32", "FP64") for s in MORE]


@functools.lru_cache(maxsize=None)
def k_mask():
    rng = np.random.default_rng(41)
    lens = [int(x) for x in rng.integers(0, 6, 203)]; lens[0] = 0; lens[100] = 0; lens[-1] = 0
    return mask_of(rng, lens, 197)


@pytest.mark.parametrize("k", K_EDGES)
@pytest.mark.parametrize("typ,sr", k_cases())
def test_k_edges(typ, sr, k):
    M = k_mask()
    rng = np.random.default_rng(k * 131 + sum(map(ord, typ + sr)))
    X = full(rng, M.nrows, k, typ); Y = full(rng, M.ncols, k, typ)
    product(X, Y, M, sr, typ, cast=False, what="k edges")


# ---- mask shapes ---------------------------------------------------------------------------------------------------------------------------------------------
def shape_lens(shape):
    """(row lengths, columns) of the mask"""
    TILE = geometry()[0]
    n = 2 * TILE + 40
    return {
        "empty_rows": ([0, 0, 0, 5, 1, 0, 0, 0, 0, 7, TILE // 2, 0, 3, 0, 0, 0], n),
        "hub": ([2, 0, 2 * TILE + 9, 1, 3, 0], n),
        "tile-1": ([TILE // 2, 0, TILE // 2 - 1], n),
        "tile": ([TILE // 2, 0, TILE // 2], n),
        "tile+1": ([TILE // 2, 0, TILE // 2, 1], n),
        "row_on_tile_boundary": ([TILE - 3, 3, 0, 2, TILE - 2, 5], n),          # the second and the fifth row end where a tile ends
        "one": ([0, 0, 1, 0], 9),
        "none": ([0, 0, 0], 9),
        "full": ([23] * 19, 23),
    }[shape]


@pytest.mark.parametrize("k", [1, 5, 70])
@pytest.mark.parametrize("shape", ["empty_rows", "hub", "tile-1", "tile", "tile+1", "row_on_tile_boundary", "one", "none", "full"])
def test_mask_shapes(shape, k):
    TILE = geometry()[0]
    lens, n = shape_lens(shape)
    rng = np.random.default_rng(len(lens) * 7 + k)
    M = mask_of(rng, lens, n)
    assert M.nvals == {"tile-1": TILE - 1, "tile": TILE, "tile+1": TILE + 1, "one": 1, "none": 0, "full": 19 * 23}.get(shape, M.nvals)
    X = full(rng, len(lens), k, "FP32"); Y = full(rng, n, k, "FP32")
    dC, exp = product(X, Y, M, "PLUS_TIMES", "FP32", what=shape)
    assert exp.nvals == M.nvals
    product(X, Y, M, "MIN_PLUS", "FP32", what=shape)
    if shape == "none":                                                          # nothing to compute: C follows the write-back rules
        keys = np.array([1, 5, 20]); Cm = MM.Mat(3, 9, keys, values(rng, "FP32", 3))
        for replace in (False, True):
            dC, exp = product(X, Y, M, "PLUS_TIMES", "FP32", C=Cm, replace=replace, what=f"none over C replace={replace}")
            assert exp.nvals == (0 if replace else 3)


def test_past_one_grid_round():
    """k = 1 (one entry per lane): one entry more than the capped grid takes in one round."""
    TILE, WAVES, CAP, _ = geometry()
    n = 512; rows = CAP * TILE // n; assert rows * n == CAP * TILE
    keys = np.arange(CAP * TILE + 1, dtype=np.int64)                              # `rows` full rows and one entry in the last
    M = MM.Mat(rows + 1, n, keys, np.ones(len(keys), np.bool_))
    rng = np.random.default_rng(5)
    X = full(rng, rows + 1, 1, "INT32"); Y = full(rng, n, 1, "INT32")
    dC, exp = product(X, Y, M, "PLUS_TIMES", "INT32", what="grid round")
    assert exp.nvals == CAP * TILE + 1


# ---- mask semantics ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sem_operands():
    TILE = geometry()[0]
    rng = np.random.default_rng(21)
    m, n, k = 37, TILE + 30, 6
    lens = [int(x) for x in rng.integers(0, 12, m)]; lens[3] = TILE + 5
    return full(rng, m, k, "INT32"), full(rng, n, k, "INT32"), tuple(lens)


def valued_mask(rng, lens, n, typ):
    M = sparse(rng, lens, n, typ)
    vals = rng.choice(np.array([0, 1, 3], NP[typ]), size=M.nvals) if typ != "BOOL" else rng.random(M.nvals) < 0.6
    M = MM.Mat(M.nrows, M.ncols, M.keys, vals.astype(NP[typ]))
    assert (~MM.mask_truth(M.vals)).any() and MM.mask_truth(M.vals).any()
    return M


@pytest.mark.parametrize("mtyp", REAL)
def test_valued_and_structural_masks(mtyp):
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(len(mtyp) + ord(mtyp[0]))
    M = valued_mask(rng, lens, Y.nrows, mtyp)
    dM = up(M)
    dC, exp = product(X, Y, M, "PLUS_TIMES", "INT32", dM=dM, struct=False, what=f"valued {mtyp}")
    assert exp.nvals == int(MM.mask_truth(M.vals).sum()) < M.nvals
    dC, exp = product(X, Y, M, "PLUS_TIMES", "INT32", dM=dM, struct=True, what=f"structural {mtyp}")
    assert exp.nvals == M.nvals


def test_complemented_mask_is_not_routed():
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(8)
    M = valued_mask(rng, lens, Y.nrows, "INT8")
    for struct in (False, True):
        product(X, Y, M, "PLUS_TIMES", "INT32", struct=struct, comp=True, routed=False, what="complemented"); off_route("complemented")


# ---- write-back ----------------------------------------------------------------------------------------------------------------------------------------------
def some_C(rng, m, n, typ, density=0.3):
    keys = np.flatnonzero(rng.random(m * n) < density).astype(np.int64)
    return MM.Mat(m, n, keys, values(rng, typ, len(keys)))


@pytest.mark.parametrize("struct", [True, False])
@pytest.mark.parametrize("replace", [False, True])
def test_replace_over_a_non_empty_C(replace, struct):
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(3)
    M = valued_mask(rng, lens, Y.nrows, "INT16")
    Cm = some_C(rng, X.nrows, Y.nrows, "INT32")
    product(X, Y, M, "PLUS_TIMES", "INT32", C=Cm, struct=struct, replace=replace, what="replace")


@pytest.mark.parametrize("accum", [("PLUS", "INT32"), ("MIN", "INT32"), ("PLUS", "INT64"), ("MIN", "FP64")])
def test_accumulators(accum):
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(4)
    M = valued_mask(rng, lens, Y.nrows, "BOOL")
    for ctyp in ("INT32", accum[1]):
        Cm = some_C(rng, X.nrows, Y.nrows, ctyp)
        for replace in (False, True):
            product(X, Y, M, "PLUS_TIMES", "INT32", C=Cm, struct=True, replace=replace, accum=accum, what=f"accum {accum} C {ctyp}")
    product(X, Y, M, "PLUS_TIMES", "INT32", C=some_C(rng, X.nrows, Y.nrows, "INT32"), struct=False, accum=accum, what=f"accum {accum} valued")


def test_output_is_an_operand():
    rng = np.random.default_rng(6)
    n = 40
    X = full(rng, n, n, "FP64"); Y = full(rng, n, n, "FP64")
    M = mask_of(rng, [int(x) for x in rng.integers(0, 9, n)], n, "FP64", all_true=True)
    dM = up(M)
    product(X, Y, M, "PLUS_TIMES", "FP64", dM=dM, C=M, dC=dM, what="C is M")
    dX = up_full(X)
    product(X, Y, M, "PLUS_TIMES", "FP64", dA=dX, C=X, dC=dX, what="C is X")
    dM = up(M)
    product(X, Y, M, "PLUS_TIMES", "FP64", dM=dM, C=M, dC=dM, accum=("PLUS", "FP64"), what="C is M, accumulated")


# ---- transposes, casts, fullness -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [False, True])
@pytest.mark.parametrize("t1", [False, True])
def test_transposed_operands(t0, t1):
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(7)
    M = mask_of(rng, lens, Y.nrows)
    A = MM.transpose(X) if t0 else X; B = Y if t1 else MM.transpose(Y)
    product(A, B, M, "MIN_PLUS", "INT32", t0=t0, t1=t1, what=f"T0={t0} T1={t1}")


def test_both_operands_one_object():
    rng = np.random.default_rng(9)
    n, k = 50, 7
    X = full(rng, n, k, "INT64"); dX = up_full(X)
    M = mask_of(rng, [int(x) for x in rng.integers(0, 6, n)], n)
    product(X, X, M, "PLUS_TIMES", "INT64", dA=dX, dB=dX, what="X X'")                       # n x n = X X'
    Mk = mask_of(rng, [int(x) for x in rng.integers(0, 6, k)], k)
    product(X, X, Mk, "PLUS_TIMES", "INT64", dA=dX, dB=dX, t0=True, t1=False, what="X' X")     # k x k = X' X
    S = full(rng, n, n, "INT64"); dS = up_full(S)
    product(S, S, M, "PLUS_TIMES", "INT64", dA=dS, dB=dS, t1=False, what="S S")               # no transpose at all: S's cached transpose is read


def test_casts():
    """INT32 operands under an FP64 semiring: both are cast once; PAIR reads neither side; the mask is FP32 (its -0.0 is false)."""
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(10)
    M = valued_mask(rng, lens, Y.nrows, "FP32")
    M.vals[np.flatnonzero(M.vals == 0)[0]] = -0.0
    product(X, Y, M, "PLUS_TIMES", "FP64", struct=False, cast=True, what="cast")
    product(X, Y, M, "PLUS_TIMES", "FP64", struct=True, cast=True, what="cast structural")
    product(X, Y, M, "PLUS_PAIR", "FP64", cast=False, what="pair")
    Xf = full(rng, X.nrows, X.ncols, "FP64")
    product(Xf, Y, M, "PLUS_FIRST", "FP64", cast=False, what="first: only X is read, and it needs no cast")
    product(Xf, Y, M, "PLUS_SECOND", "FP64", cast=True, what="second: only Y is read")


def test_fullness_with_pending_edits():
    rng = np.random.default_rng(11)
    m, n, k = 20, 30, 7
    X = full(rng, m, k, "FP64"); Y = full(rng, n, k, "FP64")
    M = mask_of(rng, [int(x) for x in rng.integers(0, 8, m)], n)
    dX = up_full(X)
    dX[4, 2] = 9.5                                                             # a queued edit on an HBM-only matrix: still full, and the product sees it
    X.vals[4 * k + 2] = 9.5
    product(X, Y, M, "PLUS_TIMES", "FP64", dA=dX, what="set element")
    del dX[11, 0]
    holed = MM.Mat(m, k, np.delete(X.keys, 11 * k), np.delete(X.vals, 11 * k))
    product(holed, Y, M, "PLUS_TIMES", "FP64", dA=dX, routed=False, what="removed element"); off_route("removed element")
    dY = up_full(Y)
    del dY[0, 0]
    holedY = MM.Mat(n, k, np.delete(Y.keys, 0), np.delete(Y.vals, 0))
    product(X, holedY, M, "PLUS_TIMES", "FP64", dB=dY, routed=False, what="Y not full"); off_route("Y not full")


# ---- routing, hook unset ---------------------------------------------------------------------------------------------------------------------------------------
def test_default_rule(monkeypatch):
    MINW = geometry()[3]
    (m0, k, n0), (m1, _, n1) = default_rule_shapes(MINW)
    assert m0 * k * n0 < MINW <= m1 * k * n1
    rng = np.random.default_rng(12)
    X = full(rng, m1, k, "FP32"); Y = full(rng, n1, k, "FP32")
    M = mask_of(rng, [int(x) for x in rng.integers(0, 4, m1)], n1)
    Xs = MM.Mat(m0, k, X.keys[:m0 * k], X.vals[:m0 * k]); Ys = MM.Mat(n0, k, Y.keys[:n0 * k], Y.vals[:n0 * k])
    inside = (M.rows < m0) & (M.cols < n0)
    Ms = MM.Mat(m0, n0, M.rows[inside] * n0 + M.cols[inside], M.vals[inside])
    monkeypatch.delenv("GRB_MI355X_SDDMM")
    product(X, Y, M, "PLUS_TIMES", "FP32", what="above the threshold")                                          # asserts the route
    product(Xs, Ys, Ms, "PLUS_TIMES", "FP32", routed=False, what="below the threshold"); off_route("below the threshold")
    product(X, Y, M, "PLUS_TIMES", "FP32", comp=True, routed=False, what="complemented"); off_route("complemented")
    monkeypatch.setenv("GRB_MI355X_SDDMM", "0")
    product(X, Y, M, "PLUS_TIMES", "FP32", routed=False, what="hook 0"); off_route("hook 0")
    monkeypatch.setenv("GRB_MI355X_SDDMM", "1")
    product(Xs, Ys, Ms, "PLUS_TIMES", "FP32", what="hook 1 below the threshold")
    monkeypatch.setenv("GRB_MI355X_FULL", "1")                                                                   # the spmm_full hook still wins
    product(X, Y, M, "PLUS_TIMES", "FP32", routed=False, what="FULL=1"); off_route("FULL=1")
    assert gb.last_kernel_plan().startswith("spmm_full<")


def test_matrix_sddmm_is_the_mxm_call():
    X, Y, lens = sem_operands()
    rng = np.random.default_rng(13)
    M = valued_mask(rng, lens, Y.nrows, "INT8")
    dX, dY, dM = up_full(X), up_full(Y), up(M)
    for structural in (True, False):
        s = dM.sddmm(dX, dY, gb.INT32.PLUS_TIMES, structural=structural)
        assert_route(X.ncols, M.nvals, False, "Matrix.sddmm")
        r = dX.mxm(dY, semiring=gb.INT32.PLUS_TIMES, mask=dM, out=gb.Matrix.sparse(gb.INT32, X.nrows, Y.nrows), desc=desc_of(struct=structural, t1=True))
        for a, b in zip(s.to_csr(), r.to_csr()):
            assert np.array_equal(a, b)
        check(s, PM.mxm(MM.empty(X.nrows, Y.nrows, "INT32"), X, Y, "PLUS", "TIMES", "INT32", mask=M, struct=structural, tran_b=True), "Matrix.sddmm")
    assert dM.sddmm(dX, dY).type is gb.INT32                                         # no semiring: the operands' type and its default semiring
    Cm = some_C(rng, X.nrows, Y.nrows, "INT32"); dC = up(Cm)
    out = dM.sddmm(dX, dY, gb.INT32.PLUS_TIMES, out=dC, accum=gb.INT32.PLUS)
    assert out is dC
    check(dC, PM.mxm(Cm, X, Y, "PLUS", "TIMES", "INT32", mask=M, struct=True, accum=("PLUS", "INT32"), tran_b=True), "Matrix.sddmm accum")


# ---- floating-point order: normal random values --------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("k", [3, 65, 257])
@pytest.mark.parametrize("typ", ["FP32", "FP64"])
def test_floating_point_order(typ, k):
    """Each entry within 2 k u sum_l |X(i,l) Y(j,l)| of the exact dot product (FP32: the FP64 product; FP64: math.fsum) — the any-order summation bound, doubled for
    the products' own rounding and a possible fused multiply-add; the same call gives the same bits twice; and one (i, j) gives the same bits under two masks, one
    where it is the first entry of a tile and one where it follows a hub row."""
    TILE = geometry()[0]
    u = 2.0 ** -24 if typ == "FP32" else 2.0 ** -53
    rng = np.random.default_rng(k)
    m, n = 9, 2 * TILE + 11
    Xd = rng.standard_normal((m, k)).astype(NP[typ]); Yd = rng.standard_normal((n, k)).astype(NP[typ])
    dX, dY = gb.Matrix.from_dense(Xd), gb.Matrix.from_dense(Yd)
    i, j = 5, 17
    # mask 1: rows 0 .. 4 hold TILE entries together, so (5, 17) is entry TILE: the first of the second tile.  mask 2: row 4 is a hub of 2 TILE + 3 entries and
    # (5, 17) follows it, in the middle of a tile.
    lens1 = [TILE - 4, 0, 1, 2, 1]; lens2 = [3, 0, 0, 1, 2 * TILE + 3]
    results = []
    for lens in (lens1, lens2):
        front = sparse(rng, lens, n, "BOOL")
        tail_cols = np.sort(rng.choice(np.arange(j + 1, n), size=6, replace=False))
        keys = np.concatenate((front.keys, [i * n + j], i * n + tail_cols, 7 * n + np.arange(0, n, 3))).astype(np.int64)
        M = MM.Mat(m, n, keys, np.ones(len(keys), np.bool_))
        at = int(np.searchsorted(M.keys, i * n + j))
        assert at == sum(lens) and (at % TILE == 0) == (lens is lens1)
        dM = up(M)
        runs = []
        for _ in range(2):
            c = dX.mxm(dY, semiring=getattr(TYPE[typ], "PLUS_TIMES"), mask=dM, out=gb.Matrix.sparse(TYPE[typ], m, n), desc=desc_of(struct=True, t1=True))
            assert_route(k, M.nvals, False, "order")
            runs.append(c.to_csr())
        for a, b in zip(*runs):
            assert np.array_equal(bits(a), bits(b)), "two runs differ"
        rp, ci, x = runs[0]
        assert np.array_equal(ci.astype(np.int64), M.cols) and len(x) == M.nvals
        for p in range(M.nvals):
            terms = Xd[M.rows[p]].astype(np.float64) * Yd[M.cols[p]].astype(np.float64)
            exact = float(terms.sum()) if typ == "FP32" else math.fsum(float(a) * float(b) for a, b in zip(Xd[M.rows[p]], Yd[M.cols[p]]))
            bound = 2 * k * u * float(np.abs(terms).sum())
            assert abs(float(x[p]) - exact) <= bound, (typ, k, p, float(x[p]), exact, bound)
        results.append(x[at])
    assert bits(results[0]).tolist() == bits(results[1]).tolist(), "one entry, two masks: different bits"
