"""The product of two full matrices (the gemm_full route of GrB_mxm: grb_gemm.hip, grb_gemm_kernels.hpp) against the numpy model of tests/product_model.py —
`PM.mxm`, which is pinned to the oracle — BIT FOR BIT on `to_csr()` (row pointers, columns, values).

Every edge is read from GrBX_gemm_geometry: TM x TN = the wide tile, TTM x TTN = the tall one (results of at most TALLN columns), KT = products per step, WAVES
and CAP = waves per workgroup and the grid cap, MINW = the work m k n from which the route is taken by itself.  Floating-point values lie on the 1/8 grid without
zeros and are small enough that every summation is exact; the narrow integer types carry their extremes (they wrap, in any order alike).  Cases run with
GRB_MI355X_GEMM=1 unless they are about the default rule, and every routed case asserts the plan string — `gemm_full<m=M,n=N,k=K,tile=TMxTN,layout=..,cast=..>`
with the values the case was built for — so that a case that went another way fails instead of passing.  op(A) is m x k, op(B) k x n.

The last section is about rounding: normal random values, where the order matters — the route promises the left-to-right order whatever the position and layout."""
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
from test_spmm_full_gpu import values, sparse, full, up, up_full, some_mask
from test_gemm_full_host import default_rule_shapes

pytestmark = pytest.mark.gpu
NP = MM.NP
REAL = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]


@functools.lru_cache(maxsize=None)
def geometry():
    out = (C.c_uint64 * 9)()
    assert gb.lib.GrBX_gemm_geometry(out) == 0
    return tuple(int(v) for v in out)              # TM, TN, TTM, TTN, KT, WAVES, CAP, MINW, TALLN


@pytest.fixture(autouse=True)
def route_hook(gpu, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_GEMM", "1")
    for name in ("GRB_MI355X_FULL", "GRB_MI355X_SDDMM", "GRB_MI355X_DETERMINISTIC", "GRB_MI355X_SPGEMM", "GRB_MI355X_MXM_ROWS", "GRB_MI355X_BATCH"):
        monkeypatch.delenv(name, raising=False)


PLAN = re.compile(r"^gemm_full<m=(\d+),n=(\d+),k=(\d+),tile=(\d+)x(\d+),layout=([NT][NT]),cast=([01])> k_full_pattern k_gemm_full ")


def assert_route(m, n, k, t0=False, t1=False, cast=None, what=""):
    TM, TN, TTM, TTN, _, _, _, _, TALLN = geometry()
    plan = gb.last_kernel_plan() + " "
    g = PLAN.match(plan)
    assert g, f"{what}: not on the gemm_full route: {plan}"
    tile = (TTM, TTN) if n <= TALLN else (TM, TN)
    assert tuple(int(v) for v in g.groups()[:5]) == (m, n, k) + tile, f"{what}: {plan}"
    assert g.group(6) == ("T" if t0 else "N") + ("T" if t1 else "N"), f"{what}: {plan}"
    if cast is not None:
        assert int(g.group(7)) == int(cast), f"{what}: {plan}"


def off_route(what):
    plan = gb.last_kernel_plan()
    assert "gemm_full<" not in plan, f"{what}: {plan}"


def product(A, B, sr, typ, dA=None, dB=None, C=None, dC=None, mask=None, dM=None, struct=False, comp=False, replace=False, accum=None, t0=False, t1=False, routed=True, cast=None,
            what=""):
    """dA.mxm(dB) into dC (a fresh matrix of the semiring's type when not given) against the model; `accum` = (operator, type).  A and B are the operands as the
    call gets them (k x m under t0, n x k under t1).  `routed`: assert the route with op(A)'s and op(B)'s shape."""
    add, mul = sr.split("_")
    dA = up_full(A) if dA is None else dA; dB = up_full(B) if dB is None else dB
    opA = MM.transpose(A) if t0 else A; opB = MM.transpose(B) if t1 else B
    if C is None:
        C = MM.empty(opA.nrows, opB.ncols, typ)
    if dC is None:
        dC = up(C)
    if mask is not None and dM is None:
        dM = up(mask)
    exp = PM.mxm(C, A, B, add, mul, typ, mask=mask, struct=struct, comp=comp, replace=replace, accum=accum, tran_a=t0, tran_b=t1)
    dA.mxm(dB, semiring=getattr(TYPE[typ], sr), mask=dM, out=dC, accum=getattr(TYPE[accum[1]], accum[0]) if accum else None, desc=desc_of(replace, struct, comp, t0, t1))
    what = f"{what} {typ}.{sr} m={opA.nrows} n={opB.ncols} k={opA.ncols}"
    if routed:
        assert_route(opA.nrows, opB.ncols, opA.ncols, t0, t1, cast, what)
    check(dC, exp, what)
    return dC, exp


# ---- tile edges: a row or column short of a tile, a whole tile, one more; the switch between the tall and the wide tile ------------------------------------------
def edge(name):
    TM, TN, TTM, TTN, KT, _, _, _, TALLN = geometry()
    return {"1": 1, "TM-1": TM - 1, "TM": TM, "TM+1": TM + 1, "TALLN-1": TALLN - 1, "TALLN": TALLN, "TALLN+1": TALLN + 1, "TN-1": TN - 1, "TN": TN, "TN+1": TN + 1,
            "2TN+1": 2 * TN + 1, "TTM-1": TTM - 1, "TTM+1": TTM + 1, "2": 2, "KT-1": KT - 1, "KT": KT, "KT+1": KT + 1, "2KT+1": 2 * KT + 1, "3": 3, "257": 257}[name]


@pytest.mark.parametrize("n", ["1", "TALLN-1", "TALLN", "TALLN+1", "TN-1", "TN", "TN+1", "2TN+1"])
@pytest.mark.parametrize("m", ["1", "TM-1", "TM", "TM+1"])
def test_tile_edges(m, n):
    m, n, k = edge(m), edge(n), 5
    rng = np.random.default_rng(m * 1000 + n)
    X = full(rng, m, k, "FP32"); W = full(rng, k, n, "FP32")
    dC, exp = product(X, W, "PLUS_TIMES", "FP32", cast=False, what="tile edges")
    assert exp.nvals == m * n and dC.is_full
    X = full(rng, m, k, "INT64"); W = full(rng, k, n, "INT64")
    product(X, W, "MIN_PLUS", "INT64", cast=False, what="tile edges")


@pytest.mark.parametrize("m", ["TTM-1", "TTM+1"])
def test_tall_tile_edges(m):
    m, n, k = edge(m), 3, 5
    rng = np.random.default_rng(m)
    product(full(rng, m, k, "FP32"), full(rng, k, n, "FP32"), "PLUS_TIMES", "FP32", what="tall edges")
    product(full(rng, m, k, "INT8"), full(rng, k, n, "INT8"), "PLUS_TIMES", "INT8", what="tall edges")
    product(full(rng, m, k, "FP64"), full(rng, k, n, "FP64"), "MIN_PLUS", "FP64", what="tall edges")


# ---- k edges: one product, a ragged first step, a whole step, a ragged last step, many steps ----------------------------------------------------------------------
K_EDGES = ["1", "2", "KT-1", "KT", "KT+1", "2KT+1", "257"]
MORE = ["MIN_PLUS", "MAX_MIN", "ANY_PAIR", "PLUS_PAIR", "PLUS_FIRST", "PLUS_SECOND"]


def k_cases():
    out = [(t, "LOR_LAND" if t == "BOOL" else "PLUS_TIMES") for t in REAL]
    out += [(t, s) for t in ("INT64", "FP32", "FP64") for s in MORE]
    return out + [("INT8", "MAX_FIRST"), ("UINT16", "TIMES_PLUS")]            # run-time operator codes (MAX_MIN above is one too); MAX_FIRST stages one side only


@pytest.mark.parametrize("k", K_EDGES)
@pytest.mark.parametrize("typ,sr", k_cases())
def test_k_edges(typ, sr, k):
    TM, TN = geometry()[:2]
    k = edge(k); m, n = TM + 3, TN + 5
    rng = np.random.default_rng(k * 131 + sum(map(ord, typ + sr)))
    X = full(rng, m, k, typ); W = full(rng, k, n, typ)
    product(X, W, sr, typ, cast=False, what="k edges")


@pytest.mark.parametrize("typ", ["INT32", "FP64"])
def test_any_second_of_constant_columns(typ):
    """ANY may keep any product: with SECOND and column j of W constant c_j != 0 every choice is c_j — and an accumulator that started from an identity, or a
    fold over LDS padding in the ragged step, would show."""
    TM, TN, _, _, KT = geometry()[:5]
    rng = np.random.default_rng(3)
    for n in (6, TN + 5):
        k = KT + 3
        c = np.arange(1, n + 1).astype(NP[typ]) * (1 if typ == "INT32" else 0.5)
        X = full(rng, TM + 3, k, typ); W = MM.Mat(k, n, np.arange(k * n, dtype=np.int64), np.tile(c, k))
        product(X, W, "ANY_SECOND", typ, what="any")


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tall", "wide"])
@pytest.mark.parametrize("t1", [False, True])
@pytest.mark.parametrize("t0", [False, True])
def test_layouts(t0, t1, shape):
    TM, TN, TTM, TTN, KT = geometry()[:5]
    m, n, k = (TTM + 3, 3, KT + 3) if shape == "tall" else (TM + 3, TN + 5, KT + 3)
    rng = np.random.default_rng(7 + 2 * t0 + t1)
    for typ, sr in (("INT32", "PLUS_TIMES"), ("FP64", "MIN_PLUS"), ("INT8", "PLUS_TIMES")):
        X = full(rng, m, k, typ); W = full(rng, k, n, typ)
        A = MM.transpose(X) if t0 else X; B = MM.transpose(W) if t1 else W
        product(A, B, sr, typ, t0=t0, t1=t1, what=f"layout {shape}")


def test_both_operands_one_object():
    TM, _, _, _, KT = geometry()[:5]
    rng = np.random.default_rng(9)
    m, k = TM + 3, KT + 1
    X = full(rng, m, k, "INT64"); dX = up_full(X)
    product(X, X, "PLUS_TIMES", "INT64", dA=dX, dB=dX, t1=True, what="X X'")                   # m x m, the Gram matrix of the rows
    product(X, X, "PLUS_TIMES", "INT64", dA=dX, dB=dX, t0=True, what="X' X")                   # k x k
    S = full(rng, 37, 37, "INT64"); dS = up_full(S)
    product(S, S, "PLUS_TIMES", "INT64", dA=dS, dB=dS, what="S S")
    product(S, S, "PLUS_TIMES", "INT64", dA=dS, dB=dS, t0=True, t1=True, what="S' S'")


# ---- masks, accumulators, casts -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wb_operands():
    TM, TN, _, _, KT = geometry()[:5]
    rng = np.random.default_rng(21)
    return full(rng, TM + 3, KT + 2, "INT32"), full(rng, KT + 2, TN + 5, "INT32")


@pytest.mark.parametrize("kind", ["valued", "structural", "complemented", "replace", "complemented_replace"])
def test_masks(kind):
    X, W = wb_operands()
    rng = np.random.default_rng(len(kind))
    M = some_mask(rng, X.nrows, W.ncols, "INT8")
    assert (M.vals == 0).any() and (M.vals != 0).any()
    keys = np.flatnonzero(rng.random(X.nrows * W.ncols) < 0.4).astype(np.int64)
    Cm = MM.Mat(X.nrows, W.ncols, keys, values(rng, "INT32", len(keys)))
    kw = dict(mask=M, struct=kind == "structural", comp=kind.startswith("complemented"), replace=kind.endswith("replace"))
    product(X, W, "PLUS_TIMES", "INT32", C=Cm, what=kind, **kw)
    product(X, W, "PLUS_TIMES", "INT32", what=kind + " empty C", **kw)


def test_accumulator_of_another_type():
    X, W = wb_operands()
    rng = np.random.default_rng(2)
    keys = np.flatnonzero(rng.random(X.nrows * W.ncols) < 0.5).astype(np.int64)
    Cm = MM.Mat(X.nrows, W.ncols, keys, values(rng, "INT64", len(keys)))
    product(X, W, "PLUS_TIMES", "INT32", C=Cm, accum=("PLUS", "INT64"), what="accum")
    Cm = MM.Mat(X.nrows, W.ncols, keys, values(rng, "FP64", len(keys)))
    product(X, W, "PLUS_TIMES", "INT32", C=Cm, accum=("MINUS", "FP64"), mask=some_mask(rng, X.nrows, W.ncols, "BOOL"), what="accum + mask")


def test_output_is_an_operand():
    rng = np.random.default_rng(4)
    n = geometry()[0] + 6
    X = full(rng, n, n, "FP64"); W = full(rng, n, n, "FP64")
    dX = up_full(X)
    product(X, W, "PLUS_TIMES", "FP64", dA=dX, C=X, dC=dX, what="C is A")
    dW = up_full(W)
    product(X, W, "PLUS_TIMES", "FP64", dB=dW, C=W, dC=dW, what="C is B")
    dX = up_full(X)
    product(X, X, "PLUS_TIMES", "FP64", dA=dX, dB=dX, C=X, dC=dX, accum=("PLUS", "FP64"), what="C is A is B, accumulated")


def test_mixed_operand_types():
    """X INT32, W FP64, an FP32 semiring: both operands are cast once; PAIR reads neither side; FIRST / SECOND read and cast one."""
    TM, TN, _, _, KT = geometry()[:5]
    rng = np.random.default_rng(8)
    X = full(rng, TM + 1, KT + 4, "INT32"); W = full(rng, KT + 4, TN + 2, "FP64")
    product(X, W, "PLUS_TIMES", "FP32", cast=True, what="mixed")
    product(X, W, "PLUS_PAIR", "FP32", cast=False, what="mixed pair")
    product(X, W, "PLUS_FIRST", "INT32", cast=False, what="first: only X is read, and it needs no cast")
    product(X, W, "PLUS_SECOND", "INT32", cast=True, what="second: only W is read")
    Xt = MM.transpose(X)
    product(Xt, W, "PLUS_TIMES", "FP32", t0=True, cast=True, what="mixed, T0")


# ---- routing, hooks unset ---------------------------------------------------------------------------------------------------------------------------------------------
def test_default_rule(monkeypatch):
    MINW = geometry()[7]
    (m0, k, n0), (m1, _, n1) = default_rule_shapes(MINW)
    assert m0 * k * n0 < MINW <= m1 * k * n1
    rng = np.random.default_rng(12)
    X = full(rng, m1, k, "FP32"); W = full(rng, k, n1, "FP32")
    Xs = MM.Mat(m0, k, X.keys[:m0 * k], X.vals[:m0 * k]); Ws = full(rng, k, n0, "FP32")
    monkeypatch.delenv("GRB_MI355X_GEMM")
    product(X, W, "PLUS_TIMES", "FP32", what="above the threshold")                                              # asserts the route
    product(Xs, Ws, "PLUS_TIMES", "FP32", routed=False, what="below the threshold"); off_route("below the threshold")
    m_one = -(-MINW // k) + 1                                                                                     # n = 1: enough work, one column
    product(full(rng, m_one, k, "FP32"), full(rng, k, 1, "FP32"), "PLUS_TIMES", "FP32", routed=False, what="n = 1"); off_route("n = 1")
    TTM, TTN = geometry()[2:4]                                                                                    # enough work in ONE tall tile: too few tiles
    kk = -(-MINW // (TTM * TTN))
    product(full(rng, TTM, kk, "FP32"), full(rng, kk, TTN, "FP32"), "PLUS_TIMES", "FP32", routed=False, what="one tile"); off_route("one tile")
    assert gb.last_kernel_plan().startswith("spmm_full<"), gb.last_kernel_plan()
    M = some_mask(rng, m1, n1, "BOOL", density=0.02)
    product(X, W, "PLUS_TIMES", "FP32", mask=M, routed=False, what="plain mask"); off_route("plain mask")
    product(X, W, "PLUS_TIMES", "FP32", mask=M, comp=True, what="complemented mask")                            # on the route
    dX = up_full(X)
    dX[4, 2] = 9.5                                                            # a queued edit on an HBM-only matrix: still full, and the product sees it
    Xe = MM.Mat(m1, k, X.keys, X.vals.copy()); Xe.vals[4 * k + 2] = 9.5
    product(Xe, W, "PLUS_TIMES", "FP32", dA=dX, what="set element")
    del dX[11, 0]
    holed = MM.Mat(m1, k, np.delete(Xe.keys, 11 * k), np.delete(Xe.vals, 11 * k))
    product(holed, W, "PLUS_TIMES", "FP32", dA=dX, routed=False, what="removed element"); off_route("removed element")
    monkeypatch.setenv("GRB_MI355X_GEMM", "0")
    product(X, W, "PLUS_TIMES", "FP32", routed=False, what="hook 0"); off_route("hook 0")
    assert gb.last_kernel_plan().startswith("spmm_full<"), gb.last_kernel_plan()                                 # the route such a call took before
    monkeypatch.setenv("GRB_MI355X_GEMM", "1")
    product(Xs, Ws, "PLUS_TIMES", "FP32", what="hook 1 below the threshold")
    product(X, W, "PLUS_TIMES", "FP32", mask=M, what="hook 1 with a plain mask")
    monkeypatch.delenv("GRB_MI355X_GEMM")
    monkeypatch.setenv("GRB_MI355X_FULL", "1")                                                                   # the spmm_full hook keeps its meaning
    product(X, W, "PLUS_TIMES", "FP32", routed=False, what="FULL=1"); off_route("FULL=1")
    assert gb.last_kernel_plan().startswith("spmm_full<"), gb.last_kernel_plan()


# ---- chains -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_chains(monkeypatch):
    TM = geometry()[0]
    rng = np.random.default_rng(10)
    n, k = TM + 7, 5
    H = full(rng, n, k, "INT64"); W = full(rng, k, k, "INT64")
    dH, dW = up_full(H), up_full(W)
    for step in range(3):
        dH, H = product(H, W, "PLUS_TIMES", "INT64", dA=dH, dB=dW, what=f"chain step {step}")
        assert dH.is_full and H.nvals == n * k
    # one layer A H W: the sparse half on the spmm_full route, the dense half here
    monkeypatch.setenv("GRB_MI355X_FULL", "1")
    A = sparse(rng, [int(x) for x in rng.integers(1, 4, n)], n, "INT64"); dA = up(A)
    dAH = dA.mxm(dH, semiring=gb.INT64.PLUS_TIMES)
    assert gb.last_kernel_plan().startswith("spmm_full<"), gb.last_kernel_plan()
    AH = PM.mxm(MM.empty(n, k, "INT64"), A, H, "PLUS", "TIMES", "INT64")
    check(dAH, AH, "A H"); assert dAH.is_full
    product(AH, W, "PLUS_TIMES", "INT64", dA=dAH, dB=dW, what="(A H) W")                                         # asserts gemm_full<


def test_past_one_grid_round():
    """One wide tile more than the capped grid takes in one round."""
    TM, TN, _, _, _, _, CAP = geometry()[:7]
    m, n, k = (CAP + 1) * TM, TN, 2
    rng = np.random.default_rng(5)
    dC, exp = product(full(rng, m, k, "INT32"), full(rng, k, n, "INT32"), "PLUS_TIMES", "INT32", what="grid round")
    assert exp.nvals == m * n


# ---- floating-point order: normal random values ----------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("k", ["3", "KT+1", "257"])
@pytest.mark.parametrize("typ", ["FP32", "FP64"])
def test_floating_point_order(typ, k):
    """Each entry within 2 k u sum_l |x w| of the exact dot product (FP32: the FP64 product; FP64: math.fsum) — the bound of test_sddmm_gpu.py, doubled for a
    possible fused multiply-add; the same call gives the same bits twice; identical rows of X at 0 and TM + 3 and identical columns of W at 0 and TN + 5 give four
    entries with the same bits (two positions in a tile, four tiles), and the same bits again when W is handed over transposed (layout NT)."""
    TM, TN = geometry()[:2]
    k = edge(k)
    u = 2.0 ** -24 if typ == "FP32" else 2.0 ** -53
    rng = np.random.default_rng(k)
    m, n = TM + 9, TN + 11
    Xd = rng.standard_normal((m, k)).astype(NP[typ]); Wd = rng.standard_normal((k, n)).astype(NP[typ])
    Xd[TM + 3] = Xd[0]; Wd[:, TN + 5] = Wd[:, 0]
    dX, dW, dWt = gb.Matrix.from_dense(Xd), gb.Matrix.from_dense(Wd), gb.Matrix.from_dense(np.ascontiguousarray(Wd.T))
    sr = getattr(TYPE[typ], "PLUS_TIMES")
    runs = []
    for _ in range(2):
        c = dX.mxm(dW, semiring=sr)
        assert_route(m, n, k, False, False, False, "order")
        runs.append(c.to_csr())
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b)), "two runs differ"
    x = runs[0][2].reshape(m, n)
    terms_abs = np.abs(Xd.astype(np.float64)) @ np.abs(Wd.astype(np.float64))
    if typ == "FP32":
        exact = Xd.astype(np.float64) @ Wd.astype(np.float64)
    else:
        exact = np.array([[math.fsum(float(a) * float(b) for a, b in zip(Xd[i], Wd[:, j])) for j in range(n)] for i in range(m)])
    err = np.abs(x.astype(np.float64) - exact); bound = 2 * k * u * terms_abs
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{typ} k={k}: largest error / bound = {float((err / bound).max()):.3g}")
    assert (err <= bound).all(), (typ, k, worst, float(x[worst]), float(exact[worst]), float(bound[worst]))
    four = [x[0, 0], x[0, TN + 5], x[TM + 3, 0], x[TM + 3, TN + 5]]
    assert all(bits(v).tolist() == bits(four[0]).tolist() for v in four), f"one dot product, four positions: {four}"
    ct = dX.mxm(dWt, semiring=sr, out=gb.Matrix.sparse(TYPE[typ], m, n), desc=desc_of(t1=True))
    assert_route(m, n, k, False, True, False, "order NT")
    xt = ct.to_csr()[2].reshape(m, n)
    four_t = [xt[0, 0], xt[0, TN + 5], xt[TM + 3, 0], xt[TM + 3, TN + 5]]
    assert all(bits(v).tolist() == bits(four[0]).tolist() for v in four_t), f"NN against NT: {four} {four_t}"
    assert np.array_equal(bits(x), bits(xt)), "NN and NT differ somewhere"
