"""A full matrix times a vector (the gemv_full route of GrB_mxv / GrB_vxm: grb_gemv.hip, grb_gemv_kernels.hpp) against the numpy model of tests/product_model.py —
`PM.mxv` / `PM.vxm`, which are pinned to the oracle — BIT FOR BIT on the result's values and pattern.

Every edge is read from GrBX_gemv_geometry: LOAD = bytes per lane load, GMAX = the longest row that shares a wave (layout N), L = products per chunk (N), WAVES
and CAP = waves per workgroup and the grid cap, RT = rows per chunk (layout T, for the inner lengths used here), MINW = the entries of A from which the route is
taken by itself.  Floating-point values lie on the 1/8 grid without zeros and are small enough that every summation is exact in any order; the narrow integer
types carry their extremes (they wrap, in any order alike).  Cases run with GRB_MI355X_GEMV=1 unless they are about the default rule, and every routed case
asserts the plan string — `gemv_full<m=M,k=K,layout=N|T,holes=..,chunks=..,cast=..>` with the values the case was built for — so that a case that went another
way fails instead of passing.  m is the outer length (the result's), k the inner.

Forms: "mxv" is w = A u (layout N), "mxv_t" w = A' u (desc T0: layout T), "vxm" w' = u' A (layout T), "vxm_t" w' = u' A' (desc T1: layout N).

The last section is about rounding: normal random values, where the order matters — the route promises an order that depends on k, the layout and u's pattern
alone, and the any-order bound."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import matrix_model as MM
import vector_model as VM
import product_model as PM
import pygraphblas_amd as gb
from helpers import TYPE
from test_matrix_kernels_at_size_gpu import desc_of
from test_vector_kernels_at_size_gpu import check, dev
from test_spmm_full_gpu import values, full, up, up_full, sparse
from test_gemv_full_host import default_rule_shapes

pytestmark = pytest.mark.gpu
NP = MM.NP
REAL = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
FORMS = {"mxv": "N", "mxv_t": "T", "vxm": "T", "vxm_t": "N"}


@functools.lru_cache(maxsize=None)
def geometry():
    return all_geometry()[:9]                      # LOAD, GMAX, L, WAVES, CAP, RT, MAXCH, MINW, UNROLL


@functools.lru_cache(maxsize=None)
def all_geometry():
    out = (C.c_uint64 * 10)()
    assert gb.lib.GrBX_gemv_geometry(out) == 0
    return tuple(int(v) for v in out)


def pack(size):
    """Values a lane loads at once: LOAD bytes' worth, at most out[9]."""
    return min(all_geometry()[0] // size, all_geometry()[9])


@pytest.fixture(autouse=True)
def route_hook(gpu, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_GEMV", "1")
    for name in ("GRB_MI355X_SPMV", "GRB_MI355X_DETERMINISTIC", "GRB_MI355X_BATCH"):
        monkeypatch.delenv(name, raising=False)


PLAN = re.compile(r"^gemv_full<m=(\d+),k=(\d+),layout=([NT]),holes=([01]),chunks=(\d+),cast=([01])> (.*)$")


def chunks_of(layout, k):
    _, GMAX, L, _, _, RT, MAXCH, _, _ = geometry()
    if layout == "N":
        return 1 if k <= GMAX else -(-k // L)
    p = 1
    while p < k: p *= 2
    rt = max(RT, p // MAXCH)                         # gemv_t_chunk of grb_gemv_geom.hpp: longer chunks for columns of more than RT MAXCH rows
    return max(1, -(-k // rt))


def assert_route(m, k, layout, holes=None, cast=None, empty=False, what=""):
    plan = gb.last_kernel_plan() + " "
    g = PLAN.match(plan)
    assert g, f"{what}: not on the gemv_full route: {plan}"
    assert (int(g.group(1)), int(g.group(2)), g.group(3)) == (m, k, layout), f"{what}: {plan}"
    if holes is not None:
        assert int(g.group(4)) == int(holes), f"{what}: {plan}"
    if cast is not None:
        assert int(g.group(6)) == int(cast), f"{what}: {plan}"
    if empty:
        assert g.group(7).strip() == "" and int(g.group(5)) == 0, f"{what}: an empty operand launches nothing: {plan}"
        return
    nch = chunks_of(layout, k)
    assert int(g.group(5)) == nch, f"{what}: {plan}"
    kernel = "k_gemv_t" if layout == "T" else "k_gemv_n_short" if k <= geometry()[1] else "k_gemv_n_wave"
    assert g.group(7).split() == [kernel] + (["k_gemv_fold"] if nch > 1 else []), f"{what}: {plan}"


def off_route(what):
    plan = gb.last_kernel_plan()
    assert "gemv_full<" not in plan, f"{what}: {plan}"


def vec(rng, typ, n, present=None):
    """A model vector: values at every position (what lies behind a hole must not matter), `present` a boolean array or None for full."""
    return VM.Vec(values(rng, typ, n), np.ones(n, bool) if present is None else np.asarray(present, bool))


def product(form, A, U, sr, typ, dA=None, dU=None, W=None, dW=None, mask=None, struct=False, comp=False, replace=False, accum=None, routed=True, cast=None, what=""):
    """One product on the device and in the model; A is the matrix as the call gets it (M = A for mxv / vxm_t, A' for mxv_t / vxm).  `accum` = (operator, type)."""
    add, mul = sr.split("_")
    layout = FORMS[form]
    m, k = (A.nrows, A.ncols) if layout == "N" else (A.ncols, A.nrows)
    dA = up_full(A) if dA is None else dA
    dU = dev(U, full=bool(U.pres.all())) if dU is None else dU
    if W is None:
        W = VM.empty(m, typ)
    if dW is None:
        dW = dev(W)
    dM = None if mask is None else dev(mask)
    kw = dict(mask=mask, struct=struct, comp=comp, replace=replace, accum=accum)
    exp = PM.mxv(W, A, U, add, mul, typ, tran=form == "mxv_t", **kw) if form.startswith("mxv") else PM.vxm(W, U, A, add, mul, typ, tran=form == "vxm_t", **kw)
    acc = getattr(TYPE[accum[1]], accum[0]) if accum else None
    if form.startswith("mxv"):
        dA.mxv(dU, semiring=getattr(TYPE[typ], sr), out=dW, mask=dM, accum=acc, desc=desc_of(replace, struct, comp, t0=form == "mxv_t"))
    else:
        dU.vxm(dA, semiring=getattr(TYPE[typ], sr), out=dW, mask=dM, accum=acc, desc=desc_of(replace, struct, comp, t1=form == "vxm_t"))
    what = f"{what} {form} {typ}.{sr} m={m} k={k} [{gb.last_kernel_plan()}]"
    if routed:
        assert_route(m, k, layout, holes=not U.pres.all(), cast=cast, empty=not U.pres.any(), what=what)
    check(dW, exp, what)
    return dW, exp


def shaped(rng, layout, m, k, typ):
    """A full model matrix whose product in the given layout has outer length m and inner length k, and the form that reads it so through mxv."""
    return (full(rng, m, k, typ), "mxv") if layout == "N" else (full(rng, k, m, typ), "vxm")


# ---- layout N: the inner length ------------------------------------------------------------------------------------------------------------------------------------
def n_inner():
    return ["1", "2", "3", "4", "5", "32", "33", "63", "64", "65", "V-1", "V", "V+1", "R-1", "R", "R+1", "L-1", "L", "L+1", "2L+1"]


def edge(name, size=4):
    LOAD, GMAX, L, WAVES, CAP, RT, _, _, UNROLL = geometry()
    V = pack(size)
    table = {"V-1": GMAX + V - 1 + V, "V": GMAX + 2 * V, "V+1": GMAX + 2 * V + 1, "R-1": 64 * V * UNROLL - 1, "R": 64 * V * UNROLL, "R+1": 64 * V * UNROLL + 1,
             "L-1": L - 1, "L": L, "L+1": L + 1, "2L+1": 2 * L + 1, "RT-1": RT - 1, "RT": RT, "RT+1": RT + 1, "2RT+1": 2 * RT + 1}
    return table[name] if name in table else int(name)


@pytest.mark.parametrize("k", n_inner())
def test_n_inner_length(k):
    """Around every group size, a packet short / whole / over behind whole ones, a whole unrolled round of the wave -/+ 1, the chunk -/+ 1 and 2 L + 1; rows whose
    address is 16-byte aligned and rows whose address is not (odd k) share every case with five rows."""
    rng = np.random.default_rng(len(k) * 977 + sum(map(ord, k)))
    for typ, sr in (("FP32", "PLUS_TIMES"), ("INT64", "MIN_PLUS"), ("INT8", "PLUS_TIMES")):
        kk = edge(k, NP[typ]().itemsize)
        A = full(rng, 5, kk, typ)
        product("mxv", A, vec(rng, typ, kk), sr, typ, cast=False, what="N inner")
        pres = rng.random(kk) < 0.5; pres[rng.integers(kk)] = True
        if not pres.all():
            product("mxv", A, vec(rng, typ, kk, pres), sr, typ, what="N inner, holes")


@pytest.mark.parametrize("k", [1, 3, 64, 65])
def test_n_outer_length(k):
    """One row, the rows of a wave and of a workgroup -/+ 1 (k <= GMAX: 64 / G rows a wave; beyond: a wave per row)."""
    _, GMAX, _, WAVES, _, _, _, _, _ = geometry()
    G = 1
    while G < min(k, GMAX): G *= 2
    per_wave = 64 // G if k <= GMAX else 1
    rng = np.random.default_rng(k)
    for m in sorted({1, max(per_wave - 1, 1), per_wave + 1, WAVES * per_wave - 1, WAVES * per_wave, WAVES * per_wave + 1}):
        product("mxv", full(rng, m, k, "INT32"), vec(rng, "INT32", k), "PLUS_TIMES", "INT32", what="N outer")
        product("vxm_t", full(rng, m, k, "FP64"), vec(rng, "FP64", k), "PLUS_TIMES", "FP64", what="N outer")


def test_n_past_one_grid_round():
    """One row more than the capped grid takes in one round, inner length 1 (64 rows a wave); and one (row, chunk) unit more with a wave per row."""
    _, GMAX, _, WAVES, CAP, _, _, _, _ = geometry()
    rng = np.random.default_rng(5)
    m = CAP * WAVES * 64 + 1
    dW, exp = product("mxv", full(rng, m, 1, "INT32"), vec(rng, "INT32", 1), "PLUS_TIMES", "INT32", what="grid round")
    assert exp.pres.all()
    m = CAP * WAVES + 1
    product("mxv", full(rng, m, GMAX + 1, "INT8"), vec(rng, "INT8", GMAX + 1), "PLUS_TIMES", "INT8", what="grid round, waves")


# ---- layout T ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ["1", "63", "64", "65", "slab-1", "slab", "slab+1", "slab+V"])
def test_t_columns(m):
    """Columns around the lanes of a wave and around the slab, both packet widths: a column count V divides takes 16-byte packets, any other one value a lane."""
    LOAD = geometry()[0]
    rng = np.random.default_rng(sum(map(ord, m)))
    for typ, sr in (("FP32", "PLUS_TIMES"), ("FP64", "MIN_PLUS"), ("UINT8", "PLUS_TIMES")):
        V = pack(NP[typ]().itemsize)
        mm = {"slab-1": 64 * V - 1, "slab": 64 * V, "slab+1": 64 * V + 1, "slab+V": 64 * V + V}.get(m) or int(m)
        k = 7
        A = full(rng, k, mm, typ)
        product("vxm", A, vec(rng, typ, k), sr, typ, cast=False, what="T columns")
        product("mxv_t", A, vec(rng, typ, k, [1, 0, 1, 1, 0, 0, 1]), sr, typ, what="T columns, holes")


@pytest.mark.parametrize("k", ["1", "2", "63", "64", "65", "RT-1", "RT", "RT+1", "2RT+1"])
def test_t_rows(k):
    """Rows around a wave's piece and around the chunk; 70 columns (one value a lane) and 72 (packets)."""
    k = edge(k)
    rng = np.random.default_rng(k)
    for m in (70, 72):
        A = full(rng, k, m, "FP32")
        product("vxm", A, vec(rng, "FP32", k), "PLUS_TIMES", "FP32", what="T rows")
        A = full(rng, k, m, "INT64")
        pres = rng.random(k) < 0.5; pres[rng.integers(k)] = True
        product("vxm", A, vec(rng, "INT64", k, pres), "MIN_PLUS", "INT64", what="T rows, holes")


def test_t_more_units_than_the_grid_cap():
    """More (slab, chunk) units than the capped grid: CAP + 2 slabs of one chunk; then several slabs times several chunks, and a column long enough for the
    longer chunks (a chunk count above MAXCH never exists, so units beyond the cap come from the slabs)."""
    _, _, _, _, CAP, RT, MAXCH, _, _ = geometry()
    rng = np.random.default_rng(6)
    m = 64 * (CAP + 1) + 1                                                         # CAP + 2 slabs of one value a lane, one row
    product("vxm", full(rng, 1, m, "INT32"), vec(rng, "INT32", 1), "PLUS_TIMES", "INT32", what="T grid round, slabs")
    k = 5 * RT + 1                                                                 # 3 slabs x 6 chunks
    product("vxm", full(rng, k, 130, "INT8"), vec(rng, "INT8", k), "PLUS_TIMES", "INT8", what="T slabs x chunks")
    k = RT * MAXCH + 1                                                             # chunks of 2 RT rows
    pres = rng.random(k) < 0.5; pres[:2 * RT] = False
    product("vxm", full(rng, k, 3, "INT32"), vec(rng, "INT32", k, pres), "MIN_PLUS", "INT32", what="T long column")


# ---- holes in u ---------------------------------------------------------------------------------------------------------------------------------------------------------
def hole_shapes():
    _, GMAX, L, _, _, RT, _, _, _ = geometry()
    return [("N", 6, 5), ("N", 3, 2 * L + 1), ("T", 70, 5), ("T", 70, 2 * RT + 1)]


@pytest.mark.parametrize("pattern", ["none", "one", "all_but_one", "chunk_absent", "first_chunk_absent"])
def test_holes(pattern):
    _, GMAX, L, _, _, RT, _, _, _ = geometry()
    rng = np.random.default_rng(len(pattern))
    for layout, m, k in hole_shapes():
        chunk = L if layout == "N" else RT
        pres = np.ones(k, bool)
        if pattern == "none": pres[:] = False
        elif pattern == "one": pres[:] = False; pres[k // 2] = True
        elif pattern == "all_but_one": pres[k - 1] = False
        elif pattern == "chunk_absent" and k > chunk: pres[chunk: 2 * chunk] = False
        elif pattern == "chunk_absent": pres[1] = False
        else: pres[:min(chunk, k - 1)] = False
        for typ, sr in (("INT32", "MIN_TIMES"), ("FP64", "PLUS_TIMES"), ("INT64", "MAX_PLUS")):
            A, form = shaped(rng, layout, m, k, typ)
            W = vec(rng, typ, m, rng.random(m) < 0.5)
            product(form, A, vec(rng, typ, k, pres), sr, typ, what=f"holes {pattern}")
            product(form, A, vec(rng, typ, k, pres), sr, typ, W=W, what=f"holes {pattern}, w had entries")      # an empty T replaces them
            product(form, A, vec(rng, typ, k, pres), sr, typ, W=W, accum=("PLUS", typ), what=f"holes {pattern}, accumulated")


@pytest.mark.parametrize("typ", ["INT32", "FP64"])
def test_any_second_with_the_first_chunk_absent(typ):
    """ANY may keep any product: with SECOND (mxv: the operand's value) and u constant c != 0 at its present positions every choice is c — and an accumulator
    that started from an identity, or a fold over a partial nobody wrote (the first chunk holds no product), would show.  MIN with its first chunk absent as well."""
    rng = np.random.default_rng(3)
    for layout, m, k in hole_shapes()[1::2]:
        chunk = geometry()[2] if layout == "N" else geometry()[5]
        pres = np.ones(k, bool); pres[:chunk] = False
        c = NP[typ](5) if typ == "INT32" else NP[typ](2.5)
        U = VM.Vec(np.where(pres, c, NP[typ](77)).astype(NP[typ]), pres)
        A, form = shaped(rng, layout, m, k, typ)
        sr = "ANY_SECOND" if form == "mxv" else "ANY_FIRST"                        # (vxm: the operand is the multiplier's first argument)
        dW, exp = product(form, A, U, sr, typ, what="any")
        assert (exp.val == c).all()
        product(form, A, U, "MIN_SECOND" if form == "mxv" else "MIN_FIRST", typ, what="min, first chunk absent")


# ---- types and semirings --------------------------------------------------------------------------------------------------------------------------------------------
MORE = ["MIN_PLUS", "MAX_MIN", "ANY_PAIR", "PLUS_PAIR", "PLUS_FIRST", "PLUS_SECOND"]


def type_cases():
    out = [(t, "LOR_LAND" if t == "BOOL" else "PLUS_TIMES") for t in REAL]
    out += [(t, s) for t in ("INT64", "FP32", "FP64") for s in MORE]
    return out + [("INT8", "MAX_FIRST"), ("UINT16", "TIMES_PLUS")]               # run-time operator codes (DynSR; MAX_MIN above is one too)


@pytest.mark.parametrize("typ,sr", type_cases())
def test_every_type_and_semiring(typ, sr):
    """Each kernel once per case: short rows, a wave per row with two chunks, and layout T with two chunks; an operand with holes in the long ones."""
    _, GMAX, L, _, _, RT, _, _, _ = geometry()
    rng = np.random.default_rng(sum(map(ord, typ + sr)))
    for layout, m, k in (("N", 7, 5), ("N", 3, L + 37), ("T", 67, RT + 9), ("T", 64, 3)):
        A, form = shaped(rng, layout, m, k, typ)
        pres = None
        if k > GMAX:
            pres = rng.random(k) < 0.7; pres[0] = True
        product(form, A, vec(rng, typ, k, pres), sr, typ, cast=False, what="types")


def test_mixed_operand_types():
    """A INT32, u FP64, an FP32 semiring: both operands are cast once; PAIR reads neither side; FIRST / SECOND read and cast one."""
    rng = np.random.default_rng(8)
    A = full(rng, 9, 70, "INT32"); U = vec(rng, "FP64", 70); Ut = vec(rng, "FP64", 9)
    product("mxv", A, U, "PLUS_TIMES", "FP32", cast=True, what="mixed")
    product("mxv", A, U, "PLUS_PAIR", "FP32", cast=False, what="mixed pair")
    product("mxv", A, U, "PLUS_FIRST", "INT32", cast=False, what="first: only A is read, and it needs no cast")
    product("mxv", A, U, "PLUS_SECOND", "INT32", cast=True, what="second: only u is read")
    product("vxm", A, Ut, "PLUS_TIMES", "FP32", cast=True, what="mixed, T")
    product("vxm", A, Ut, "PLUS_FIRST", "INT32", cast=True, what="vxm first: only u is read")


# ---- masks, accumulators, the output ---------------------------------------------------------------------------------------------------------------------------------
def some_vmask(rng, n, typ):
    pres = rng.random(n) < 0.7
    val = (rng.random(n) < 0.5).astype(NP[typ])
    return VM.Vec(val, pres)


@pytest.mark.parametrize("form", ["mxv", "vxm"])
@pytest.mark.parametrize("kind", ["valued", "structural", "complemented", "replace", "complemented_replace"])
def test_masks(kind, form):
    rng = np.random.default_rng(len(kind))
    A = full(rng, 75, 75, "INT32")
    M = some_vmask(rng, 75, "INT8")
    assert (M.val[M.pres] == 0).any() and (M.val[M.pres] != 0).any() and not M.pres.all()
    W = vec(rng, "INT32", 75, rng.random(75) < 0.4)
    kw = dict(mask=M, struct=kind == "structural", comp=kind.startswith("complemented"), replace=kind.endswith("replace"))
    product(form, A, vec(rng, "INT32", 75), "PLUS_TIMES", "INT32", W=W, what=kind, **kw)
    product(form, A, vec(rng, "INT32", 75), "PLUS_TIMES", "INT32", what=kind + " empty w", **kw)


def test_accumulators_and_output_is_operand():
    rng = np.random.default_rng(2)
    A = full(rng, 75, 75, "INT32")
    W = vec(rng, "INT64", 75, rng.random(75) < 0.5)
    product("mxv", A, vec(rng, "INT32", 75), "PLUS_TIMES", "INT32", W=W, accum=("PLUS", "INT64"), what="accum of another type")
    W = vec(rng, "FP64", 75, rng.random(75) < 0.5)
    product("vxm", A, vec(rng, "INT32", 75), "PLUS_TIMES", "INT32", W=W, accum=("MINUS", "FP64"), mask=some_vmask(rng, 75, "BOOL"), what="accum + mask")
    for form in ("mxv", "vxm"):
        U = vec(rng, "INT32", 75, rng.random(75) < 0.8); dU = dev(U)
        product(form, A, U, "PLUS_TIMES", "INT32", dU=dU, W=U, dW=dU, what="out = u")
        U = vec(rng, "INT32", 75); dU = dev(U, full=True)
        product(form, A, U, "MIN_PLUS", "INT32", dU=dU, W=U, dW=dU, accum=("MIN", "INT32"), what="out = u, accumulated")


def test_pending_fill_then_accumulating_product():
    """`w[:] = s` that was requested and not written yet, then `w += A u` with the monoid's operator: the sparse path folds the fill into its store; here it is
    written first and the write-back reads it."""
    rng = np.random.default_rng(4)
    A = full(rng, 80, 70, "FP32"); U = vec(rng, "FP32", 70)
    for form, AA, UU, m in (("mxv", A, U, 80), ("vxm", A, vec(rng, "FP32", 80), 70)):
        W = VM.Vec(np.full(m, 0.25, np.float32), np.ones(m, bool))
        dW = gb.Vector.sparse(gb.FP32, m)
        dW[:] = 0.25
        product(form, AA, UU, "PLUS_TIMES", "FP32", W=W, dW=dW, accum=("PLUS", "FP32"), what="pending fill")


@pytest.mark.parametrize("form", ["mxv", "mxv_t", "vxm", "vxm_t"])
def test_descriptors(form):
    """mxv with T0 and vxm with T1, each on both layouts, on a matrix that is not square."""
    L = geometry()[2]
    rng = np.random.default_rng(11)
    A = full(rng, 9, L + 5, "FP64")
    k = A.ncols if FORMS[form] == "N" else A.nrows
    product(form, A, vec(rng, "FP64", k), "PLUS_TIMES", "FP64", what="descriptor")
    product(form, A, vec(rng, "FP64", k, rng.random(k) < 0.6), "MIN_PLUS", "FP64", what="descriptor, holes")


# ---- edits and routing ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_edits_on_the_full_operand():
    rng = np.random.default_rng(12)
    X = full(rng, 40, 70, "FP32"); dX = up_full(X)
    U = vec(rng, "FP32", 70)
    dX[4, 2] = 9.5                                                                # a queued edit on an HBM-only matrix: still full, and the product sees it
    Xe = MM.Mat(40, 70, X.keys, X.vals.copy()); Xe.vals[4 * 70 + 2] = 9.5
    product("mxv", Xe, U, "PLUS_TIMES", "FP32", dA=dX, what="set element")
    product("vxm", Xe, vec(rng, "FP32", 40), "PLUS_TIMES", "FP32", dA=dX, what="set element, T")
    del dX[11, 0]
    holed = MM.Mat(40, 70, np.delete(Xe.keys, 11 * 70), np.delete(Xe.vals, 11 * 70))
    product("mxv", holed, U, "PLUS_TIMES", "FP32", dA=dX, routed=False, what="removed element"); off_route("removed element")


def test_routing(monkeypatch):
    """Hooks unset: the default rule admits layout N with rows of at least MIN_INNER values from MINW entries (the measured wins) and nothing else.  The shapes at
    the threshold hold 2^24 values, so they are compared with the exact numpy product (values on the 1/8 grid: X u is exact in FP64 and in FP32), not through
    the entry-by-entry model."""
    MINW = geometry()[7]
    (r0, c), (r1, _) = default_rule_shapes(MINW)
    assert r0 * c < MINW <= r1 * c
    rng = np.random.default_rng(13)
    Xd = values(rng, "FP32", r1 * c).reshape(r1, c); ud = values(rng, "FP32", c); yd = values(rng, "FP32", r1)
    dX, dXs = gb.Matrix.from_dense(Xd), gb.Matrix.from_dense(Xd[:r0])
    dU = gb.Vector.from_dense_array(ud, gb.FP32); dY = gb.Vector.from_dense_array(yd, gb.FP32); dY0 = gb.Vector.from_dense_array(yd[:r0], gb.FP32)
    exp_n = (Xd.astype(np.float64) @ ud.astype(np.float64)).astype(np.float32); exp_t = (yd.astype(np.float64) @ Xd.astype(np.float64)).astype(np.float32)
    exp_t0 = (yd[:r0].astype(np.float64) @ Xd[:r0].astype(np.float64)).astype(np.float32)

    def same(w, exp, what):
        x, p = w.to_dense_arrays()
        assert (p != 0).all() and np.array_equal(x.view(np.uint32), exp.view(np.uint32)), f"{what} [{gb.last_kernel_plan()}]"

    monkeypatch.delenv("GRB_MI355X_GEMV")
    same(dX.mxv(dU, semiring=gb.FP32.PLUS_TIMES), exp_n, "above the threshold"); assert_route(r1, c, "N", holes=False, cast=False, what="above the threshold")
    same(dU.vxm(dX, semiring=gb.FP32.PLUS_TIMES, desc=desc_of(t1=True)), exp_n, "above the threshold, vxm T1"); assert_route(r1, c, "N", what="above the threshold, vxm T1")
    same(dXs.mxv(dU, semiring=gb.FP32.PLUS_TIMES), exp_n[:r0], "below the threshold"); off_route("below the threshold")
    same(dY.vxm(dX, semiring=gb.FP32.PLUS_TIMES), exp_t, "layout T"); off_route("layout T is not taken by itself")
    short = full(rng, 2 * r1, 64, "FP32")                                                                         # as many entries, short rows
    product("mxv", short, vec(rng, "FP32", 64), "PLUS_TIMES", "FP32", routed=False, what="short rows"); off_route("short rows")
    monkeypatch.setenv("GRB_MI355X_GEMV", "0")
    same(dX.mxv(dU, semiring=gb.FP32.PLUS_TIMES), exp_n, "hook 0"); off_route("hook 0")
    monkeypatch.setenv("GRB_MI355X_GEMV", "1")
    same(dXs.mxv(dU, semiring=gb.FP32.PLUS_TIMES), exp_n[:r0], "hook 1 below the threshold"); assert_route(r0, c, "N", what="hook 1 below the threshold")
    same(dY0.vxm(dXs, semiring=gb.FP32.PLUS_TIMES), exp_t0, "hook 1, layout T"); assert_route(c, r0, "T", what="hook 1, layout T")
    monkeypatch.setenv("GRB_MI355X_SPMV", "xcd")                                                                  # a kernel asked for by name keeps its route
    same(dX.mxv(dU, semiring=gb.FP32.PLUS_TIMES), exp_n, "SPMV=xcd"); off_route("SPMV=xcd")
    monkeypatch.delenv("GRB_MI355X_SPMV")
    S = sparse(rng, [int(x) for x in rng.integers(1, 4, 50)], 70, "FP32")                                         # a sparse A
    dS = up(S); dV = dev(vec(rng, "FP32", 70), full=True)
    dS.mxv(dV, semiring=gb.FP32.PLUS_TIMES); off_route("sparse A")
    dF = up_full(full(rng, 50, 70, "INT64")); dV = dev(vec(rng, "INT64", 70), full=True)
    dF.mxv(dV, semiring=gb.INT64.MIN_SECONDI); off_route("positional semiring")                                   # an off-table semiring
    H = gb.Matrix.sparse(gb.FP32, 1 << 40, 1 << 40); H[3, 5] = 1.0                                                # a hypersparse operand: its compacted 1 x 1 form is full
    hv = gb.Vector.sparse(gb.FP32, 1 << 40); hv[5] = 2.0
    H.mxv(hv, semiring=gb.FP32.PLUS_TIMES); off_route("hypersparse")


def test_no_transposed_image_after_a_routed_vxm(monkeypatch):
    """GxB_Matrix_memoryUsage counts the cached transpose's arrays: it reports the same bytes after a routed vxm and a routed mxv under T0 as before, and more once
    the old route (hook 0) has built the transposed copy."""
    rng = np.random.default_rng(14)
    X = full(rng, 300, 70, "FP32"); dX = up_full(X)
    size = C.c_size_t(0)

    def usage():
        assert gb.lib.GxB_Matrix_memoryUsage(C.byref(size), dX._h) == 0
        return size.value

    before = usage()
    product("vxm", X, vec(rng, "FP32", 300), "PLUS_TIMES", "FP32", dA=dX, what="no transpose")
    product("mxv_t", X, vec(rng, "FP32", 300), "PLUS_TIMES", "FP32", dA=dX, what="no transpose, T0")
    assert usage() == before
    monkeypatch.setenv("GRB_MI355X_GEMV", "0")
    product("vxm", X, vec(rng, "FP32", 300), "PLUS_TIMES", "FP32", dA=dX, routed=False, what="old route")
    assert usage() > before


# ---- floating-point order: normal random values ----------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("layout", ["N", "T"])
@pytest.mark.parametrize("k", ["1000", "2chunk+1"])
@pytest.mark.parametrize("typ", ["FP32", "FP64"])
def test_floating_point_order(typ, k, layout):
    """Each output within 2 k u sum_l |a u| of the exact dot product (FP32: the FP64 product; FP64: math.fsum) — the any-order bound, doubled for a possible fused
    multiply-add; the same call gives the same bits twice; the same inner vector planted at several outer positions (rows 0, 1, 2 and m - 1 — aligned and
    unaligned addresses for odd k — or columns in different lanes, packets and slabs) gives the same bits; and the same bits again in a matrix of another outer
    length; with holes in u as well."""
    LOAD, _, L, _, _, RT, _, _, _ = geometry()
    k = 1000 if k == "1000" else 2 * (L if layout == "N" else RT) + 1
    u_ = 2.0 ** -24 if typ == "FP32" else 2.0 ** -53
    V = pack(NP[typ]().itemsize)
    rng = np.random.default_rng(k)
    inner = rng.standard_normal(k).astype(NP[typ])
    sr = getattr(TYPE[typ], "PLUS_TIMES")

    def run(m, places, U):
        Md = rng.standard_normal((m, k)).astype(NP[typ])
        Md[places] = inner
        Ad = Md if layout == "N" else np.ascontiguousarray(Md.T)
        dA = gb.Matrix.from_dense(Ad); dU = dev(U, full=bool(U.pres.all()))
        outs = []
        for _ in range(2):
            w = dA.mxv(dU, semiring=sr) if layout == "N" else dU.vxm(dA, semiring=sr)
            assert_route(m, k, layout, holes=not U.pres.all(), cast=False, what="order")
            x, p = w.to_dense_arrays(); assert (p != 0).all()
            outs.append(x)
        assert np.array_equal(bits(outs[0]), bits(outs[1])), "two runs differ"
        return Md, outs[0]

    for pres in (np.ones(k, bool), rng.random(k) < 0.5):
        U = VM.Vec(rng.standard_normal(k).astype(NP[typ]), pres)
        m1 = 64 * V + V + 3 if layout == "T" else 9                               # T: V does not divide it (one value a lane) ...
        places1 = [0, 1, 2, m1 - 1]
        Md, x = run(m1, places1, U)
        uv = np.where(pres, U.val, 0).astype(np.float64)
        terms_abs = np.abs(Md.astype(np.float64)) @ np.abs(uv)
        exact = Md.astype(np.float64) @ uv if typ == "FP32" else np.array([math.fsum(float(a) * float(b) for a, b in zip(row, uv)) for row in Md])
        err = np.abs(x.astype(np.float64) - exact); bound = 2 * k * u_ * terms_abs
        print(f"{typ} {layout} k={k} holes={not pres.all()}: largest error / bound = {float((err / bound).max()):.3g}")
        assert (err <= bound).all(), (typ, k, int(np.argmax(err - bound)))
        same = [x[p] for p in places1]
        assert all(bits(v).tolist() == bits(same[0]).tolist() for v in same), f"one inner vector, several outer positions: {same}"
        m2 = 128 * V if layout == "T" else 4                                      # ... and V divides it (16-byte packets): another outer length
        places2 = [0, 3, m2 - 1] if layout == "N" else [0, V + 1, 64 * V + 2, m2 - 1]
        _, x2 = run(m2, places2, U)
        assert all(bits(x2[p]).tolist() == bits(same[0]).tolist() for p in places2), f"another outer length: {same[0]} {[x2[p] for p in places2]}"
