"""The product with a full right operand (the spmm_full route of GrB_mxm: grb_spmm.hip, grb_spmm_kernels.hpp) against the numpy model of tests/product_model.py, BIT
FOR BIT on `to_csr()` (row pointers, columns, values), and Matrix.from_dense / to_dense_tensor / is_full (GrBX_Matrix_import_Full / export_Full).

Every edge is read from GrBX_spmm_geometry: L = entries per piece (longer rows are cut into chunks), SLAB = columns per slab of the wide kernel, WAVES and CAP =
waves per workgroup and the grid cap, MINP = the products from which the route is taken by itself.  Floating-point values lie on the 1/8 grid without zeros, so
every summation order is exact; the narrow integer types carry their extremes (they wrap, in any order alike).  Cases run with GRB_MI355X_FULL=1 unless they are
about the default rule, and every case asserts the plan string — `spmm_full<k=K,group=G,slabs=S,long=N,...` with the values the case was built for — so that a
case that went another way fails instead of passing."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import matrix_model as MM
import product_model as PM
import pygraphblas_amd as gb
from helpers import TYPE, rand_values
from test_matrix_kernels_at_size_gpu import check, desc_of

pytestmark = pytest.mark.gpu
NP = MM.NP
REAL = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]


@functools.lru_cache(maxsize=None)
def geometry():
    out = (C.c_uint64 * 5)()
    assert gb.lib.GrBX_spmm_geometry(out) == 0
    return tuple(int(v) for v in out)              # L, SLAB, WAVES, CAP, MINP


@pytest.fixture(autouse=True)
def route_hook(gpu, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_FULL", "1")
    for name in ("GRB_MI355X_DETERMINISTIC", "GRB_MI355X_SPGEMM", "GRB_MI355X_MXM_ROWS", "GRB_MI355X_BATCH"):
        monkeypatch.delenv(name, raising=False)


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------------------
def values(rng, typ, n):
    x = rand_values(rng, typ, n)
    if typ.startswith("FP"):
        x[x == 0] = 0.125
    elif typ in ("INT8", "UINT8", "INT16", "UINT16") and n:
        i = np.iinfo(NP[typ]); at = rng.random(n) < 1 / 16
        x[at] = rng.choice(np.array([i.min, i.max, i.max - 1], NP[typ]), size=int(at.sum()))
    return x


def sparse(rng, lens, ncols, typ):
    """Rows of the given lengths, the columns of each drawn without repetition."""
    keys = [r * ncols + np.sort(rng.choice(ncols, size=int(n), replace=False)) for r, n in enumerate(lens) if n]
    keys = np.concatenate(keys).astype(np.int64) if keys else np.zeros(0, np.int64)
    return MM.Mat(len(lens), ncols, keys, values(rng, typ, len(keys)))


def full(rng, n, k, typ):
    return MM.Mat(n, k, np.arange(n * k, dtype=np.int64), values(rng, typ, n * k))


def up(m):
    if m.nvals == 0:
        return gb.Matrix.sparse(TYPE[m.typ], m.nrows, m.ncols)
    return gb.Matrix.from_arrays(m.rows.astype(np.uint64), m.cols.astype(np.uint64), m.vals, m.nrows, m.ncols, TYPE[m.typ])


def up_full(m):
    """A full model matrix through from_dense: it lives in HBM only."""
    assert m.nvals == m.nrows * m.ncols
    return gb.Matrix.from_dense(m.vals.reshape(m.nrows, m.ncols))


def pow2ceil(k):
    g = 1
    while g < k: g *= 2
    return g


PLAN = re.compile(r"^spmm_full<k=(\d+),group=(\d+),slabs=(\d+),long=(\d+),cast=([01])> ")


def assert_route(k, nlong, cast=None, what=""):
    """The plan of the last product: the route, and the shape it reports for k columns and `nlong` split rows."""
    L, SLAB = geometry()[:2]
    plan = gb.last_kernel_plan() + " "
    m = PLAN.match(plan)
    assert m, f"{what}: not on the spmm_full route: {plan}"
    got = tuple(int(v) for v in m.groups())
    group, slabs = (pow2ceil(k), 1) if k <= 64 else (0, -(-k // SLAB))
    assert got[:4] == (k, group, slabs, nlong), f"{what}: {plan}"
    assert ("k_spmm_narrow " in plan) == (k <= 64) and ("k_spmm_wide " in plan) == (k > 64) and ("k_spmm_fold " in plan) == (nlong > 0), plan
    if cast is not None:
        assert got[4] == int(cast), plan


def nlong_of(A):
    L = geometry()[0]
    return int((np.bincount(A.rows, minlength=A.nrows) > L).sum())


def product(A, B, sr, typ, dA=None, dB=None, C=None, dC=None, mask=None, dM=None, struct=False, comp=False, replace=False, accum=None, t0=False, t1=False, routed=True, cast=None,
            what=""):
    """dA.mxm(dB) into dC (a fresh matrix of the semiring's type when not given) against the model; `accum` = (operator, type).  `routed`: assert the route."""
    add, mul = sr.split("_")
    dA = up(A) if dA is None else dA; dB = up(B) if dB is None else dB
    opA = MM.transpose(A) if t0 else A; opB = MM.transpose(B) if t1 else B
    if C is None:
        C = MM.empty(opA.nrows, opB.ncols, typ)
    if dC is None:
        dC = up(C)
    if mask is not None and dM is None:
        dM = up(mask)
    exp = PM.mxm(C, A, B, add, mul, typ, mask=mask, struct=struct, comp=comp, replace=replace, accum=accum, tran_a=t0, tran_b=t1)
    dA.mxm(dB, semiring=getattr(TYPE[typ], sr), mask=dM, out=dC, accum=getattr(TYPE[accum[1]], accum[0]) if accum else None, desc=desc_of(replace, struct, comp, t0, t1))
    what = f"{what} {typ}.{sr} k={opB.ncols}"
    if routed:
        assert_route(opB.ncols, nlong_of(opA), cast, what)
    check(dC, exp, what)
    return dC, exp


# ---- column widths ----------------------------------------------------------------------------------------------------------------------------------------------
def widths():
    return [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, "slab+1", "2slab+1"]


@functools.lru_cache(maxsize=None)
def width_A(typ):
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 40] * 32 + [40, 0]                      # 130 rows: more than one wave of rows at G = 1
    return sparse(rng, lens, 50, typ)


@pytest.mark.parametrize("k", widths())
@pytest.mark.parametrize("typ,sr", [("FP32", "PLUS_TIMES"), ("INT64", "MIN_PLUS")])
def test_column_widths(typ, sr, k):
    SLAB = geometry()[1]
    k = {"slab+1": SLAB + 1, "2slab+1": 2 * SLAB + 1}.get(k, k)
    A = width_A(typ); assert A.nrows == 130
    B = full(np.random.default_rng(k), 50, k, typ)
    product(A, B, sr, typ, dB=up_full(B), what="widths")


# ---- row lengths ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 65])
@pytest.mark.parametrize("shape", ["edges", "no_entries", "no_empty_row"])
def test_row_lengths(shape, k):
    L = geometry()[0]
    lens = {"edges": [0, 1, 2, L - 1, L, L + 1, 2 * L + 1, 0], "no_entries": [0] * 9, "no_empty_row": [1, 2, L - 1, L, L + 1, 2 * L + 1]}[shape]
    rng = np.random.default_rng(len(lens) + k)
    A = sparse(rng, lens, 2 * L + 5, "FP32"); B = full(rng, 2 * L + 5, k, "FP32")
    assert nlong_of(A) == (0 if shape == "no_entries" else 2)
    dC, exp = product(A, B, "PLUS_TIMES", "FP32", what=shape)
    assert exp.nvals == k * sum(1 for n in lens if n)
    product(A, B, "MIN_PLUS", "FP32", what=shape)


def test_past_one_grid_round():
    """k = 1 (64 rows per wave): one row more than the capped grid takes in one round, one entry per row."""
    L, SLAB, WAVES, CAP, _ = geometry()
    m = CAP * WAVES * 64 + 1; n = 7
    rng = np.random.default_rng(5)
    A = MM.Mat(m, n, np.arange(m, dtype=np.int64) * n + rng.integers(0, n, m), values(rng, "INT32", m))
    B = full(rng, n, 1, "INT32")
    dC, exp = product(A, B, "PLUS_TIMES", "INT32", what="grid round")
    assert exp.nvals == m


# ---- every type and semiring ----------------------------------------------------------------------------------------------------------------------------------
def type_cases():
    out = []
    for typ in PM.MXM_TYPES:
        srs = list(PM.mxm_semirings(typ))
        srs += ["ANY_PAIR"] if typ == "BOOL" else [s for s in ("PLUS_PAIR", "MAX_FIRST", "MIN_SECOND") if s not in srs]
        out += [(typ, s) for s in srs]
    return out


@pytest.mark.parametrize("typ,sr", type_cases())
def test_every_type_and_semiring(typ, sr):
    L = geometry()[0]
    rng = np.random.default_rng(sum(map(ord, typ + sr)))
    lens = [0, 3, L, L + 1, 1, 2 * L + 3, 0, 2]
    A = sparse(rng, lens, 2 * L + 9, typ)
    for k in (5, 70):
        B = full(rng, 2 * L + 9, k, typ)
        product(A, B, sr, typ, cast=False, what="types")


@pytest.mark.parametrize("typ", ["INT32", "FP64"])
def test_any_second_of_constant_columns(typ):
    """ANY may keep any product: with SECOND and column j of B constant c_j != 0 every choice is c_j — and an accumulator padded with an identity would show."""
    L = geometry()[0]
    rng = np.random.default_rng(3)
    A = sparse(rng, [0, 1, L, L + 2, 7, 3 * L + 1], 3 * L + 4, typ)
    for k in (6, 80):
        c = np.arange(1, k + 1).astype(NP[typ]) * (1 if typ == "INT32" else 0.5)
        B = MM.Mat(A.ncols, k, np.arange(A.ncols * k, dtype=np.int64), np.tile(c, A.ncols))
        product(A, B, "ANY_SECOND", typ, what="any")


def test_mixed_operand_types():
    """A INT32, B FP64, an FP32 semiring: both operands are cast."""
    L = geometry()[0]
    rng = np.random.default_rng(8)
    A = sparse(rng, [2, 0, L + 1, 5], L + 6, "INT32"); B = full(rng, L + 6, 4, "FP64")
    product(A, B, "PLUS_TIMES", "FP32", cast=True, what="mixed")
    product(A, B, "PLUS_PAIR", "FP32", cast=False, what="mixed pair")          # (PAIR reads neither side: nothing to cast)


# ---- descriptor and write-back --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wb_operands():
    L = geometry()[0]
    rng = np.random.default_rng(21)
    n = L + 8
    A = sparse(rng, [3, 0, L + 2, 1, 0, 9, 40, 2, 0], n, "INT32")
    return A, full(rng, n, 6, "INT32"), rng


def some_mask(rng, nr, nc, typ, density=0.5):
    keys = np.flatnonzero(rng.random(nr * nc) < density).astype(np.int64)
    vals = rng.choice(np.array([0, 1, 3], NP[typ]), size=len(keys)) if typ != "BOOL" else rng.random(len(keys)) < 0.6
    return MM.Mat(nr, nc, keys, vals)


def test_transposed_operands():
    A, B, rng = wb_operands()
    At = MM.transpose(A); Bt = MM.transpose(B)
    product(At, B, "PLUS_TIMES", "INT32", t0=True, what="T0")
    product(A, Bt, "PLUS_TIMES", "INT32", t1=True, what="T1")                  # B given as k x n: a full matrix transposed is full
    product(At, Bt, "MIN_PLUS", "INT32", t0=True, t1=True, what="T0T1")


@pytest.mark.parametrize("kind", ["valued", "structural", "complemented", "replace", "complemented_replace"])
def test_masks(kind):
    A, B, rng = wb_operands()
    rng = np.random.default_rng(len(kind))
    M = some_mask(rng, A.nrows, B.ncols, "INT8")
    assert (M.vals == 0).any() and (M.vals != 0).any()
    keys = np.flatnonzero(rng.random(A.nrows * B.ncols) < 0.4).astype(np.int64)
    C = MM.Mat(A.nrows, B.ncols, keys, values(rng, "INT32", len(keys)))
    product(A, B, "PLUS_TIMES", "INT32", C=C, mask=M, struct=kind == "structural", comp=kind.startswith("complemented"), replace=kind.endswith("replace"), what=kind)
    product(A, B, "PLUS_TIMES", "INT32", mask=M, struct=kind == "structural", comp=kind.startswith("complemented"), replace=kind.endswith("replace"), what=kind + " empty C")


def test_accumulator_of_another_type():
    A, B, rng = wb_operands()
    rng = np.random.default_rng(2)
    keys = np.flatnonzero(rng.random(A.nrows * B.ncols) < 0.5).astype(np.int64)
    C = MM.Mat(A.nrows, B.ncols, keys, values(rng, "INT64", len(keys)))
    product(A, B, "PLUS_TIMES", "INT32", C=C, accum=("PLUS", "INT64"), what="accum")
    C = MM.Mat(A.nrows, B.ncols, keys, values(rng, "FP64", len(keys)))
    product(A, B, "PLUS_TIMES", "INT32", C=C, accum=("MINUS", "FP64"), mask=some_mask(rng, A.nrows, B.ncols, "BOOL"), what="accum + mask")


def test_output_is_an_operand():
    rng = np.random.default_rng(4)
    n = 40
    A = sparse(rng, [int(x) for x in rng.integers(0, 9, n)], n, "FP64"); B = full(rng, n, n, "FP64")
    dB = up_full(B)
    product(A, B, "PLUS_TIMES", "FP64", dB=dB, C=B, dC=dB, what="C is B")
    dA = up(A)
    product(A, B, "PLUS_TIMES", "FP64", dA=dA, C=A, dC=dA, what="C is A")


# ---- routing, hook unset --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def routing_operands():
    MINP = geometry()[4]
    rng = np.random.default_rng(31)
    rows = -(-MINP // (8 * 40)) + 1                            # rows of 40 entries: nnz 8 >= MINP > nnz 2
    A = sparse(rng, [40] * rows, 64, "FP32")
    assert A.nvals * 8 >= MINP > A.nvals * 2
    return A, full(rng, 64, 8, "FP32"), full(rng, 64, 2, "FP32")


def off_route(what):
    plan = gb.last_kernel_plan()
    assert "spmm_full<" not in plan, f"{what}: {plan}"


def test_default_rule(monkeypatch):
    A, B8, B2 = routing_operands()
    dA = up(A)
    monkeypatch.delenv("GRB_MI355X_FULL")
    product(A, B8, "PLUS_TIMES", "FP32", dA=dA, what="above the threshold")                                   # asserts the route
    rng = np.random.default_rng(6)
    M = some_mask(rng, A.nrows, 8, "BOOL")
    product(A, B8, "PLUS_TIMES", "FP32", dA=dA, mask=M, routed=False, what="plain mask"); off_route("plain mask")
    product(A, B8, "PLUS_TIMES", "FP32", dA=dA, mask=M, comp=True, what="complemented mask")                  # on the route
    holed = MM.Mat(B8.nrows, B8.ncols, np.delete(B8.keys, 77), np.delete(B8.vals, 77))
    product(A, holed, "PLUS_TIMES", "FP32", dA=dA, routed=False, what="one entry of B missing"); off_route("B not full")
    product(A, B2, "PLUS_TIMES", "FP32", dA=dA, routed=False, what="below the threshold"); off_route("below the threshold")
    monkeypatch.setenv("GRB_MI355X_FULL", "0")
    product(A, B8, "PLUS_TIMES", "FP32", dA=dA, routed=False, what="hook 0"); off_route("hook 0")
    monkeypatch.setenv("GRB_MI355X_FULL", "1")
    product(A, B2, "PLUS_TIMES", "FP32", dA=dA, what="hook 1 below the threshold")
    product(A, B8, "PLUS_TIMES", "FP32", dA=dA, mask=M, what="hook 1 with a plain mask")
    product(A, holed, "PLUS_TIMES", "FP32", dA=dA, routed=False, what="hook 1, B not full"); off_route("hook 1, B not full")


# ---- pending edits, chains, run to run ------------------------------------------------------------------------------------------------------------------------
def test_pending_edits_on_a_full_operand():
    rng = np.random.default_rng(9)
    A = sparse(rng, [3, 0, 5, 1, 12], 20, "FP64"); B = full(rng, 20, 7, "FP64")
    dB = up_full(B)
    dB[4, 2] = 9.5                                                             # a queued edit on an HBM-only matrix: still full
    B.vals[4 * 7 + 2] = 9.5
    assert dB.is_full
    product(A, B, "PLUS_TIMES", "FP64", dB=dB, what="set element")
    del dB[11, 0]
    holed = MM.Mat(20, 7, np.delete(B.keys, 11 * 7), np.delete(B.vals, 11 * 7))
    product(A, holed, "PLUS_TIMES", "FP64", dB=dB, routed=False, what="removed element"); off_route("removed element")
    assert not dB.is_full


def test_chains():
    rng = np.random.default_rng(10)
    n = 30
    A = sparse(rng, [int(x) for x in rng.integers(1, 4, n)], n, "INT64"); H = full(rng, n, 5, "INT64")
    dA, dH = up(A), up_full(H)
    for step in range(3):
        dH, H = product(A, H, "PLUS_TIMES", "INT64", dA=dA, dB=dH, what=f"chain step {step}")
        assert dH.is_full and H.nvals == n * 5
    lens = [int(x) for x in rng.integers(1, 4, n)]; lens[7] = 0
    A = sparse(rng, lens, n, "INT64"); dA = up(A)
    dH, H = product(A, H, "PLUS_TIMES", "INT64", dA=dA, dB=dH, what="empty row, first product")
    assert not dH.is_full and H.nvals == (n - 1) * 5
    product(A, H, "PLUS_TIMES", "INT64", dA=dA, dB=dH, routed=False, what="empty row, second product"); off_route("second product")


def test_run_to_run():
    """Rows of 4 L entries, rng.random values: the sums round, and the fixed order makes two runs agree in every bit."""
    L = geometry()[0]
    rng = np.random.default_rng(12)
    n = 4 * L + 3
    lens = [4 * L, 4 * L, 17, 4 * L]
    keys = np.concatenate([r * n + np.sort(rng.choice(n, size=k, replace=False)) for r, k in enumerate(lens)]).astype(np.int64)
    dA = up(MM.Mat(len(lens), n, keys, rng.random(len(keys)).astype(np.float32)))
    for k in (9, 100):
        Bd = rng.random((n, k)).astype(np.float32); dB = gb.Matrix.from_dense(Bd)
        runs = []
        for _ in range(2):
            c = dA.mxm(dB, semiring=gb.FP32.PLUS_TIMES)
            assert_route(k, 3, what="run to run")
            runs.append(c.to_csr())
        for a, b in zip(*runs):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        dense = np.zeros((len(lens), n), np.float64); dense[keys // n, keys % n] = dA.to_csr()[2]
        assert np.allclose(runs[0][2].reshape(len(lens), k), dense @ Bd.astype(np.float64), rtol=1e-4)      # 1 024 float32 terms


# ---- from_dense / to_dense_tensor / is_full -------------------------------------------------------------------------------------------------------------------
def dense_values(typ, nr, nc):
    rng = np.random.default_rng(nr * nc)
    if typ == "BOOL": return rng.random((nr, nc)) < 0.5
    if typ.startswith("FP"):
        x = rng.standard_normal((nr, nc)).astype(NP[typ]); x[0, 0] = -0.0; x[1, 2] = np.nan; x[2, 1] = np.inf
        return x
    i = np.iinfo(NP[typ]); x = rng.integers(i.min, i.max, (nr, nc), endpoint=True, dtype=NP[typ]); x[0, 0] = i.min; x[1, 1] = i.max
    return x


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("typ", REAL)
def test_dense_round_trip(typ):
    import torch
    from pygraphblas_amd.matrix import _torch_dtype
    X = dense_values(typ, 37, 5)
    for src in ("numpy", "gpu"):
        if src == "numpy":
            m = gb.Matrix.from_dense(X)
        else:
            m = gb.Matrix.from_dense(torch.from_numpy(X.view(np.uint8).reshape(37, -1)).cuda().view(_torch_dtype(TYPE[typ])))
        assert gb.last_kernel_plan().startswith("import_full<rows=37,cols=5> k_full_pattern"), src
        assert m.type is TYPE[typ] and (m.nrows, m.ncols, m.nvals) == (37, 5, 185) and m.is_full, src
        t = m.to_dense_tensor()
        assert t.is_cuda and tuple(t.shape) == (37, 5) and t.dtype == _torch_dtype(TYPE[typ])
        assert np.array_equal(bits(t.cpu().view(torch.uint8).numpy()), bits(X)), src
        I, J = np.divmod(np.arange(185, dtype=np.uint64), np.uint64(5))
        ref = gb.Matrix.from_arrays(I, J, X.ravel(), 37, 5, TYPE[typ])
        for a, b in zip(m.to_csr(), ref.to_csr()):
            assert np.array_equal(bits(a), bits(b)), src


def test_dense_odds_and_ends():
    import torch
    base = torch.arange(60, dtype=torch.float32, device="cuda").reshape(6, 10)
    view = base.t()[1:9:2]                                    # 4 x 6, neither contiguous nor at the base address
    assert not view.is_contiguous()
    m = gb.Matrix.from_dense(view)
    assert np.array_equal(m.to_dense_tensor().cpu().numpy(), view.cpu().numpy())
    m = gb.Matrix.from_dense(np.arange(12.0).reshape(3, 4)[:, ::2])
    assert m.type is gb.FP64 and np.array_equal(m.to_csr()[2], [0, 2, 4, 6, 8, 10])
    m = gb.Matrix.from_dense(np.arange(6).reshape(2, 3), gb.FP32)             # a numpy array is cast to the type asked for
    assert m.type is gb.FP32 and m.to_dense_tensor().dtype == torch.float32
    del m[1, 1]
    assert not m.is_full
    with pytest.raises(gb.InvalidValue):
        m.to_dense_tensor()
    with pytest.raises(TypeError):                            # (the package has no complex type objects; the entry point's own refusal: test_spmm_full_host.py)
        gb.Matrix.from_dense(np.zeros((2, 2), np.complex64))
    h = C.c_void_p(); x = np.zeros(8)
    assert gb.lib.GrBX_Matrix_import_Full(C.byref(h), C.c_void_p(gb._capi.handle("GxB_FC64")), C.c_uint64(2), C.c_uint64(2), x.ctypes.data_as(C.c_void_p), 0) == 7      # GrB_DOMAIN_MISMATCH
    e = gb.Matrix.from_dense(torch.zeros((0, 5), dtype=torch.int16, device="cuda"))
    assert e.type is gb.INT16 and (e.nrows, e.ncols, e.nvals) == (0, 5, 0) and tuple(e.to_dense_tensor().shape) == (0, 5)
