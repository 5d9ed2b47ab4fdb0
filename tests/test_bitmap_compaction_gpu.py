"""The bitmap-compaction primitive (grb_compact.hip: present_positions / scatter_present) through the routes whose values it now moves as words and that no
other test runs at these widths or sizes: the few-rows product and the few-rows element-wise operations at 1- and 2-byte types, the batch bitmap-to-CSR past
its grid cap (8192 x 256 positions), and the push product's operand list past its cap (4096 x 256).  Every expected result is computed in numpy on dense
arrays: csr_compact sits under the generic routes too, so a device-against-device comparison could hide a shared mistake.  Values are small integers (floats
on a 1/8 grid), so every sum is exact and the comparison is bit for bit.  Row / column assign and diag at length 257 in all four widths are covered by
test_assign_gpu.py, test_index_lists_gpu.py and test_diag_gpu.py."""
import numpy as np
import pytest

from oracle import oracle as O
import pygraphblas_amd as gb
from pygraphblas_amd import descriptor as D
from helpers import TYPE

pytestmark = pytest.mark.gpu
NP = O.NP


# ---- dense models ------------------------------------------------------------------------------------------------------------------------------------------
def values(rng, typ, shape):
    if typ == "BOOL": return rng.random(shape) < 0.8
    if typ.startswith("FP"): return (rng.integers(1, 17, shape) / 8.0).astype(NP[typ])
    return rng.integers(1, 4, shape).astype(NP[typ])


def upload(typ, val, pres):
    I, J = np.nonzero(pres)
    return gb.Matrix.from_arrays(I.astype(np.uint64), J.astype(np.uint64), np.ascontiguousarray(val[pres]), pres.shape[0], pres.shape[1], TYPE[typ])


def same(got, typ, val, pres, what):
    """`got` holds exactly the entries of the dense model (val, pres), row-major with ascending columns, bit for bit."""
    I, J, X = got.to_arrays(); ei, ej = np.nonzero(pres)
    assert got.type.__name__ == typ and (got.nrows, got.ncols) == pres.shape, what
    assert got.nvals == len(ei) and np.array_equal(I, ei.astype(np.uint64)) and np.array_equal(J, ej.astype(np.uint64)), f"pattern differs: {what}"
    assert X.dtype == NP[typ] and np.array_equal(X, val[pres].astype(NP[typ])), f"values differ: {what}"


# ---- the few-rows product ----------------------------------------------------------------------------------------------------------------------------------
K = 300


def product_operands(typ, ncols, seed, empty=False):
    """A is 3 x 300 with row 1 empty; B is 300 x ncols.  Result row 0 holds the first and the last column, row 2 every column (B's rows 10 .. 19 cover
    them, rows 10 and 11 twice: sums of two products).  `empty`: A's entries meet only rows of B that hold nothing."""
    rng = np.random.default_rng(seed)
    ap = np.zeros((3, K), bool); bp = np.zeros((K, ncols), bool)
    bp[5, 0] = True; bp[7, ncols - 1] = True; bp[7, 0] = True
    for j in range(10): bp[10 + j, j::10] = True
    bp[10, :] |= bp[11, :]
    bp[20:100] = rng.random((80, ncols)) < 0.1                           # rows no entry of A meets
    if empty: ap[0, [100, 150]] = True; ap[2, 200:210] = True            # (B's rows from 100 on are empty)
    else: ap[0, [5, 7]] = True; ap[2, 10:20] = True
    return values(rng, typ, ap.shape), ap, values(rng, typ, bp.shape), bp


def product_model(typ, av, ap, bv, bp):
    pres = (ap.astype(np.int64) @ bp.astype(np.int64)) > 0
    if typ == "BOOL": return ((av & ap).astype(np.int64) @ (bv & bp).astype(np.int64)) > 0, pres
    return (np.where(ap, av, 0).astype(np.float64) @ np.where(bp, bv, 0).astype(np.float64)).astype(NP[typ]), pres      # (sums below 2^12 on a 1/64 grid: exact)


@pytest.mark.parametrize("ncols", [257, 1])
@pytest.mark.parametrize("typ,sr", [("BOOL", "LOR_LAND"), ("INT16", "PLUS_TIMES"), ("FP32", "PLUS_TIMES"), ("INT64", "PLUS_TIMES")])
def test_few_rows_product_every_width(gpu, typ, sr, ncols, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_MXM_ROWS", "1")
    for empty in (False, True):
        av, ap, bv, bp = product_operands(typ, ncols, 11 + ncols, empty)
        got = upload(typ, av, ap).mxm(upload(typ, bv, bp), semiring=getattr(TYPE[typ], sr))
        plan = gb.last_kernel_plan(); what = f"{typ}.{sr} ncols={ncols} empty={empty} plan={plan}"
        assert "mxm_rows<" in plan, what
        val, pres = product_model(typ, av, ap, bv, bp)
        if empty: assert not pres.any()
        else: assert pres[0, 0] and pres[0, ncols - 1] and pres[0].sum() == min(ncols, 2) and not pres[1].any() and pres[2].all()
        same(got, typ, val, pres, what)
        if empty:                                                        # 0 entries and a row pointer that the next operation can read
            again = got.eadd(got, getattr(TYPE[typ], "LOR" if typ == "BOOL" else "PLUS"))
            assert got.nvals == 0 and again.nvals == 0, what


# ---- the few-rows element-wise operations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", ["UINT8", "INT16", "FP32", "FP64"])
def test_few_rows_ewise_every_width(gpu, typ, monkeypatch):
    monkeypatch.setenv("GRB_MI355X_EWISE_ROWS", "1"); monkeypatch.setenv("GRB_MI355X_BATCH", "0")
    rng = np.random.default_rng(23); shape = (3, 257); plus = TYPE[typ].PLUS
    ap = rng.random(shape) < 0.4; bp = rng.random(shape) < 0.4
    ap[0, 0] = ap[2, 256] = bp[2, 256] = True; ap[1] = False; bp[1] = False; bp[1, 256] = True      # (row 1: one entry, in the second workgroup)
    av, bv = values(rng, typ, shape), values(rng, typ, shape)
    A, B = upload(typ, av, ap), upload(typ, bv, bp)
    tv = (np.where(ap, av, 0) + np.where(bp, bv, 0)).astype(NP[typ]); tp = ap | bp
    got = A.eadd(B, plus); plan = gb.last_kernel_plan()
    assert "ewise_rows<" in plan, plan
    same(got, typ, tv, tp, f"eadd {typ} plan={plan}")
    # two disjoint patterns: the intersection is empty
    B2 = upload(typ, bv, ~ap & bp)
    got = A.emult(B2, TYPE[typ].TIMES); plan = gb.last_kernel_plan()
    assert "ewise_rows<" in plan, plan
    same(got, typ, tv, np.zeros(shape, bool), f"emult of disjoint patterns {typ} plan={plan}")
    # C<!M, replace> = A + B over an existing C: what the mask's true entries cover goes, the rest is the sum
    cp = rng.random(shape) < 0.5; cv = values(rng, typ, shape); mp = rng.random(shape) < 0.6; mv = rng.random(shape) < 0.7
    Cm = upload(typ, cv, cp)
    A.eadd(B, plus, out=Cm, mask=upload("BOOL", mv, mp), desc=D.RC); plan = gb.last_kernel_plan()
    assert "ewise_rows<" in plan, plan
    same(Cm, typ, tv, tp & ~(mp & mv), f"eadd <!M, replace> {typ} plan={plan}")


# ---- a batch bitmap to CSR ---------------------------------------------------------------------------------------------------------------------------------
def batch_sum(typ, ap, bp, rng, monkeypatch, what):
    """A + B through the bitmap route (the result lives as a bitmap only), then its tuples: they are read from the CSR that mat_bitmap_to_csr makes."""
    monkeypatch.setenv("GRB_MI355X_BATCH", "1")
    av, bv = values(rng, typ, ap.shape), values(rng, typ, bp.shape)
    got = upload(typ, av, ap).eadd(upload(typ, bv, bp), TYPE[typ].PLUS); plan = gb.last_kernel_plan()
    assert "ewise_batch" in plan, (what, plan)
    same(got, typ, (np.where(ap, av, 0) + np.where(bp, bv, 0)).astype(NP[typ]), ap | bp, f"{what} plan={plan}")


@pytest.mark.parametrize("typ", ["UINT8", "INT16", "FP32", "INT64"])
def test_batch_bitmap_to_csr_every_width(gpu, typ, monkeypatch):
    rng = np.random.default_rng(31); shape = (2, 65536)                    # the smallest batch shape
    for empty_row in (None, 0, 1):
        ap = rng.random(shape) < 0.01; bp = rng.random(shape) < 0.01
        ap[0, 0] = True; bp[1, 65535] = True
        if empty_row is not None: ap[empty_row] = False; bp[empty_row] = False
        batch_sum(typ, ap, bp, rng, monkeypatch, f"{typ} 2 x 65536 empty row {empty_row}")


def test_batch_bitmap_to_csr_past_the_grid_cap(gpu, monkeypatch):
    """33 x 65 536 = 2 162 688 positions > 8192 workgroups x 256: the scatter's loop takes a second round, and the last position holds an entry."""
    rng = np.random.default_rng(37); shape = (33, 65536)
    assert shape[0] * shape[1] > 8192 * 256
    ap = rng.random(shape) < 0.01; bp = rng.random(shape) < 0.002
    ap[0, 0] = True; ap[32, 65535] = True; ap[16] = False; bp[16] = False
    batch_sum("UINT8", ap, bp, rng, monkeypatch, "UINT8 33 x 65536")


# ---- the push product's operand list -----------------------------------------------------------------------------------------------------------------------
def test_push_operand_list_past_the_grid_cap(gpu, monkeypatch):
    """n = 2^20 + 257 > 4096 workgroups x 256: the operand's first position, one of the second round and the last one are present; the matrix has one entry
    per row, so w = u lor.land A holds exactly the three columns of those rows."""
    n = (1 << 20) + 257; at = np.array([0, 1 << 20, n - 1])
    assert n > 4096 * 256
    rows = np.arange(n, dtype=np.uint64); cols = (rows * np.uint64(7) + np.uint64(3)) % np.uint64(n)      # (7 and n are coprime: a permutation)
    assert len(np.unique(cols[at])) == 3
    A = gb.Matrix.from_arrays(rows, cols, np.ones(n, np.bool_), n, n, gb.BOOL)
    pres = np.zeros(n, np.uint8); pres[at] = [1, 2, 255]                               # (any byte != 0 says "present")
    u = gb.Vector.from_dense_array(np.ones(n, np.bool_), gb.BOOL, present=pres)      # (no host list of the entries: the list is made on the device)
    monkeypatch.setenv("GRB_MI355X_SPMV", "push")
    w = u.vxm(A, semiring=gb.BOOL.LOR_LAND); plan = gb.last_kernel_plan()
    assert "k_spmspv_push<" in plan, plan
    I, X = w.to_arrays()
    assert np.array_equal(I, np.sort(cols[at])) and X.all() and len(X) == 3, plan
