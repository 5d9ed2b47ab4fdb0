"""Pins tests/product_model.py (the numpy model the GPU tests of the masked-pull and push SpMV kernels compare with) on the CPU against the oracle
(oracle/grb_oracle.c through O.mxv / O.vxm — never the library): random small products for every type, every semiring of test_mxv_vxm_gpu.SEMIRINGS, valued /
structural / complemented masks of four types, accumulators, replace, transposed descriptors, operands and outputs of other types than the semiring's, and
value pools that hold the monoids' terminals and identities (the types' extremes, 0, 1, +-inf).  Pattern and values must agree exactly (NaN equals NaN); no
case is skipped.  No test here needs the library's kernels or a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
import matrix_model as MM
import vector_model as VM
import product_model as PM
from test_mxv_vxm_gpu import ALL, SEMIRINGS, family

CASES_PER_TYPE = 60           # 660 cases in all, each as mxv or vxm


def pool(typ, sr, small):
    """The values a case draws from.  Integer quotients stay away from zero divisors and INT_MIN / -1 (matrix_model._idiv's contract)."""
    if typ == "BOOL": return np.array([False, True, True])
    t = MM.NP[typ]
    if "DIV" in sr and not typ.startswith("FP"):
        return np.array([1, 2, 3, 7, 50] if typ[0] == "U" or small else [1, 2, -3, 7, -50], t)
    if small: return np.array([0, 1, 2, 3], t)
    if typ.startswith("FP"):
        big = [] if sr.startswith("PLUS") else [np.finfo(t).max, -np.finfo(t).max]          # (a sum that overflows on the way depends on its order)
        return np.array([0, 1, -1, 0.125, -2.5, 7, np.inf, -np.inf] + big, t)
    i = np.iinfo(t)
    return np.array([0, 1, 2, 5, i.max, i.min, i.max - 1, i.min + 1] + ([] if typ[0] == "U" else [-1, -4]), t)


def rand_vec(rng, typ, n, dens, values):
    p = rng.random(n) < dens
    return VM.Vec(rng.choice(values, size=n).astype(MM.NP[typ]), p)


def tuples_of(v, row):
    at = np.flatnonzero(v.pres)
    return (O.row_vector if row else O.col_vector)(v.typ, v.n, at, v.val[at])


MASK_VALUES = {"BOOL": [False, True, True], "UINT8": [0, 0, 1, 200], "INT32": [0, 1, -3], "FP64": [0.0, 1.5, np.nan, -2.0, 0.0]}


@pytest.mark.parametrize("typ", ALL)
def test_model_agrees_with_the_oracle(typ):
    rng = np.random.default_rng(ALL.index(typ) + 900)
    srs = SEMIRINGS[family(typ)]
    seen = set()
    for case in range(CASES_PER_TYPE):
        sr = srs[case % len(srs)]; add, mul = sr.split("_")
        vxm, tran = bool(rng.integers(0, 2)), rng.random() < 0.4
        cast_case = case % 5 == 4                                                  # operands and output of other types, small values
        a_typ, u_typ, out_typ = (str(rng.choice(ALL)), str(rng.choice(ALL)), str(rng.choice(ALL))) if cast_case else (typ, typ, typ)
        if cast_case and "DIV" in sr: a_typ = u_typ = typ
        if typ.startswith("FP") and out_typ[0] == "U": out_typ = "INT" + out_typ[4:]      # (a negative floating-point value has no unsigned image)
        nr, nc = int(rng.choice([1, 2, 5, 9, 12])), int(rng.choice([1, 3, 8, 11]))
        vals = pool(typ, sr, cast_case)
        keys = np.flatnonzero(rng.random(nr * nc) < rng.choice([0.1, 0.4, 0.9]))
        A = MM.Mat(nr, nc, keys, rng.choice(vals, size=len(keys)).astype(MM.NP[a_typ]))
        eff_r, eff_c = (nc, nr) if tran else (nr, nc)
        n_in, n_out = (eff_r, eff_c) if vxm else (eff_c, eff_r)
        u = rand_vec(rng, u_typ, n_in, rng.choice([0.3, 0.7, 1.0]), vals)
        w = rand_vec(rng, out_typ, n_out, 0.4, pool(out_typ, sr, True) if cast_case else vals)
        mkind = str(rng.choice(["none", "valued", "structural", "complemented", "structural complemented"]))
        mtyp = str(rng.choice(list(MASK_VALUES)))
        mask = None if mkind == "none" else rand_vec(rng, mtyp, n_out, 0.6, np.array(MASK_VALUES[mtyp], MM.NP[mtyp]))
        struct, comp = "structural" in mkind, "complemented" in mkind
        replace = rng.random() < 0.4
        accum = None if rng.random() < 0.5 else ("LOR" if out_typ == "BOOL" else str(rng.choice(["PLUS", "MIN", "SECOND"])))
        seen |= {sr, mkind, "vxm" if vxm else "mxv", "tran" if tran else "plain", "accum" if accum else "no accum", "replace" if replace else "keep"}
        kw = dict(mask=mask, struct=struct, comp=comp, replace=replace, accum=(accum, out_typ) if accum else None, tran=tran)
        got = PM.vxm(w, u, A, add, mul, typ, **kw) if vxm else PM.mxv(w, A, u, add, mul, typ, **kw)
        At = O.Tuples(a_typ, nr, nc, A.rows, A.cols, A.vals)
        okw = dict(mask=None if mask is None else tuples_of(mask, vxm), accum=accum, accum_type=out_typ, replace=replace, mask_comp=comp, mask_struct=struct, tran_a=tran)
        exp = O.vxm(tuples_of(w, True), tuples_of(u, True), At, add, mul, typ, **okw) if vxm else O.mxv(tuples_of(w, False), At, tuples_of(u, False), add, mul, typ, **okw)
        what = (typ, case, sr, "vxm" if vxm else "mxv", tran, a_typ, u_typ, out_typ, mkind, mtyp, replace, accum)
        assert got.typ == out_typ and got.n == n_out, what
        at = np.flatnonzero(got.pres)
        assert np.array_equal(at, (exp.J if vxm else exp.I).astype(np.int64)), (what, at, exp.I, exp.J)
        assert np.array_equal(got.val[at], exp.X, equal_nan=out_typ.startswith("FP")), (what, got.val[at], exp.X)
    assert seen >= set(srs) | {"none", "valued", "structural", "complemented", "structural complemented", "vxm", "mxv", "tran", "plain", "accum", "no accum", "replace", "keep"}


def dense_vec(vals, pres, typ):
    return VM.Vec(np.array(vals, MM.NP[typ]), np.array(pres, bool))


def test_absent_operand_positions_and_terminals():
    """The rules the GPU tests lean on, by hand: an absent operand position contributes nothing (whatever value lies behind the hole), a row of absent
    contributions has no entry, the terminal of MIN is a value like any other, ANY takes the contribution with the largest column."""
    lo = np.iinfo(np.int32).min
    A = MM.from_coo(4, 3, [0, 0, 0, 1, 1, 3], [0, 1, 2, 0, 2, 1], [5, lo, 7, lo, 9, 4], "INT32")
    u = dense_vec([1, lo, 1], [True, False, True], "INT32")
    t = PM.product("MIN", "FIRST", "INT32", A, u)
    assert t.pres.tolist() == [True, True, False, False] and t.val[:2].tolist() == [5, lo]
    t = PM.product("ANY", "FIRST", "INT32", A, u)
    assert t.pres.tolist() == [True, True, False, False] and t.val[:2].tolist() == [7, 9]
    t = PM.product("MIN", "FIRST", "INT32", A, u, allow=np.array([True, False, True, True]))
    assert t.pres.tolist() == [True, False, False, False]
    u3 = dense_vec([2, 3, 4, 5], [True, True, False, True], "INT32")
    w = PM.vxm(VM.empty(3, "INT32"), u3, A, "PLUS", "MINUS", "INT32")                  # u(i) - A(i, j), summed over the present i
    w32 = lambda xs: np.array(xs, np.int64).astype(np.int32).tolist()                   # (sums with INT32_MIN wrap)
    assert w.pres.tolist() == [True, True, True] and w.val.tolist() == w32([(2 - 5) + (3 - lo), (2 - lo) + (5 - 4), (2 - 7) + (3 - 9)])
    w = PM.mxv(VM.empty(3, "INT32"), A, u3, "PLUS", "MINUS", "INT32", tran=True)        # A(i, j) - u(i)
    assert w.val.tolist() == w32([(5 - 2) + (lo - 3), (lo - 2) + (4 - 5), (7 - 2) + (9 - 3)])
    b = PM.product("EQ", "LOR", "BOOL", MM.from_coo(2, 3, [0, 0, 0, 1, 1], [0, 1, 2, 0, 1], [False, False, True, False, False], "BOOL"), dense_vec([False, False, False], [True, True, True], "BOOL"))
    assert b.val.tolist() == [True, True] and b.pres.all()                              # two false contributions: even


# ---- the masked matrix product (product_model.masked_mxm / mxm) --------------------------------------------------------------------------------------------------
from product_model import MXM_MASK_TYPES as MASK_TYPES, MXM_TYPES, mxm_semirings

MXM_CASES_PER_TYPE = 60          # 420 cases in all
MXM_MASK_VALUES = {"BOOL": [False, True], "INT8": [0, 1, -128], "UINT16": [0, 0, 256, 65535], "FP32": [0.0, -0.0, 1.5, np.nan], "INT64": [0, 1 << 32, -1],
                   "FP64": [0.0, -0.0, np.nan, -2.0, 2.0 ** -300]}


def rand_mat(rng, typ, nr, nc, dens, vals, empty_rows=True):
    keys = np.flatnonzero(rng.random(nr * nc) < dens)
    if empty_rows and nr > 1: keys = keys[keys // nc != rng.integers(0, nr)]                 # one row without entries
    return MM.Mat(nr, nc, keys, rng.choice(vals, size=len(keys)).astype(MM.NP[typ]))


def tuples_of_mat(m):
    return O.Tuples(m.typ, m.nrows, m.ncols, m.rows, m.cols, m.vals)


@pytest.mark.parametrize("typ", MXM_TYPES)
def test_masked_mxm_agrees_with_the_oracle(typ):
    """`C<M, replace> = accum(C, op(A) add.mul op(B))` of the model against O.mxm, exactly: every type and semiring of tests/test_spgemm_masked_at_size_gpu.py,
    valued and structural masks of its six mask types with false values, -0.0 and NaN, complemented masks (the write-back alone), rows without entries in A, B
    and M, transposed operands, accumulators and replace, values that wrap (the types' extremes)."""
    rng = np.random.default_rng(MXM_TYPES.index(typ) + 1900); srs = mxm_semirings(typ); seen = set()
    for case in range(MXM_CASES_PER_TYPE):
        sr = srs[case % len(srs)]; add, mul = sr.split("_")
        m, k, n = (int(rng.choice([1, 3, 7, 12])) for _ in range(3))
        ta, tb = rng.random() < 0.3, rng.random() < 0.3
        vals = pool(typ, sr, typ.startswith("FP"))                                  # (floating point: small values, so that every sum is exact in any order)
        A = rand_mat(rng, typ, *((k, m) if ta else (m, k)), rng.choice([0.2, 0.6, 1.0]), vals)
        B = rand_mat(rng, typ, *((n, k) if tb else (k, n)), rng.choice([0.2, 0.6, 1.0]), vals)
        Cm = rand_mat(rng, typ, m, n, 0.3, vals, empty_rows=False)
        mtyp = MASK_TYPES[case % len(MASK_TYPES)]
        mkind = str(rng.choice(["valued", "valued", "structural", "complemented", "structural complemented"]))
        M = rand_mat(rng, mtyp, m, n, rng.choice([0.3, 0.8]), np.array(MXM_MASK_VALUES[mtyp], MM.NP[mtyp]))
        struct, comp = "structural" in mkind, "complemented" in mkind
        replace = rng.random() < 0.4
        accum = None if rng.random() < 0.5 else ("LOR" if typ == "BOOL" else str(rng.choice(["PLUS", "MIN"])))
        seen |= {sr, mkind, mtyp, "ta" if ta else "a", "tb" if tb else "b", "accum" if accum else "no accum", "replace" if replace else "keep"}
        got = PM.mxm(Cm, A, B, add, mul, typ, mask=M, struct=struct, comp=comp, replace=replace, accum=(accum, typ) if accum else None, tran_a=ta, tran_b=tb)
        exp = O.mxm(tuples_of_mat(Cm), tuples_of_mat(A), tuples_of_mat(B), add, mul, typ, mask=tuples_of_mat(M), accum=accum, accum_type=typ, replace=replace, mask_comp=comp,
                    mask_struct=struct, tran_a=ta, tran_b=tb).sorted()
        what = (typ, case, sr, mkind, mtyp, ta, tb, replace, accum)
        assert np.array_equal(got.rows, exp.I.astype(np.int64)) and np.array_equal(got.cols, exp.J.astype(np.int64)), (what, got.keys, exp.I, exp.J)
        assert got.typ == typ and np.array_equal(got.vals, exp.X, equal_nan=typ.startswith("FP")), (what, got.vals, exp.X)
    assert seen >= set(srs) | set(MASK_TYPES) | {"valued", "structural", "complemented", "structural complemented", "ta", "a", "tb", "b", "accum", "no accum", "replace", "keep"}


def test_masked_mxm_by_hand():
    """A false or absent mask entry prunes its products; an allowed entry without a product is absent; the fold runs in ascending k (ANY keeps the largest)."""
    A = MM.from_coo(2, 3, [0, 0, 0, 1], [0, 1, 2, 1], [1, 2, 3, 4], "INT32")
    B = MM.from_coo(3, 3, [0, 0, 1, 1, 2], [0, 1, 0, 2, 0], [10, 20, 30, 40, 50], "INT32")
    M = MM.from_coo(2, 3, [0, 0, 0, 1, 1], [0, 1, 2, 0, 1], [-0.0, 1.0, np.nan, 2.0, 1.0], "FP64")
    t = PM.masked_mxm("PLUS", "TIMES", "INT32", A, B, M)
    assert t.keys.tolist() == [1, 2, 3] and t.vals.tolist() == [20, 80, 120]        # (0, 0) is false; (1, 1) receives nothing
    t = PM.masked_mxm("PLUS", "TIMES", "INT32", A, B, M, struct=True)
    assert t.keys.tolist() == [0, 1, 2, 3] and t.vals.tolist() == [10 + 60 + 150, 20, 80, 120]
    t = PM.masked_mxm("ANY", "SECOND", "INT32", A, B, None)
    assert t.keys.tolist() == [0, 1, 2, 3, 5] and t.vals.tolist() == [50, 20, 40, 30, 40]
