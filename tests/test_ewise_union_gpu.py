"""GxB_Matrix_eWiseUnion / GxB_Vector_eWiseUnion on the device against the numpy model of tests/union_model.py, on every route eWiseAdd takes: the CSR merge
(k_merge_fill), the bitmap vector kernels (k_vec_ewise, the one-pass k_vec_ewise_fused), the two batch routes, the compiled kernel of a user-defined operator and
the hypersparse relabelling.  The route is asserted from GrBX_last_kernel_plan, where a union names itself.

Comparisons are bit-exact on `to_csr()` / the bitmap (one exception: FP64 POW, with the math-library bound of test_math_library_operators).  Shapes, patterns and
values are those of test_matrix_kernels_at_size_gpu.py and test_vector_kernels_at_size_gpu.py.  alpha != beta throughout, so that an operator called with the
wrong scalar, on the wrong side or in the wrong order shows: integer types alpha = 7, beta = 3; floating point alpha = 0.5, beta = -2.0; BOOL true / false."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import matrix_model as MM
import vector_model as VM
import union_model as UM
import pygraphblas_amd as gb
from pygraphblas_amd import descriptor as D
from helpers import TYPE
from test_matrix_kernels_at_size_gpu import pattern, mat, values, same_bits, desc_of, dev, check, new, sub, operand_pairs, mask_over
from test_vector_kernels_at_size_gpu import N_MID, N_BIG, presence, operand, dev as vdev, check as vcheck, mask_values

pytestmark = pytest.mark.gpu

NP = MM.NP
MAT_TYPES = ["BOOL", "INT8", "UINT16", "FP32", "INT64", "FP64"]
WIDTHS = ["INT8", "UINT16", "FP32", "INT64"]


def fills(typ):
    return (True, False) if typ == "BOOL" else (7, 3) if "INT" in typ else (0.5, -2.0)


def plan():
    return gb.last_kernel_plan()


def assert_union_plan(on, kernel, opname=None):
    """"ewise_union<on=matrix|vector,op=NAME> KERNEL<union>": what the CSR merge and the vector kernels leave for a union."""
    p = plan()
    assert p.startswith(f"ewise_union<on={on},op=") and p.endswith(f"> {kernel}<union>") and (opname is None or f"_{opname}_" in p or p.count(opname)), p


def div_safe(A, B, typ):
    """Integer DIV: no zero divisor (beta is 3) and no most-negative numerator (alpha is 7)."""
    if "INT" not in typ: return A, B
    lo = np.iinfo(NP[typ]).min
    fix = lambda m, bad, good: MM.Mat(m.nrows, m.ncols, m.keys, np.where(m.vals == bad, NP[typ](good), m.vals))
    return fix(A, lo, 7), fix(fix(B, 0, 3), lo, 7)


# ---- matrices: the CSR merge ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", MAT_TYPES)
def test_matrix_union_through_the_csr_merge(gpu, typ):
    """Every operand pairing on `uniform` (60 000 entries, no multiple of 256), two independent patterns on `ragged`, `mult256`, `mult256p1` and `single`.  MINUS
    and DIV tell order and side apart, FIRST must give alpha at B-only entries and SECOND beta at A-only ones, ISGT compares with the fill value; the values hold
    the types' extremes, so MINUS wraps."""
    T = TYPE[typ]; alpha, beta = fills(typ)
    ops = ["LXOR", "LAND", "FIRST", "SECOND"] if typ == "BOOL" else ["MINUS", "DIV", "FIRST", "SECOND", "ISGT"]
    for name in ("uniform", "ragged", "mult256", "mult256p1", "single"):
        for label, A, B in operand_pairs(name, typ):
            if name != "uniform" and label != "independent": continue
            a, b = dev(A), dev(B)
            for op in ops:
                A1, B1 = div_safe(A, B, typ) if op == "DIV" else (A, B)
                got = (dev(A1).eunion(dev(B1), T.DIV, alpha, beta) if op == "DIV" else a.eunion(b, getattr(T, op), alpha, beta))
                assert_union_plan("matrix", "k_merge_fill", op)
                check(got, UM.union(op, typ, A1, alpha, B1, beta), f"eunion {op} {typ} {name}: {label}")


def test_first_gives_alpha_where_only_b_has_an_entry(gpu):
    """Written out, not through the model: disjoint patterns, FIRST and SECOND."""
    A = mat("uniform", "INT64", seed=2); B0 = mat("uniform", "INT64", seed=3, variant=1); B = sub(B0, ~np.isin(B0.keys, A.keys))
    first = dev(A).eunion(dev(B), gb.INT64.FIRST, 7, 3); second = dev(A).eunion(dev(B), gb.INT64.SECOND, 7, 3)
    keys = np.union1d(A.keys, B.keys); from_b = np.isin(keys, B.keys)
    va = np.zeros(len(keys), np.int64); va[~from_b] = A.vals; vb = np.zeros(len(keys), np.int64); vb[from_b] = B.vals
    check(first, MM.Mat(A.nrows, A.ncols, keys, np.where(from_b, np.int64(7), va)), "FIRST: a at A's entries, alpha at B's")
    check(second, MM.Mat(A.nrows, A.ncols, keys, np.where(from_b, vb, np.int64(3))), "SECOND: beta at A's entries, b at B's")


def test_matrix_union_pow_within_the_math_library_bound(gpu):
    """FP64 POW on `uniform` (the MATH = true instantiation of the fill kernel): bases in [0.5, 2.5], exponents in [0, 0.5], alpha = 1.5 a base and beta = 0.25 an
    exponent, rtol = 1e-12 against np.power as in test_math_library_operators — every entry goes through the operator; the pattern is exact."""
    rng = np.random.default_rng(9)
    nr, nc, ka = pattern("uniform"); _, _, kb0 = pattern("uniform", 1)
    kb = np.union1d(kb0[::2], ka[::3])
    A = MM.Mat(nr, nc, ka, 0.5 + 2.0 * rng.random(len(ka))); B = MM.Mat(nr, nc, kb, 0.5 * rng.random(len(kb)))
    got = dev(A).eunion(dev(B), gb.FP64.POW, 1.5, 0.25); exp = UM.union("POW", "FP64", A, 1.5, B, 0.25)
    rp, ci, x = got.to_csr(); erp, eci, ex = MM.to_csr(exp)
    assert np.array_equal(rp, erp) and np.array_equal(ci, eci)
    assert np.allclose(x, ex, rtol=1e-12, atol=0.0)
    only_a = ~np.isin(exp.keys, kb)
    assert only_a.sum() > 1000 and not np.allclose(x[only_a], A.vals[~np.isin(ka, kb)], rtol=1e-3), "a ** beta, not a, where only A has an entry"


def test_scalars_of_another_type_are_cast_into_the_operators(gpu):
    """FP64 operands and FP64 scalars under INT32.MINUS: 2.75 acts as 2 and -1.5 as -1, the operands are truncated the same way."""
    A = mat("uniform", "FP64", seed=2); B = mat("uniform", "FP64", seed=3, variant=1)
    got = dev(A).eunion(dev(B), gb.INT32.MINUS, 2.75, -1.5, cast=gb.INT32)
    exp = UM.union("MINUS", "INT32", A, 2.75, B, -1.5)
    check(got, exp, "FP64 scalars into INT32.MINUS")
    check(got, UM.union("MINUS", "INT32", A, 2, B, -1), "... which is alpha = 2, beta = -1")


@pytest.mark.parametrize("typ", ["INT8", "FP32"])
def test_matrix_union_transposed_and_aliased(gpu, typ):
    """GrB_INP0, GrB_INP1 (the cached transpose is the operand) and C aliased to A, then to B."""
    T = TYPE[typ]; alpha, beta = fills(typ)
    P = mat("uniform", typ, seed=4, extreme=True); Q = mat("uniform", typ, seed=5, variant=1, extreme=True)
    exp = UM.union("MINUS", typ, P, alpha, Q, beta)
    p, q, pt, qt = dev(P), dev(Q), dev(MM.transpose(P)), dev(MM.transpose(Q))
    check(pt.eunion(q, T.MINUS, alpha, beta, out=new(typ, P.nrows, P.ncols), desc=D.T0), exp, f"INP0 {typ}")
    check(p.eunion(qt, T.MINUS, alpha, beta, out=new(typ, P.nrows, P.ncols), desc=D.T1), exp, f"INP1 {typ}")
    assert_union_plan("matrix", "k_merge_fill", "MINUS")
    a = dev(P); a.eunion(q, T.MINUS, alpha, beta, out=a); check(a, exp, f"C is A {typ}")
    b = dev(Q); p.eunion(b, T.MINUS, alpha, beta, out=b); check(b, exp, f"C is B {typ}"); check(p, P, "A is unchanged")


@pytest.mark.parametrize("typ", ["INT32", "FP32"])
def test_matrix_union_write_back(gpu, typ):
    """C<M, replace> = accum(C, T) is the existing write-back: a valued, a structural and a complemented mask with and without replace, an accumulator, a mask
    of another type — all against matrix_model.write_back of the model's T."""
    T = TYPE[typ]; alpha, beta = fills(typ); rng = np.random.default_rng(21)
    A = mat("uniform", typ, seed=2, extreme=True); B = mat("uniform", typ, seed=3, variant=1, extreme=True); C0 = mat("uniform", typ, seed=6, variant=2)
    Tm = UM.union("MINUS", typ, A, alpha, B, beta); a, b = dev(A), dev(B)
    M = mask_over(rng, typ, A, B, C0); Mo = mask_over(rng, "INT8" if typ == "FP32" else "FP64", A, B, C0)
    cases = [(M, s, c, r, None) for s, c in ((False, False), (True, False), (False, True)) for r in (False, True)]
    cases += [(None, False, False, False, "PLUS"), (M, False, False, False, "PLUS"), (Mo, False, False, True, None), (Mo, False, True, False, "PLUS")]
    for mask, struct, comp, replace, accum in cases:
        c = dev(C0)
        a.eunion(b, T.MINUS, alpha, beta, out=c, mask=None if mask is None else dev(mask), accum=getattr(T, accum) if accum else None, desc=desc_of(replace, struct, comp))
        exp = MM.write_back(C0, Tm, mask, struct, comp, replace, (accum, typ) if accum else None)
        check(c, exp, f"write-back {typ}: mask={None if mask is None else mask.typ} struct={struct} comp={comp} replace={replace} accum={accum}")
        assert_union_plan("matrix", "k_merge_fill", "MINUS")


# ---- vectors -------------------------------------------------------------------------------------------------------------------------------------------------
PAIRS = [("half", "blocks"), ("full", "half"), ("half", "full"), ("empty", "half"), ("half", "empty"), ("full", "full"), ("empty", "empty")]


def vec_pair(typ, n, pu, pv):
    U = operand(typ, n, pu, seed=7, extreme=True); V = operand(typ, n, pv, seed=8, extreme=True)
    return U, V, vdev(U, full=pu == "full"), vdev(V, full=pv == "full")


@pytest.mark.parametrize("typ", WIDTHS)
@pytest.mark.parametrize("n", [15, 16, 17, N_MID])
def test_vector_union_on_the_three_kernel_and_the_one_pass_route(gpu, monkeypatch, typ, n):
    """No mask and no accumulator: k_vec_ewise, T adopted.  With an accumulator or a mask, every type w's own: k_vec_ewise_fused.  Every value width, the sizes
    around one 16-byte group and N_MID (past one round of the grid); presence half / blocks / full / empty on either side."""
    monkeypatch.delenv("GRB_MI355X_EWISE_FUSED", raising=False)
    T = TYPE[typ]; alpha, beta = fills(typ)
    for pu, pv in (PAIRS if n != N_MID else PAIRS[:4]):
        U, V, u, v = vec_pair(typ, n, pu, pv)
        exp = UM.union("MINUS", typ, U, alpha, V, beta)
        vcheck(u.eunion(v, T.MINUS, alpha, beta), exp, f"eunion MINUS {typ} n={n} {pu}/{pv}")
        assert_union_plan("vector", "k_vec_ewise", "MINUS")
        W = operand(typ, n, "half", seed=9); w = vdev(W)
        u.eunion(v, T.MINUS, alpha, beta, out=w, accum=T.PLUS)
        assert_union_plan("vector", "k_vec_ewise_fused", "MINUS")
        vcheck(w, VM.write_back(W, exp, accum=("PLUS", typ)), f"eunion MINUS accum=PLUS {typ} n={n} {pu}/{pv}")
        vcheck(u, U, "the first operand is unchanged")
    # ISGT and DIV with a mask of another type, replace: the one-pass kernel reads the mask in place
    U, V, u, v = vec_pair(typ, n, "half", "blocks")
    V = VM.Vec(np.where(V.val == 0, NP[typ](3), V.val), V.pres); U = VM.Vec(np.where(U.val == np.iinfo(NP[typ]).min, NP[typ](7), U.val) if "INT" in typ else U.val, U.pres)
    u, v = vdev(U), vdev(V)
    M = VM.Vec(mask_values(np.random.default_rng(10), "INT8" if typ != "INT8" else "FP32", n), presence("half", n, 11))
    for op, struct, comp in (("DIV", False, False), ("ISGT", True, False), ("DIV", False, True)):
        W = operand(typ, n, "half", seed=9); w = vdev(W)
        u.eunion(v, getattr(T, op), alpha, beta, out=w, mask=vdev(M), desc=desc_of(True, struct, comp))
        assert_union_plan("vector", "k_vec_ewise_fused", op)
        vcheck(w, VM.write_back(W, UM.union(op, typ, U, alpha, V, beta), M, struct, comp, True), f"eunion {op} {typ} n={n} masked, replace")


def test_vector_union_at_n_big(gpu):
    """INT32 at N_BIG: the grid-stride loops of k_vec_ewise and k_vec_ewise_fused run more than one round (grid_for caps at 2048 workgroups of 256)."""
    assert N_BIG > 2 * 2048 * 256
    U, V, u, v = vec_pair("INT32", N_BIG, "half", "blocks")
    exp = UM.union("MINUS", "INT32", U, 7, V, 3)
    vcheck(u.eunion(v, gb.INT32.MINUS, 7, 3), exp, "N_BIG, k_vec_ewise")
    assert_union_plan("vector", "k_vec_ewise")
    W = operand("INT32", N_BIG, "half", seed=9); w = vdev(W)
    u.eunion(v, gb.INT32.MINUS, 7, 3, out=w, accum=gb.INT32.PLUS)
    assert_union_plan("vector", "k_vec_ewise_fused")
    vcheck(w, VM.write_back(W, exp, accum=("PLUS", "INT32")), "N_BIG, k_vec_ewise_fused")


def test_vector_union_with_the_one_pass_kernel_switched_off_and_with_mixed_types(gpu, monkeypatch):
    """GRB_MI355X_EWISE_FUSED=0: k_allow, k_vec_ewise, k_vec_epilogue under a mask and an accumulator.  INT8 operands under an FP64 operator take that route by
    themselves (k_cast on the way in and out)."""
    n = N_MID; typ = "INT64"; T = TYPE[typ]
    U, V, u, v = vec_pair(typ, n, "half", "blocks"); exp = UM.union("MINUS", typ, U, 7, V, 3)
    M = VM.Vec(mask_values(np.random.default_rng(10), "FP32", n), presence("half", n, 11))
    monkeypatch.setenv("GRB_MI355X_EWISE_FUSED", "0")
    for comp, replace, accum in ((False, False, "PLUS"), (True, True, None), (False, True, "SECOND")):
        W = operand(typ, n, "half", seed=9); w = vdev(W)
        u.eunion(v, T.MINUS, 7, 3, out=w, mask=vdev(M), accum=getattr(T, accum) if accum else None, desc=desc_of(replace, False, comp))
        assert_union_plan("vector", "k_vec_ewise", "MINUS")
        vcheck(w, VM.write_back(W, exp, M, False, comp, replace, (accum, typ) if accum else None), f"EWISE_FUSED=0 comp={comp} replace={replace} accum={accum}")
    monkeypatch.delenv("GRB_MI355X_EWISE_FUSED", raising=False)
    U8, V8, u8, v8 = vec_pair("INT8", n, "half", "blocks"); W = operand("FP64", n, "half", seed=9); w = vdev(W)
    u8.eunion(v8, gb.FP64.MINUS, 7, 3, out=w, accum=gb.FP64.PLUS)                  # (the scalars are made in the operands' promoted type, INT8)
    assert_union_plan("vector", "k_vec_ewise", "MINUS")
    vcheck(w, VM.write_back(W, UM.union("MINUS", "FP64", U8, 7, V8, 3), accum=("PLUS", "FP64")), "INT8 operands under FP64.MINUS")


def test_vector_union_into_its_own_operand(gpu):
    """w aliased to u, on both kernels: everything of position i is read before anything of position i is written."""
    for typ in ("FP32", "INT64"):
        T = TYPE[typ]; alpha, beta = fills(typ)
        U, V, u, v = vec_pair(typ, N_MID, "half", "blocks"); exp = UM.union("MINUS", typ, U, alpha, V, beta)
        u.eunion(v, T.MINUS, alpha, beta, out=u); vcheck(u, exp, f"w is u {typ}"); assert_union_plan("vector", "k_vec_ewise")
        u2 = vdev(U); u2.eunion(v, T.MINUS, alpha, beta, out=u2, accum=T.PLUS)
        assert_union_plan("vector", "k_vec_ewise_fused")
        vcheck(u2, VM.write_back(U, exp, accum=("PLUS", typ)), f"w is u, accum {typ}")
        v2 = vdev(V); u2 = vdev(U); u2.eunion(v2, T.MINUS, alpha, beta, out=v2, accum=T.SECOND); vcheck(v2, VM.write_back(V, exp, accum=("SECOND", typ)), f"w is v {typ}")


def abs_then_union():
    """`t = abs(t)` immediately before `t.eunion(r, MINUS, 0, 0)`: in non-blocking mode the apply is queued, and the union — never queued itself — has to run after
    it.  Returns the mode the library ran in as the number of chains it had run before and after."""
    from test_vector_kernels_at_size_gpu import lazy_stats
    Tm = operand("FP64", N_MID, "half", seed=7); R = operand("FP64", N_MID, "blocks", seed=8)
    t, r = vdev(Tm), vdev(R)
    before = lazy_stats()["chains"]
    t = t.apply(gb.FP64.ABS)
    got = t.eunion(r, gb.FP64.MINUS, 0, 0)
    assert_union_plan("vector", "k_vec_ewise", "MINUS")
    vcheck(got, UM.union("MINUS", "FP64", VM.apply("ABS", "FP64", Tm), 0, R, 0), "abs(t) - r over the union")
    vcheck(t, VM.apply("ABS", "FP64", Tm), "t = abs(t)")
    return lazy_stats()["chains"] - before


def test_vector_union_after_queued_work(gpu):
    """The residual `|t| - r` of an iteration, in this (non-blocking) process — where the apply must have gone through the queue — and in a GRB_MI355X_BLOCKING=1
    child, where nothing is queued."""
    assert abs_then_union() >= 1, "the apply in front of the union was not queued: this process does not run non-blocking"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r}); import test_ewise_union_gpu as t; print('chains', t.abs_then_union())"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GRB_MI355X_BLOCKING="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "chains 0", (r.stdout, r.stderr)


# ---- the batch routes ----------------------------------------------------------------------------------------------------------------------------------------
def batch_pair(ncols, seed=0):
    rng = np.random.default_rng([ncols, seed])
    mk = lambda: MM.Mat(4, ncols, np.sort(rng.choice(4 * ncols, size=30001, replace=False)).astype(np.int64), values(rng, "FP32", 30001, True))
    return mk(), mk()


def csr_route_result(A, B):
    got = dev(A).eunion(dev(B), gb.FP32.MINUS, 0.5, -2.0)
    assert_union_plan("matrix", "k_merge_fill", "MINUS")
    return got


def test_batch_matrix_union_as_one_vector(gpu, monkeypatch):
    """GRB_MI355X_BATCH=1.  The bitmap route takes matrices of at most 64 rows whose column count is a multiple of 64 (mat_batch_shape): a 4 x 70 000 pair stays on
    the CSR merge whatever the variable says, a 4 x 70 016 pair goes through the vector kernel as one vector of 280 064 positions."""
    monkeypatch.delenv("GRB_MI355X_EWISE_ROWS", raising=False)
    for ncols, batch in ((70000, False), (70016, True)):
        A, B = batch_pair(ncols); exp = UM.union("MINUS", "FP32", A, 0.5, B, -2.0)
        monkeypatch.delenv("GRB_MI355X_BATCH", raising=False)
        ref = csr_route_result(A, B); check(ref, exp, f"4 x {ncols}, CSR merge")
        monkeypatch.setenv("GRB_MI355X_BATCH", "1")
        got = dev(A).eunion(dev(B), gb.FP32.MINUS, 0.5, -2.0)
        if batch: assert plan() == f"ewise_batch<4 x {ncols} as one vector, union>", plan()
        else: assert_union_plan("matrix", "k_merge_fill", "MINUS")
        check(got, exp, f"4 x {ncols}, GRB_MI355X_BATCH=1")
        g, r = got.to_csr(), ref.to_csr()
        assert all(np.array_equal(x, y) for x, y in zip(g[:2], r[:2])) and same_bits(g[2], r[2]).all(), "the batch route and the CSR merge agree"
        if batch:                                                                   # ... with an accumulator: the one-pass kernel over the flattened bitmap
            C0 = batch_pair(ncols, 1)[0]; c = dev(C0)
            dev(A).eunion(dev(B), gb.FP32.MINUS, 0.5, -2.0, out=c, accum=gb.FP32.PLUS)
            assert plan() == f"ewise_batch<4 x {ncols} as one vector, union>", plan()
            check(c, MM.write_back(C0, exp, accum=("PLUS", "FP32")), "batch, accum=PLUS")


def test_batch_matrix_union_row_by_row(gpu, monkeypatch):
    """GRB_MI355X_EWISE_ROWS=1: the 4 x 70 000 pair row by row through the vector entry point."""
    monkeypatch.delenv("GRB_MI355X_BATCH", raising=False); monkeypatch.delenv("GRB_MI355X_EWISE_ROWS", raising=False)
    A, B = batch_pair(70000); exp = UM.union("MINUS", "FP32", A, 0.5, B, -2.0)
    ref = csr_route_result(A, B)
    monkeypatch.setenv("GRB_MI355X_EWISE_ROWS", "1")
    got = dev(A).eunion(dev(B), gb.FP32.MINUS, 0.5, -2.0)
    assert plan() == "ewise_rows<4 x vector eWise union>", plan()
    check(got, exp, "4 x 70 000, GRB_MI355X_EWISE_ROWS=1")
    g, r = got.to_csr(), ref.to_csr()
    assert all(np.array_equal(x, y) for x, y in zip(g[:2], r[:2])) and same_bits(g[2], r[2]).all(), "the row-wise route and the CSR merge agree"


# ---- a user-defined operator -----------------------------------------------------------------------------------------------------------------------------------
def f(x, y):
    return x - 2 * y


def test_user_defined_operator_is_called_on_every_entry(gpu):
    """`f(x, y) = x - 2 y` through Matrix.eunion on `uniform` and Vector.eunion at N_MID: the compiled kernel (kind eunion) calls f where one operand alone has the
    entry too — a - 2 beta there, not a."""
    op = gb.binary_op(gb.FP64)(f); alpha, beta = 0.5, -2.0
    A = mat("uniform", "FP64", seed=2); B = mat("uniform", "FP64", seed=3, variant=1)
    got = dev(A).eunion(dev(B), op, alpha, beta)
    assert plan().startswith("userop<name=f,kind=eunion,type=GrB_FP64>"), plan()
    exp = UM.union(f, "FP64", A, alpha, B, beta)
    check(got, exp, "user-defined f on uniform")
    only_a = ~np.isin(A.keys, B.keys); x = got.to_csr()[2][np.isin(exp.keys, A.keys[only_a])]
    assert only_a.sum() > 50000 and np.array_equal(x, A.vals[only_a] + 4.0) and not np.array_equal(x, A.vals[only_a]), "a - 2 beta where only A has an entry"
    c = dev(mat("uniform", "FP64", seed=6, variant=2)); C0 = mat("uniform", "FP64", seed=6, variant=2)
    dev(A).eunion(dev(B), op, alpha, beta, out=c, accum=gb.FP64.PLUS); check(c, MM.write_back(C0, exp, accum=("PLUS", "FP64")), "user-defined f, accum")
    for n in (17, N_MID):
        U, V, u, v = vec_pair("FP64", n, "half", "blocks")
        w = u.eunion(v, op, alpha, beta)
        assert plan().startswith("userop<name=f,kind=eunion,type=GrB_FP64>"), plan()
        ve = UM.union(f, "FP64", U, alpha, V, beta); vcheck(w, ve, f"user-defined f on a vector, n = {n}")
        lone = U.pres & ~V.pres; assert np.array_equal(w.to_dense_arrays()[0][lone], U.val[lone] + 4.0)


# ---- hypersparse containers ------------------------------------------------------------------------------------------------------------------------------------
def test_hypersparse_union(gpu):
    """2^60-sized operands with a dozen entries each, partly overlapping: the relabelling is that of a union, the scalars pass through."""
    IMAX = 1 << 60; rng = np.random.default_rng(5)
    pool = np.unique(np.concatenate([rng.integers(0, IMAX, 24, dtype=np.uint64), np.array([0, 1, IMAX - 1, (1 << 32) - 1, 1 << 32], np.uint64)]))
    ia, ib = pool[::2][:12], pool[::3][:12]
    assert len(np.intersect1d(ia, ib)) >= 2 and len(np.setdiff1d(ia, ib)) >= 2 and len(np.setdiff1d(ib, ia)) >= 2
    xa = rng.integers(-16, 17, len(ia)) / 8.0; xb = rng.integers(-16, 17, len(ib)) / 8.0
    model = lambda ka, kb: {k: (xa[list(ka).index(k)] if k in ka else 0.5) - (xb[list(kb).index(k)] if k in kb else -2.0) for k in sorted(set(ka) | set(kb))}
    u = gb.Vector.from_arrays(ia, xa, IMAX, gb.FP64); v = gb.Vector.from_arrays(ib, xb, IMAX, gb.FP64)
    w = u.eunion(v, gb.FP64.MINUS, 0.5, -2.0)
    I, X = w.to_arrays(); exp = model([int(k) for k in ia], [int(k) for k in ib])
    assert w.size == IMAX and dict(zip([int(i) for i in I], X.tolist())) == exp
    ja, jb = pool[::-1][::2][:12], pool[::-1][::3][:12]                          # columns: another pairing of the same pool
    A = gb.Matrix.from_arrays(ia, ja, xa, IMAX, IMAX, gb.FP64); B = gb.Matrix.from_arrays(ib, jb, xb, IMAX, IMAX, gb.FP64)
    Cm = A.eunion(B, gb.FP64.MINUS, 0.5, -2.0)
    I, J, X = Cm.to_arrays()
    ka = [(int(i), int(j)) for i, j in zip(ia, ja)]; kb = [(int(i), int(j)) for i, j in zip(ib, jb)]
    assert Cm.shape == (IMAX, IMAX) and dict(zip([(int(i), int(j)) for i, j in zip(I, J)], X.tolist())) == model(ka, kb)
    assert len(set(ka) & set(kb)) >= 1 and len(set(ka) - set(kb)) >= 2 and len(set(kb) - set(ka)) >= 2


# ---- errors on the device: the output is untouched -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(gpu):
    A = mat("single", "FP64", seed=2); C0 = mat("single", "FP64", seed=6); c = dev(C0)
    wrong = gb.Matrix.sparse(gb.FP64, 300, 301)
    with pytest.raises(gb.base.DimensionMismatch):
        dev(A).eunion(wrong, gb.FP64.MINUS, 0.5, -2.0, out=c)
    check(c, C0, "after a dimension mismatch")
    U = operand("FP64", 17, "half", seed=7); w = vdev(U)
    with pytest.raises(gb.base.DimensionMismatch):
        vdev(U).eunion(gb.Vector.sparse(gb.FP64, 18), gb.FP64.MINUS, 0.5, -2.0, out=w)
    vcheck(w, U, "after a size mismatch")
    # a complex operand (the package has no Python class for the complex types: through the C ABI), refused before the dimensions are looked at
    Z = C.c_void_p(); fc64 = C.c_void_p(gb._capi.handle("GxB_FC64"))
    assert gb.lib.GrB_Matrix_new(C.byref(Z), fc64, C.c_uint64(300), C.c_uint64(301)) == 0
    s = C.c_void_p(); assert gb.lib.GxB_Scalar_new(C.byref(s), C.c_void_p(gb.FP64._h)) == 0 and gb.lib.GxB_Scalar_setElement_FP64(s, C.c_double(1.0)) == 0
    a = dev(A); op = C.c_void_p(gb.FP64.MINUS.get_op())
    assert gb.lib.GxB_Matrix_eWiseUnion(c._h, None, None, op, a._h, s, Z, s, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    assert gb.lib.GxB_Matrix_eWiseUnion(c._h, None, None, op, Z, s, a._h, s, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    check(c, C0, "after a complex operand")
    gb.lib.GxB_Scalar_free(C.byref(s)); gb.lib.GrB_Matrix_free(C.byref(Z))


# ---- eWiseAdd and eWiseMult are what they were -------------------------------------------------------------------------------------------------------------------
# GrBX_last_kernel_plan after eadd / emult, recorded on the commit before GxB_eWiseUnion existed.  The CSR merge leaves the string alone (here: what the upload of
# the operands behind a 2 x 2 product left), the batch routes write their own.
UNCHANGED = [("uniform", "INT32", "PLUS", None, "build<type=INT32,dup=none,key=u32,sorted=1,fold=none,rows=heads> k_build_keys k_build_unpack",
              "build<type=INT32,dup=none,key=u32,sorted=1,fold=none,rows=heads> k_build_keys k_build_unpack"),
             ("4 x 70016", "FP32", "MINUS", "GRB_MI355X_BATCH", "ewise_batch<4 x 70016 as one vector>", "ewise_batch<4 x 70016 as one vector>"),
             ("4 x 70000", "FP32", "MINUS", "GRB_MI355X_EWISE_ROWS", "ewise_rows<4 x vector eWise>", "ewise_rows<4 x vector eWise>")]


def plans_of_eadd_and_emult(shape, typ, op, env):
    """(plan after eadd, plan after emult, the two results) with `env` set to 1 for the calls, each behind a fresh 2 x 2 product."""
    if shape == "uniform": A = mat("uniform", typ, seed=2, extreme=True); B = mat("uniform", typ, seed=3, variant=1, extreme=True)
    else: A, B = batch_pair(int(shape.split()[-1]))
    out = []
    for union in (True, False):
        e = gb.Matrix.from_lists([0], [0], [1], 2, 2, gb.INT64); e.mxm(e, semiring=gb.INT64.PLUS_TIMES)
        a, b = dev(A), dev(B)
        if env: os.environ[env] = "1"
        try: got = (a.eadd if union else a.emult)(b, getattr(TYPE[typ], op))
        finally:
            if env: del os.environ[env]
        out.append((plan(), got, MM.ewise(op, typ, A, B, union)))
    return out


@pytest.mark.parametrize("shape,typ,op,env,plan_add,plan_mult", UNCHANGED)
def test_eadd_and_emult_are_unchanged(gpu, monkeypatch, shape, typ, op, env, plan_add, plan_mult):
    for v in ("GRB_MI355X_BATCH", "GRB_MI355X_EWISE_ROWS"): monkeypatch.delenv(v, raising=False)
    (pa, ga, ea), (pm, gm, em) = plans_of_eadd_and_emult(shape, typ, op, env)
    assert pa == plan_add and pm == plan_mult, (pa, pm)
    check(ga, ea, f"eadd {op} {typ} {shape}"); check(gm, em, f"emult {op} {typ} {shape}")
