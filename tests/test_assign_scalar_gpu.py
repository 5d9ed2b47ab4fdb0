"""Matrix scalar assign in HBM (grb_assign_scalar.hip behind GrB_Matrix_assign_<T>): C<M, replace>(I, J) = accum(C(I, J), s) with T built on the device — from
the mask's pattern when the mask is not complemented, as the closed-form block otherwise — and the Python surface over it (Matrix.assign_scalar, the scalar
branches of __setitem__, Matrix.sparse(fill=, mask=)).

References, none of them the code under test: the numpy model of tests/assign_scalar_model.py (the C API's rule; its mask-restricted formulation for regions
too large to form), and the host-built block every earlier version ran (GRB_MI355X_ASSIGN_SCALAR=0).  All values are small integers, so every result,
accumulated ones included, is exact in every type and compared bit for bit.  No list names an index twice except in the one test of that fallback.
"""
import contextlib
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import assign_scalar_model as model
import matrix_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 400                                                              # the C of the kernel-edge tests: 400 x 400, about 2 000 entries
WIDTHS = ["BOOL", "INT16", "FP32", "FP64"]                           # value widths 1, 2, 4, 8
KINDS = ["all", "range", "stride", "backwards", "sorted", "shuffled"]
BLOCKS = [(1, 1), (1, 3), (3, 1), (5, 7), (37, 29), (300, 301)]      # 37 x 29 = 1 073 entries: past one workgroup's 1 024; 300 x 301: many workgroups, odd ncs


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def random_mat(rng, nrows, ncols, typ, nnz, zeros=False):
    """nnz distinct positions; values 1 .. 3 (BOOL: true), with `zeros` a third of them explicit zeros."""
    keys = np.unique(rng.integers(0, nrows * ncols, nnz, dtype=np.int64))
    vals = np.ones(len(keys), np.int64) if typ == "BOOL" else rng.integers(1, 4, len(keys))
    if zeros:
        vals[rng.integers(0, 3, len(keys)) == 0] = 0
    return mm.Mat(nrows, ncols, keys, vals.astype(mm.NP[typ]))


def upload(gb, m):
    return gb.Matrix.from_arrays(m.rows.astype(np.uint64), m.cols.astype(np.uint64), m.vals, m.nrows, m.ncols, getattr(gb, m.typ))


def download(A, typ):
    I, J, X = A.to_arrays()
    return mm.Mat(A.nrows, A.ncols, I.astype(np.int64) * np.int64(A.ncols) + J.astype(np.int64), X.astype(mm.NP[typ], copy=False))


def same(got, exp, what):
    assert got.typ == exp.typ and np.array_equal(got.keys, exp.keys), f"{what}: pattern differs ({got.nvals} / {exp.nvals} entries)"
    assert got.vals.tobytes() == exp.vals.tobytes(), f"{what}: values differ"


def pick(kind, d, n, rng):
    """(argument for the Python surface, the positions it names): n indices of a dimension d >= n in one index kind (all: every index), without repeats."""
    if kind == "all":
        return None, list(range(d))
    if kind == "range":
        a = int(rng.integers(0, d - n + 1))
        return slice(a, a + n - 1), list(range(a, a + n))
    if kind in ("stride", "backwards"):
        s = 1 if n == 1 else int(rng.integers(1, (d - 1) // (n - 1) + 1)); s = min(s, 3)
        a = int(rng.integers(0, d - (n - 1) * s))
        if kind == "stride":
            return slice(a, a + (n - 1) * s, s), list(range(a, a + (n - 1) * s + 1, s))
        return slice(a + (n - 1) * s, a, -s), list(range(a + (n - 1) * s, a - 1, -s))
    lst = [int(x) for x in rng.permutation(d)[:n]]
    if kind == "sorted":
        lst = sorted(lst)
    return lst, lst


def descriptor(gb, struct=False, comp=False, replace=False):
    d = None
    for on, p in ((replace, gb.descriptor.R), (struct, gb.descriptor.S), (comp, gb.descriptor.C)):
        if on:
            d = p if d is None else (d & p)
    return d


def run(gb, Cm, s, rarg, carg, Mm=None, struct=False, comp=False, replace=False, accum=None, mask_is_c=False):
    """One call on fresh containers -> (C afterwards as a model matrix, the plan string); run.before: the plan string just before the call."""
    Cg = upload(gb, Cm)
    Mg = Cg if mask_is_c else (upload(gb, Mm) if Mm is not None else None)
    acc = getattr(getattr(gb, Cm.typ), accum) if accum else None
    run.before = gb.last_kernel_plan()
    Cg.assign_scalar(s, rarg, carg, mask=Mg, accum=acc, desc=descriptor(gb, struct, comp, replace))
    return download(Cg, Cm.typ), gb.last_kernel_plan()


def entries_of(plan):
    return int(re.search(r"entries=(\d+)", plan).group(1))


@pytest.fixture(scope="module")
def base(gb):
    rng = np.random.default_rng(4100)
    return {t: random_mat(rng, N, N, t, 2000) for t in WIDTHS}


# ---- 1. lane groups and workgroup edges of the block fill -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", WIDTHS)
@pytest.mark.parametrize("block", BLOCKS, ids=lambda b: f"{b[0]}x{b[1]}")
def test_block_fill_edges(gb, gpu, base, block, typ):
    rng = np.random.default_rng(4200 + block[0] * 7 + block[1] + WIDTHS.index(typ) * 1000)
    Cm = base[typ]
    ran = 0
    for rk in KINDS:
        for ck in KINDS:
            rarg, rows = pick(rk, N, block[0], rng)
            carg, cols = pick(ck, N, block[1], rng)
            for accum in (None, "PLUS"):
                if rk == "all" and ck == "all" and accum is None:
                    continue                                         # (the csr_dense_fill shortcut of M[:, :] = x: not this route)
                s = 1 if typ == "BOOL" else 2
                got, plan = run(gb, Cm, s, rarg, carg, accum=accum)
                name = {"all": "all", "sorted": "list", "shuffled": "list"}.get(rk, "range"), {"all": "all", "sorted": "list", "shuffled": "list"}.get(ck, "range")
                assert plan.startswith(f"assign_scalar<rows={name[0]},cols={name[1]},mask=none,accum=") and "k_assign_scalar_fill<block>" in plan, plan
                assert entries_of(plan) == len(rows) * len(cols), plan
                same(got, model.assign_scalar(Cm, s, rows, cols, accum=(accum, typ) if accum else None), f"{typ} {block} rows={rk} cols={ck} accum={accum}")
                ran += 1
    assert ran == 71


# ---- 2. the mask-driven route ---------------------------------------------------------------------------------------------------------------------------
def regions(rng):
    return [pick("range", N, 1, rng) + pick("all", N, N, rng), pick("range", N, 37, rng) + pick("stride", N, 29, rng), pick("shuffled", N, 300, rng) + pick("backwards", N, 130, rng),
            pick("sorted", N, 5, rng) + pick("shuffled", N, 7, rng), pick("all", N, N, rng) + pick("all", N, N, rng)]


@pytest.mark.parametrize("mtyp", ["UINT8", "FP64"])
@pytest.mark.parametrize("ctyp", WIDTHS)
def test_mask_driven_route(gb, gpu, base, ctyp, mtyp):
    rng = np.random.default_rng(4300 + WIDTHS.index(ctyp) + (50 if mtyp == "FP64" else 0))
    Cm = base[ctyp]
    Mm = random_mat(rng, N, N, mtyp, 3000, zeros=True)
    ran = 0
    for rarg, rows, carg, cols in regions(rng):
        for struct in (False, True):
            for replace in (False, True):
                for accum in (None, "PLUS"):
                    s = 1 if ctyp == "BOOL" else 3
                    got, plan = run(gb, Cm, s, rarg, carg, Mm, struct=struct, replace=replace, accum=accum)
                    assert plan.startswith("assign_scalar<") and "mask=pattern" in plan and "k_assign_scalar_flags" in plan, plan
                    exp_t = model.mask_block(Cm, s, rows, cols, Mm, struct)
                    assert entries_of(plan) == exp_t.nvals <= Mm.nvals, plan
                    same(got, model.assign_scalar(Cm, s, rows, cols, Mm, struct, False, replace, (accum, ctyp) if accum else None), f"{ctyp} mask {mtyp} struct={struct} replace={replace} accum={accum}")
                    ran += 1
    assert ran == 40


@pytest.mark.parametrize("ctyp", ["INT16", "FP64"])
def test_mask_driven_route_special_masks(gb, gpu, base, ctyp):
    """An empty M, M the same object as C (`A.assign_scalar(0, mask=A)`), and an M none of whose entries lies in the region."""
    rng = np.random.default_rng(4400)
    Cm = base[ctyp]
    for replace in (False, True):
        for accum in (None, "PLUS"):
            acc = (accum, ctyp) if accum else None
            got, plan = run(gb, Cm, 2, None, None, mm.empty(N, N, "BOOL"), replace=replace, accum=accum)
            assert "mask=pattern" in plan and entries_of(plan) == 0, plan
            same(got, model.assign_scalar(Cm, 2, range(N), range(N), mm.empty(N, N, "BOOL"), False, False, replace, acc), "empty mask")
            for struct in (False, True):
                got, plan = run(gb, Cm, 0, None, slice(10, 300), struct=struct, replace=replace, accum=accum, mask_is_c=True)
                assert "mask=pattern" in plan and entries_of(plan) <= Cm.nvals, plan
                same(got, model.assign_scalar(Cm, 0, range(N), range(10, 301), Cm, struct, False, replace, acc), "mask is C")
            Mm = random_mat(rng, N, N, "UINT8", 500)
            Mm = mm.Mat(N, N, Mm.keys[Mm.rows >= 200], Mm.vals[Mm.rows >= 200])
            got, plan = run(gb, Cm, 2, slice(0, 199), [5, 3, 399], Mm, replace=replace, accum=accum)
            assert "mask=pattern" in plan and entries_of(plan) == 0, plan
            same(got, model.assign_scalar(Cm, 2, range(200), [5, 3, 399], Mm, False, False, replace, acc), "mask outside the region")


# ---- 3. a complemented mask: the block route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctyp", WIDTHS)
@pytest.mark.parametrize("block", [(37, 29), (300, 301)], ids=lambda b: f"{b[0]}x{b[1]}")
def test_complemented_mask(gb, gpu, base, block, ctyp):
    rng = np.random.default_rng(4500 + block[0] + WIDTHS.index(ctyp))
    Cm = base[ctyp]
    Mm = random_mat(rng, N, N, "UINT8", 3000, zeros=True)
    ran = 0
    for rk, ck in (("range", "shuffled"), ("shuffled", "backwards"), ("stride", "sorted")):
        rarg, rows = pick(rk, N, block[0], rng)
        carg, cols = pick(ck, N, block[1], rng)
        for struct in (False, True):
            for replace in (False, True):
                for accum in (None, "PLUS"):
                    s = 1 if ctyp == "BOOL" else 3
                    got, plan = run(gb, Cm, s, rarg, carg, Mm, struct=struct, comp=True, replace=replace, accum=accum)
                    assert plan.startswith("assign_scalar<") and "mask=comp" in plan and "k_assign_scalar_fill<block>" in plan and entries_of(plan) == block[0] * block[1], plan
                    same(got, model.assign_scalar(Cm, s, rows, cols, Mm, struct, True, replace, (accum, ctyp) if accum else None), f"{ctyp} {block} comp struct={struct} replace={replace} accum={accum}")
                    ran += 1
    assert ran == 24


# ---- 4. the capability: a masked assign over a region no block can hold ----------------------------------------------------------------------------------
BIG = 70000


@pytest.fixture(scope="module")
def big(gb):
    rng = np.random.default_rng(4600)
    return random_mat(rng, BIG, BIG, "FP64", 200000), random_mat(rng, BIG, BIG, "UINT8", 100000, zeros=True), rng


@pytest.mark.parametrize("variant", ["plain", "replace+accum"])
@pytest.mark.parametrize("region", ["all x all", "row range x all", "shuffled rows x column stride"])
def test_masked_assign_over_70000_squared(gb, gpu, big, region, variant):
    """C<M> = s over up to 4.9e9 positions costs what nnz(M) + nnz(C) cost; the host-built block refused it with GrB_OUT_OF_MEMORY ("assign: region too large")."""
    Cm, Mm, _ = big
    rng = np.random.default_rng(4700)
    if region == "all x all":
        rarg, rows, carg, cols = None, np.arange(BIG), None, np.arange(BIG)
    elif region == "row range x all":
        rarg, rows, carg, cols = slice(1000, 69000), np.arange(1000, 69001), None, np.arange(BIG)
    else:
        rows = rng.permutation(BIG)[:20000]; rarg = rows.astype(np.uint64)
        carg, cols = slice(3, 69999, 2), np.arange(3, 70000, 2)
    replace, accum = (True, "PLUS") if variant == "replace+accum" else (False, None)
    got, plan = run(gb, Cm, 5, rarg, carg, Mm, replace=replace, accum=accum)
    assert "mask=pattern" in plan and entries_of(plan) <= Mm.nvals, plan
    same(got, model.assign_scalar_restricted(Cm, 5, rows, cols, Mm, False, replace, (accum, "FP64") if accum else None), f"{region} {variant}")


def test_unmasked_70000_squared_is_still_refused(gb, gpu, big):
    Cg = upload(gb, big[0])
    for kw in ({}, {"accum": gb.FP64.PLUS}, {"mask": upload(gb, big[1]), "desc": gb.descriptor.C}):
        with pytest.raises(gb.base.OutOfMemory, match="assign: region too large"):
            Cg.assign_scalar(1.0, **kw)
    same(download(Cg, "FP64"), big[0], "C after the refused calls")


# ---- 5. the routes agree --------------------------------------------------------------------------------------------------------------------------------
def test_routes_agree(gb, gpu, base):
    """A sample of the cases above once more with GRB_MI355X_ASSIGN_SCALAR=0: the host-built block gives the same bits and leaves the plan string as it found it."""
    rng = np.random.default_rng(4800)
    Mm = random_mat(rng, N, N, "FP64", 3000, zeros=True)
    ran = 0
    for ctyp in WIDTHS:
        Cm = base[ctyp]
        for block, rk, ck in (((5, 7), "shuffled", "backwards"), ((37, 29), "stride", "shuffled"), ((300, 301), "range", "sorted"), ((1, 3), "all", "stride")):
            rarg, rows = pick(rk, N, block[0], rng)
            carg, cols = pick(ck, N, block[1], rng)
            for mask, comp, struct, replace, accum in ((None, False, False, False, None), (None, False, False, False, "PLUS"), (Mm, False, False, True, "PLUS"), (Mm, False, True, False, None),
                                                       (Mm, True, False, False, None), (Mm, True, True, True, "PLUS")):
                s = 1 if ctyp == "BOOL" else 2
                dev, plan = run(gb, Cm, s, rarg, carg, mask, struct=struct, comp=comp, replace=replace, accum=accum)
                assert plan.startswith("assign_scalar<"), plan
                with env(GRB_MI355X_ASSIGN_SCALAR=0):
                    host, plan0 = run(gb, Cm, s, rarg, carg, mask, struct=struct, comp=comp, replace=replace, accum=accum)
                assert plan0 == run.before, (plan0, run.before)     # the host-built block writes no plan string, as ever: it is what it was before the call
                same(dev, host, f"{ctyp} {block} device route vs host-built block")
                ran += 1
    assert ran == 96


# ---- 6. the fallbacks keep their answers ------------------------------------------------------------------------------------------------------------------
def test_a_repeated_index_keeps_the_host_built_block(gb, gpu, base):
    Cm = base["FP32"]
    gb.Matrix.from_lists([0], [0], [1], 2, 2, gb.INT32).mxv(gb.Vector.from_lists([0], [1], 2, gb.INT32), semiring=gb.INT32.PLUS_TIMES)      # (another call's plan string)
    for accum in (None, "PLUS"):
        for rarg, carg in (([7, 3, 7, 90], slice(2, 40, 3)), (slice(2, 40, 3), [7, 3, 7, 90])):
            got, plan = run(gb, Cm, 2, rarg, carg, accum=accum)
            assert plan == run.before and not plan.startswith("assign_scalar<"), plan
            rows, cols = ([7, 3, 90], list(range(2, 41, 3))) if isinstance(rarg, list) else (list(range(2, 41, 3)), [7, 3, 90])
            same(got, model.assign_scalar(Cm, 2, rows, cols, accum=(accum, "FP32") if accum else None), f"repeat, accum={accum}")


def test_hypersparse_and_complex_containers_keep_the_host_route(gb, gpu):
    H = gb.Matrix.sparse(gb.INT32)                                   # 2^60 x 2^60
    H[5, 1 << 40] = 7; H[1 << 50, 3] = 1
    H.assign_scalar(4, [5, 1 << 50], [3, 1 << 40], accum=gb.INT32.PLUS)
    assert not gb.last_kernel_plan().startswith("assign_scalar<")
    assert sorted(H) == [(5, 3, 4), (5, 1 << 40, 11), (1 << 50, 3, 5), (1 << 50, 1 << 40, 4)]
    Mh = gb.Matrix.sparse(gb.BOOL); Mh[1, 1] = True
    assert list(gb.Matrix.sparse(gb.FP64, fill=3.14, mask=Mh)) == [(1, 1, 3.14)] and list(gb.Matrix.sparse(gb.FP64, mask=Mh)) == [(1, 1, 0.0)]      # the reference's docstring, hypersparse as there

    class FC64(C.Structure):
        _fields_ = [("re", C.c_double), ("im", C.c_double)]
    lib, u64 = gb.lib, C.c_uint64
    fc64 = C.c_void_p.in_dll(lib, "GxB_FC64")
    lib.GxB_Matrix_setElement_FC64.argtypes = [C.c_void_p, FC64, u64, u64]
    Z = C.c_void_p()
    assert lib.GrB_Matrix_new(C.byref(Z), fc64, u64(4), u64(4)) == 0 and lib.GxB_Matrix_setElement_FC64(Z, FC64(1.0, 2.0), 1, 0) == 0
    rows, cols = (u64 * 2)(1, 3), (u64 * 2)(0, 2)
    assert lib.GrB_Matrix_assign_FP64(Z, None, None, C.c_double(2.5), rows, u64(2), cols, u64(2), None) == 0
    assert not gb.last_kernel_plan().startswith("assign_scalar<")
    nv, x = u64(0), FC64()
    assert lib.GrB_Matrix_nvals(C.byref(nv), Z) == 0 and nv.value == 4
    assert lib.GxB_Matrix_extractElement_FC64(C.byref(x), Z, u64(1), u64(0)) == 0 and (x.re, x.im) == (2.5, 0.0)
    assert lib.GrB_Matrix_free(C.byref(Z)) == 0


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------------------------------------
def small(gb):
    rng = np.random.default_rng(4900)
    Cm = random_mat(rng, 6, 7, "INT32", 15)
    Mm = random_mat(rng, 6, 7, "UINT8", 20, zeros=True)
    return Cm, Mm


def test_assign_scalar_argument_forms(gb, gpu):
    Cm, Mm = small(gb)
    forms = [((), {}, range(6), range(7)), ((2,), {}, [2], range(7)), ((None, 3), {}, range(6), [3]), ((slice(1, 4), slice(2, 5)), {}, range(1, 5), range(2, 6)),
             ((slice(5, 1, -2), [6, 0, 2]), {}, [5, 3, 1], [6, 0, 2]), ((np.array([4, 0], np.int32), slice(0, 6, 3)), {}, [4, 0], [0, 3, 6]), ((slice(None), slice(None, None, 2)), {}, range(6), [0, 2, 4, 6]),
             (((1, 2), range(3)), {}, [1, 2], [0, 1, 2])]
    for args, _, rows, cols in forms:
        for mask, comp, replace, accum in ((None, False, False, None), (None, False, False, "PLUS"), (Mm, False, False, None), (Mm, False, True, "MIN"), (Mm, True, False, "TIMES")):
            Cg = upload(gb, Cm)
            Cg.assign_scalar(9, *args, mask=upload(gb, mask) if mask is not None else None, accum=getattr(gb.INT32, accum) if accum else None, desc=descriptor(gb, comp=comp, replace=replace))
            same(download(Cg, "INT32"), model.assign_scalar(Cm, 9, rows, cols, mask, False, comp, replace, (accum, "INT32") if accum else None), f"assign_scalar{args} comp={comp} replace={replace} accum={accum}")


def test_setitem_scalar_branches(gb, gpu):
    Cm, Mm = small(gb)
    Bm = random_mat(np.random.default_rng(4901), 6, 7, "INT32", 12)
    allr, allc = range(6), range(7)
    cases = [(lambda A, M, B: A.__setitem__(M, 9), lambda: model.assign_scalar(Cm, 9, allr, allc, Mm)),
             (lambda A, M, B: A.__setitem__(M, B), lambda: mm.write_back(Cm, Bm, Mm)),
             (lambda A, M, B: A.__setitem__(2, 9), lambda: model.assign_scalar(Cm, 9, [2], allc)),
             (lambda A, M, B: A.__setitem__(slice(1, 3), 9), lambda: model.assign_scalar(Cm, 9, [1, 2, 3], allc)),
             (lambda A, M, B: A.__setitem__((4, slice(2, 5)), 9), lambda: model.assign_scalar(Cm, 9, [4], [2, 3, 4, 5])),
             (lambda A, M, B: A.__setitem__((slice(0, 4, 2), 6), 9), lambda: model.assign_scalar(Cm, 9, [0, 2, 4], [6])),
             (lambda A, M, B: A.__setitem__((slice(3, 5), slice(None)), 9), lambda: model.assign_scalar(Cm, 9, [3, 4, 5], allc)),
             (lambda A, M, B: A.__setitem__(([5, 0], [1, 6, 3]), 9), lambda: model.assign_scalar(Cm, 9, [5, 0], [1, 6, 3])),
             (lambda A, M, B: A.__setitem__((slice(None), slice(None)), 9), lambda: model.assign_scalar(Cm, 9, allr, allc)),
             (lambda A, M, B: A.__setitem__((1, 1), 9), lambda: model.assign_scalar(Cm, 9, [1], [1]))]
    for k, (do, expect) in enumerate(cases):
        A, M, B = upload(gb, Cm), upload(gb, Mm), upload(gb, Bm)
        do(A, M, B)
        same(download(A, "INT32"), expect(), f"__setitem__ case {k}")
    with pytest.raises(TypeError):
        upload(gb, Cm)[upload(gb, Mm)] = "x"
    with pytest.raises(TypeError):
        upload(gb, Cm)[2:3, 1:2] = "x"


def test_setitem_existing_branches_are_unchanged(gb, gpu):
    Cm, _ = small(gb)
    v7 = gb.Vector.from_lists([0, 3], [5, 6], 7, gb.INT32); v6 = gb.Vector.from_lists([1, 5], [5, 6], 6, gb.INT32)
    A = upload(gb, Cm); A[2] = v7
    assert (A[2].to_lists() == [[0, 3], [5, 6]])
    A = upload(gb, Cm); A[2, :] = v7
    assert (A[2].to_lists() == [[0, 3], [5, 6]])
    A = upload(gb, Cm); A[:, 4] = v6
    assert (A[:, 4].to_lists() == [[1, 5], [5, 6]])
    B = gb.Matrix.from_lists([0, 1], [1, 0], [8, 9], 2, 2, gb.INT32)
    A = upload(gb, Cm); A[1:2, 3:4] = B
    assert A[1:2, 3:4].to_lists() == [[0, 1], [1, 0], [8, 9]]
    A = upload(gb, Cm); A[0:1] = gb.Matrix.from_lists([0, 1], [1, 0], [8, 9], 2, 7, gb.INT32)
    assert A[0:1].to_lists() == [[0, 1], [1, 0], [8, 9]]


def test_reference_docstring_results(gb, gpu):
    with open(os.path.join(ROOT, "tests", "golden", "reference_assign_scalar_docs.json")) as f:
        doc = json.load(f)
    Mx = gb.Matrix.sparse(gb.BOOL, 3, 3)
    forms = {"assign_scalar()": lambda: Mx.assign_scalar(True), "M[:,:]": lambda: Mx.__setitem__((slice(None), slice(None)), True), "assign_scalar(1)": lambda: Mx.assign_scalar(True, 1),
             "M[1]": lambda: Mx.__setitem__(1, True), "M[1,:]": lambda: Mx.__setitem__((1, slice(None)), True), "assign_scalar(None,1)": lambda: Mx.assign_scalar(True, None, 1),
             "M[:,1]": lambda: Mx.__setitem__((slice(None), 1), True), "M[0:1,0:1]": lambda: Mx.__setitem__((slice(0, 1), slice(0, 1)), True)}
    assert sorted(forms) == sorted(c["form"] for c in doc["cases"])
    for case in doc["cases"]:
        Mx.clear()
        forms[case["form"]]()
        assert [[i, j] for i, j, x in Mx if x] == case["entries"] and Mx.nvals == len(case["entries"]), case["form"]
    Mx.clear()
    Mx[1] = gb.Vector.from_lists([0, 1], [True, True], 3)
    assert [[i, j] for i, j, x in Mx if x] == doc["row_vector"]["entries"]
    for case in doc["sparse_fill"]:
        mask = gb.Matrix.sparse(gb.BOOL, 4, 4); mask[tuple(case["mask_entry"])] = True
        kw = {} if case["fill"] is None else {"fill": case["fill"]}
        assert [list(t) for t in gb.Matrix.sparse(getattr(gb, case["type"]), 4, 4, mask=mask, **kw)] == case["tuples"]


def test_sparse_with_fill_and_mask(gb, gpu):
    n = 500
    Mm = random_mat(np.random.default_rng(4950), n, n, "UINT8", 4000, zeros=True)
    A = gb.Matrix.sparse(gb.FP64, n, n, fill=3.14, mask=upload(gb, Mm))
    assert "mask=pattern" in gb.last_kernel_plan()
    same(download(A, "FP64"), model.assign_scalar_restricted(mm.empty(n, n, "FP64"), 3.14, range(n), range(n), Mm), "Matrix.sparse(fill=, mask=)")
    assert gb.Matrix.sparse(gb.FP64, n, n, fill=3.14).nvals == 0 and gb.Matrix.sparse(gb.FP64, n, n).nvals == 0      # `fill` without a mask is ignored, as in the reference


# ---- 8. non-blocking mode -----------------------------------------------------------------------------------------------------------------------------------
def test_after_queued_vector_work(gb, gpu):
    """Element-wise vector work may still be queued when the matrix scalar assign is issued: a mask made from its result sees it, and work that stays queued
    across the assign is complete and right afterwards (the pattern of tests/test_nonblocking_gpu.py)."""
    n = 3000
    rng = np.random.default_rng(4990)
    ux, vx = rng.integers(1, 5, n).astype(np.float64), rng.integers(1, 5, n).astype(np.float64)
    idx = np.arange(n, dtype=np.uint64)
    u, v = gb.Vector.from_arrays(idx, ux, n, gb.FP64), gb.Vector.from_arrays(idx, vx, n, gb.FP64)
    w = u.eadd(v, gb.FP64.MINUS)                                     # queued: u - v, zero where they agree
    w = abs(w)
    z = u.emult(v, gb.FP64.TIMES)                                    # stays queued across the assign
    D = gb.Matrix.from_diag(w)                                       # reads w: its chain is completed first
    Cm = random_mat(rng, n, n, "FP64", 5000)
    Cg = upload(gb, Cm)
    Cg.assign_scalar(7.0, slice(100, 2900), None, mask=D)
    assert "mask=pattern" in gb.last_kernel_plan()
    d = np.abs(ux - vx)
    Dm = mm.Mat(n, n, np.arange(n, dtype=np.int64) * (n + 1), d)
    same(download(Cg, "FP64"), model.assign_scalar(Cm, 7.0, range(100, 2901), range(n), Dm), "assign after queued work")
    zi, zx = z.to_arrays()
    assert np.array_equal(zi, idx) and np.array_equal(zx, ux * vx)
