"""Sort and top-k on the device: grb_sort.hip behind GxB_Matrix_sort / GxB_Vector_sort / GrBX_*_select_topk, against the numpy model (tests/sort_model.py).

Sorting moves values and adds nothing, so every comparison is exact: values as bits, indices as integers; no tolerance occurs.  The row lengths sit at every edge
of the three bins (one wave up to 64, the LDS kernel up to its edge, the segmented radix sort beyond) and of the four-rows-per-wave packing (16), and the plan
string's bin counts are checked against counts made here.  The default route's edges are GrBX_sort_thresholds' (the LDS edge is the largest at which that bin did
not measure slower than the segmented sort); the LDS kernel has two shapes — one wave per row for edges up to LDS_WAVE_CAP, four waves up to its capacity
LDS_CAP — so every bin case runs three times: under the default edges and with GRB_MI355X_SORT_EDGES at each shape's capacity."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import sort_model as M

pytestmark = pytest.mark.gpu

NROWS = 300
LDS_CAP = 4096                      # the LDS kernel's capacity (grb_sort_keys.hpp SORT_LDS_MAX: 160 KiB / 2 workgroups / 12 bytes, rounded down to a power of two)
LDS_WAVE_CAP = 512                  # edges up to this run the LDS kernel with one wave per row (grb_sort.hip SORT_LDS_WAVE_MAX)
EDGES = [None, "64,%d" % LDS_WAVE_CAP, "64,%d" % LDS_CAP]   # the default edges, and each shape of the LDS kernel at its capacity
EDGE_IDS = ["default-edges", "lds-one-wave-at-capacity", "lds-four-waves-at-capacity"]


@contextlib.contextmanager
def hook(value, name="GRB_MI355X_SORT"):
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(value)
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def edges_hook(edges):
    return hook(edges, "GRB_MI355X_SORT_EDGES")


def bin_counts(gb, lens, edges):
    """(wave, lds, prim) rows for the edges in force, counted here from the row lengths."""
    wave_max, lds_max = thresholds(gb) if edges is None else tuple(int(x) for x in edges.split(","))
    return int((lens <= wave_max).sum()), int(((lens > wave_max) & (lens <= lds_max)).sum()), int((lens > lds_max).sum())


def thresholds(gb):
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert gb.lib.GrBX_sort_thresholds(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def same(got, want):
    return got.dtype == want.dtype and np.array_equal(M.bits(got), M.bits(want))


def bins_of(plan):
    m = re.search(r"wave=(\d+),lds=(\d+),prim=(\d+)", plan)
    assert m, plan
    return tuple(int(g) for g in m.groups())


_structure = {}


def edge_structure(gb):
    """300 rows whose lengths sit at every edge: 0, 1, 2, 15, 16, 17, 63, 64, 65, then d - 1, d, d + 1 for the default LDS edge d, for LDS_WAVE_CAP and for
    LDS_CAP, and 4 LDS_CAP + 3 (the four longest lengths three times each, the others 19 times, three more empty rows), shuffled.  Made once and shared; never written to."""
    if not _structure:
        wave_max, lds_max = 64, LDS_CAP
        d = thresholds(gb)[1]
        assert thresholds(gb)[0] == wave_max and wave_max < d <= lds_max
        rng = np.random.default_rng(11)
        long_lens = [lds_max - 1, lds_max, lds_max + 1, 4 * lds_max + 3]
        lens = np.array(long_lens * 3 + [0, 1, 2, 15, 16, 17, 63, 64, 65, d - 1, d, d + 1, LDS_WAVE_CAP - 1, LDS_WAVE_CAP, LDS_WAVE_CAP + 1] * 19 + [0] * 3, np.int64)
        assert len(lens) == NROWS
        rng.shuffle(lens)
        ncols = 4 * lds_max + 20
        I = np.repeat(np.arange(NROWS), lens).astype(np.uint64)
        J = np.concatenate([np.sort(rng.choice(ncols, size=k, replace=False)) for k in lens]).astype(np.uint64)
        _structure.update(lens=lens, ncols=ncols, I=I, J=J)
        assert all(all(bin_counts(gb, lens, e)) for e in EDGES), "rows in all three bins under every setting"
        I.setflags(write=False)
        J.setflags(write=False)
    return _structure


def edge_values(rng, gb, name, n):
    dt = getattr(gb, name)._np
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    if name in ("FP32", "FP64"):
        return rng.standard_normal(n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def tie_values(rng, gb, name, n):
    """Three distinct numbers, so almost everything ties; NaN, both zeros and both infinities for floats, the type's minimum and maximum for integers."""
    dt = getattr(gb, name)._np
    if name in ("FP32", "FP64"):
        pool = np.array([2.5, -7.0, 0.125, np.nan, 0.0, -0.0, np.inf, -np.inf], dt)
        p = np.array([0.3, 0.3, 0.3, 0.02, 0.02, 0.02, 0.02, 0.02])
    else:
        info = np.iinfo(dt)
        pool = np.array([3, -4 if info.min < 0 else 4, 100, info.min, info.max], dt)
        p = np.array([0.32, 0.32, 0.32, 0.02, 0.02])
    return pool[rng.choice(len(pool), size=n, p=p)]


def check_sort(gb, I, J, X, nrows, ncols, typ, gt, by_col=False, key=None, ctype=None):
    """C and P of one call against the model; returns the plan string."""
    A = gb.Matrix.from_arrays(I, J, X, nrows, ncols, typ)
    wi, wj, wx, wp = M.matrix_sort(I, J, X, gt=gt, by_col=by_col, key_dtype=key._np if key else None)
    opt = key or typ
    Cm = gb.Matrix.sparse(ctype or typ, nrows, ncols)
    Pm = gb.Matrix.sparse(gb.INT64, nrows, ncols)
    desc = C.c_void_p(gb.descriptor.T0.get_desc()) if by_col else None
    assert gb.lib.GxB_Matrix_sort(Cm._h, Pm._h, C.c_void_p((opt.GT if gt else opt.LT).get_op()), A._h, desc) == 0
    plan = gb.last_kernel_plan()
    assert residency(gb, Cm) == 2 and residency(gb, Pm) == 2, "the outputs live in HBM, their host mirrors are invalid"
    ci, cj, cx = Cm.to_arrays()
    pi, pj, px = Pm.to_arrays()
    assert np.array_equal(ci, wi) and np.array_equal(cj, wj) and np.array_equal(pi, wi) and np.array_equal(pj, wj), "pattern"
    assert same(cx, M.cast(wx, ctype._np) if ctype else wx), "values"
    assert same(px, wp), "permutation"
    return plan


@pytest.mark.parametrize("edges", EDGES, ids=EDGE_IDS)
@pytest.mark.parametrize("gt", [False, True], ids=["lt", "gt"])
@pytest.mark.parametrize("name", ["FP64", "FP32", "INT64", "UINT64", "INT8", "BOOL"])
def test_row_lengths_at_every_edge(gb, gpu, name, gt, edges):
    s = edge_structure(gb)
    rng = np.random.default_rng(2 * ["FP64", "FP32", "INT64", "UINT64", "INT8", "BOOL"].index(name) + int(gt))
    X = edge_values(rng, gb, name, len(s["I"]))
    with edges_hook(edges):
        plan = check_sort(gb, s["I"], s["J"], X, NROWS, s["ncols"], getattr(gb, name), gt)
    assert plan.startswith("sort<on=matrix,by=row,op=%s,key=%d," % ("gt" if gt else "lt", 64 if name in ("FP64", "INT64", "UINT64") else 32)), plan
    want = bin_counts(gb, s["lens"], edges)
    assert bins_of(plan) == want, plan
    for k in ("k_sort_bins", "k_sort_wave", "segmented_radix_sort", "k_sort_gather"):
        assert k in plan, plan
    assert ("k_sort_lds" in plan) == (want[1] > 0), plan
    assert "k_cast_values" not in plan, "the operator's type is A's: no cast pass"


@pytest.mark.parametrize("edges", EDGES, ids=EDGE_IDS)
@pytest.mark.parametrize("gt", [False, True], ids=["lt", "gt"])
@pytest.mark.parametrize("name", ["FP32", "FP64", "INT64", "INT8"])
def test_ties(gb, gpu, name, gt, edges):
    s = edge_structure(gb)
    rng = np.random.default_rng(5)
    X = tie_values(rng, gb, name, len(s["I"]))
    with edges_hook(edges):
        plan = check_sort(gb, s["I"], s["J"], X, NROWS, s["ncols"], getattr(gb, name), gt)
    assert bins_of(plan) == bin_counts(gb, s["lens"], edges), plan


@pytest.mark.parametrize("name,gt", [("FP32", False), ("INT64", True)])
def test_past_one_grid_round(gb, gpu, name, gt):
    """200 000 rows of 1 .. 8 entries (more four-row groups than waves in flight) and one row of 300 000 entries."""
    rng = np.random.default_rng(3)
    nshort, big = 200000, 300000
    lens = np.r_[rng.integers(1, 9, nshort), big].astype(np.int64)
    nrows, ncols = nshort + 1, 310000
    I = np.repeat(np.arange(nrows), lens).astype(np.uint64)
    start = np.repeat(np.cumsum(lens) - lens, lens)
    within = np.arange(len(I)) - start
    first, step = np.repeat(np.r_[rng.integers(0, 1000, nshort), 0], lens), np.repeat(np.r_[rng.integers(1, 1000, nshort), 1], lens)
    J = (first + within * step).astype(np.uint64)
    X = rng.integers(-20, 20, len(I)).astype(getattr(gb, name)._np)
    plan = check_sort(gb, I, J, X, nrows, ncols, getattr(gb, name), gt)
    assert bins_of(plan) == (nshort, 0, 1), plan


def test_by_column_and_the_output_variants(gb, gpu):
    rng = np.random.default_rng(9)
    nrows, ncols = 500, 700
    flat = np.sort(rng.choice(nrows * ncols, size=int(nrows * ncols * 0.05), replace=False))
    I, J = np.divmod(flat.astype(np.uint64), np.uint64(ncols))
    X = (rng.integers(-400, 400, len(flat)) / 8.0).astype(np.float64)
    for gt in (False, True):
        plan = check_sort(gb, I, J, X, nrows, ncols, gb.FP64, gt, by_col=True)
        assert "by=col" in plan and "csr_transpose" in plan, plan
        # the by-column result is the by-row result of the transpose, transposed
        A = gb.Matrix.from_arrays(I, J, X, nrows, ncols, gb.FP64)
        op = gb.FP64.GT if gt else gb.FP64.LT
        Cc, Pc = A.sort(op=op, desc=gb.descriptor.T0)
        Ct, Pt = A.transpose().sort(op=op)
        for got, via in ((Cc, Ct.transpose()), (Pc, Pt.transpose())):
            g, v = got.to_arrays(), via.to_arrays()
            assert np.array_equal(g[0], v[0]) and np.array_equal(g[1], v[1]) and same(g[2], v[2])
        # C only, P only, C is A
        wi, wj, wx, wp = M.matrix_sort(I, J, X, gt=gt)
        Conly, none = A.sort(op=op, perm=False)
        none2, Ponly = A.sort(op=op, values=False)
        assert none is None and none2 is None and same(Conly.to_arrays()[2], wx) and same(Ponly.to_arrays()[2], wp) and np.array_equal(Ponly.to_arrays()[1], wj)
        assert gb.lib.GxB_Matrix_sort(A._h, None, C.c_void_p(op.get_op()), A._h, None) == 0
        assert residency(gb, A) == 2
        ai, aj, ax = A.to_arrays()
        assert np.array_equal(ai, wi) and np.array_equal(aj, wj) and same(ax, wx)
        assert A.nvals == len(wx) and same(A.sort(op=op)[0].to_arrays()[2], wx), "what was derived from the old image of A is gone: sorting the sorted matrix again reads the new one"
    # a cast by C (FP64 A into an INT32 C), and a cast by the operator (GrB_LT_INT32 on FP64 values)
    check_sort(gb, I, J, X, nrows, ncols, gb.FP64, False, ctype=gb.INT32)
    plan = check_sort(gb, I, J, X, nrows, ncols, gb.FP64, False, key=gb.INT32)
    assert "key=32" in plan and "k_cast_values" in plan, plan
    assert not np.array_equal(M.matrix_sort(I, J, X, key_dtype=np.int32)[3], M.matrix_sort(I, J, X)[3]), "the case must tell the two comparison types apart"
    plan = check_sort(gb, I, J, X, nrows, ncols, gb.FP64, True, by_col=True, key=gb.INT32, ctype=gb.INT32)


@pytest.mark.parametrize("density", [0.01, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 64, 65, 1000003])
def test_vector(gb, gpu, n, density):
    rng = np.random.default_rng(n % 97 + int(density * 100))
    nv = int(round(n * density))
    idx = np.sort(rng.choice(n, size=nv, replace=False)).astype(np.uint64)
    for name, gt in (("FP32", False), ("FP64", True), ("INT8", True), ("UINT64", False)):
        typ = getattr(gb, name)
        x = tie_values(rng, gb, name, nv) if name in ("FP32", "INT8") else edge_values(rng, gb, name, nv)
        wx, px = M.vector_sort(idx, x, gt=gt)
        u = gb.Vector.from_arrays(idx, x, n, typ)
        with hook(1):                                                       # (the small ones would take the host route by themselves)
            w, p = u.sort(op=typ.GT if gt else typ.LT)
            plan = gb.last_kernel_plan()
            assert plan.startswith("sort<on=vector,op=%s,key=%d,nvals=%d>" % ("gt" if gt else "lt", 64 if name in ("FP64", "UINT64") else 32, nv)), plan
            assert residency(gb, w) == 2 and residency(gb, p) == 2
            gi, gx = w.to_arrays()
            hi, hx = p.to_arrays()
            # the presence bytes form exactly the prefix 0 .. nvals - 1
            assert np.array_equal(gi, np.arange(nv, dtype=np.uint64)) and np.array_equal(hi, gi) and w.nvals == nv and p.nvals == nv
            assert same(gx, wx) and same(hx, px), (name, n, density)
            for k in (0, 1, 7, nv + 1):
                ti, tx = M.vector_topk(idx, x, k, gt=gt)
                t = u.topk(k, largest=gt)
                assert gb.last_kernel_plan().startswith("topk<on=vector,") and residency(gb, t) == 2
                oi, ox = t.to_arrays()
                assert np.array_equal(oi, ti) and same(ox, tx), (name, n, density, k)
            assert gb.lib.GxB_Vector_sort(u._h, None, C.c_void_p((typ.GT if gt else typ.LT).get_op()), u._h, None) == 0      # w is u
            assert same(u.to_arrays()[1], wx)


@pytest.mark.parametrize("edges", EDGES, ids=EDGE_IDS)
@pytest.mark.parametrize("name,gt", [("INT8", True), ("FP64", False), ("FP32", True)])
def test_topk(gb, gpu, name, gt, edges):
    s = edge_structure(gb)
    lds_max = LDS_CAP
    rng = np.random.default_rng(21)
    typ = getattr(gb, name)
    X = tie_values(rng, gb, name, len(s["I"]))
    op = C.c_void_p((typ.GT if gt else typ.LT).get_op())
    # a row in which the k-th and the (k + 1)-th value tie, for every k used below that a row is long enough for
    _, _, sx, _ = M.matrix_sort(s["I"], s["J"], X, gt=gt)
    longest = int(np.argmax(s["lens"]))
    row = sx[np.cumsum(s["lens"])[longest] - s["lens"][longest]:np.cumsum(s["lens"])[longest]]
    for k in (1, 64, 65, thresholds(gb)[1] + 1, lds_max + 1):
        a, b = row[k - 1], row[k]
        assert a == b or (a != a and b != b), "the test's own premise: a tie across the cut"
    for k in (0, 1, 64, 65, thresholds(gb)[1] + 1, lds_max + 1):
        A = gb.Matrix.from_arrays(s["I"], s["J"], X, NROWS, s["ncols"], typ)
        out = gb.Matrix.sparse(typ, NROWS, s["ncols"])
        with edges_hook(edges):
            assert gb.lib.GrBX_Matrix_select_topk(out._h, op, A._h, C.c_uint64(k), None) == 0
        plan = gb.last_kernel_plan()
        assert plan.startswith("topk<on=matrix,by=row,") and (",k=%d>" % k) in plan and bins_of(plan) == bin_counts(gb, s["lens"], edges), plan
        assert residency(gb, out) == 2
        oi, oj, ox = out.to_arrays()
        ti, tj, tx = M.matrix_topk(s["I"], s["J"], X, k, gt=gt)
        assert np.array_equal(np.bincount(oi.astype(np.int64), minlength=NROWS), np.minimum(k, s["lens"])), "min(k, len) entries per row"
        have = set(zip(s["I"].tolist(), s["J"].tolist()))
        assert all(c in have for c in zip(oi.tolist(), oj.tolist())), "the pattern is a subset of A's"
        assert np.array_equal(oi, ti) and np.array_equal(oj, tj) and same(ox, tx), (name, gt, k)
    # per column, and C is A
    A = gb.Matrix.from_arrays(s["I"], s["J"], X, NROWS, s["ncols"], typ)
    ti, tj, tx = M.matrix_topk(s["I"], s["J"], X, 2, gt=gt, by_col=True)
    assert gb.lib.GrBX_Matrix_select_topk(A._h, op, A._h, C.c_uint64(2), C.c_void_p(gb.descriptor.T0.get_desc())) == 0
    assert "by=col" in gb.last_kernel_plan() and residency(gb, A) == 2
    oi, oj, ox = A.to_arrays()
    assert np.array_equal(oi, ti) and np.array_equal(oj, tj) and same(ox, tx)


@pytest.mark.parametrize("edges", EDGES, ids=EDGE_IDS)
def test_prim_route_gives_identical_bits(gb, gpu, edges):
    s = edge_structure(gb)
    rng = np.random.default_rng(33)
    for name, gt in (("FP64", False), ("FP32", True), ("INT8", False)):
        typ = getattr(gb, name)
        X = tie_values(rng, gb, name, len(s["I"]))
        A = gb.Matrix.from_arrays(s["I"], s["J"], X, NROWS, s["ncols"], typ)
        op = typ.GT if gt else typ.LT
        with edges_hook(edges):
            Cd, Pd = A.sort(op=op)
        assert bins_of(gb.last_kernel_plan()) == bin_counts(gb, s["lens"], edges)
        with hook("prim"):
            Cp, Pp = A.sort(op=op)
            assert bins_of(gb.last_kernel_plan()) == (0, 0, NROWS), gb.last_kernel_plan()
            Tp = A.topk(65, largest=gt)
        with edges_hook(edges):
            Td = A.topk(65, largest=gt)
        for d, p in ((Cd, Cp), (Pd, Pp), (Td, Tp)):
            assert residency(gb, d) == 2 and residency(gb, p) == 2
            a, b = d.to_arrays(), p.to_arrays()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same(a[2], b[2])
        with hook(0):
            Ch, Ph = A.sort(op=op)
            assert gb.last_kernel_plan() == ""
        assert same(Ch.to_arrays()[2], Cd.to_arrays()[2]) and same(Ph.to_arrays()[2], Pd.to_arrays()[2]), "the host route agrees as well"


def test_python_surface(gb, gpu):
    """Matrix.topk(2) of the 7-vertex docstring graph (edge e carries the value e): only vertex 6 has more than two out-edges, and loses its lightest one."""
    I = [0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 6, 6]
    J = [1, 3, 4, 6, 5, 0, 2, 5, 2, 2, 3, 4]
    A = gb.Matrix.from_lists(I, J, list(range(12)), 7, 7)
    want = [(0, 1, 0), (0, 3, 1), (1, 4, 2), (1, 6, 3), (2, 5, 4), (3, 0, 5), (3, 2, 6), (4, 5, 7), (5, 2, 8), (6, 3, 10), (6, 4, 11)]
    with hook(1):
        T = A.topk(2)
        assert gb.last_kernel_plan().startswith("topk<on=matrix,by=row,op=gt,key=64,wave=7,lds=0,prim=0,k=2>"), gb.last_kernel_plan()
        assert sorted(T) == want
        assert sorted(A.topk(1, largest=False)) == [(0, 1, 0), (1, 4, 2), (2, 5, 4), (3, 0, 5), (4, 5, 7), (5, 2, 8), (6, 2, 9)]
        Cm, Pm = A.sort(op=gb.INT64.GT)
        assert sorted(Cm)[-3:] == [(6, 0, 11), (6, 1, 10), (6, 2, 9)] and sorted(Pm)[-3:] == [(6, 0, 4), (6, 1, 3), (6, 2, 2)]
    assert sorted(A.topk(2)) == want, "and the host route of the same call"
