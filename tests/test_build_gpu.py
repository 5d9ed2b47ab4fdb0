"""Build from tuples on the device (grb_build.hip) against the host route of the same call (GRB_MI355X_BUILD=0: the code every earlier version ran) and the numpy
model (tests/build_model.py), BIT FOR BIT: rowptr / col / val of GrBX_Matrix_export_CSR, values / presence of GrBX_Vector_export_Bitmap, the values compared as
bytes (NaN payloads and -0.0 count).  There is no tolerance; the one place where the sign of a zero is left open is test_signed_zeros_in_min_max_runs, which says
why.  test_the_largest_dimensions is device-only (a 16 GiB row pointer has no affordable host twin) and checks a hand-computed result.  GRB_MI355X_BUILD=1 is set around every device call, so the sizes can stay small."""
import contextlib
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import build_model as bm
import operator_model as om

pytestmark = pytest.mark.gpu
INVALID_VALUE, OUTPUT_NOT_EMPTY, INDEX_OUT_OF_BOUNDS = 5, 9, 12
DIM_MAX = 0xFFFFFFF0
GRID_ROUND = 4096 * 256                                               # one round of grid_1d's capped grid


@contextlib.contextmanager
def route(value):
    old = os.environ.get("GRB_MI355X_BUILD")
    if value is None: os.environ.pop("GRB_MI355X_BUILD", None)
    else: os.environ["GRB_MI355X_BUILD"] = value
    try:
        yield
    finally:
        if old is None: os.environ.pop("GRB_MI355X_BUILD", None)
        else: os.environ["GRB_MI355X_BUILD"] = old


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def thresholds(gb):
    out = (C.c_uint64 * 3)()
    assert gb.lib.GrBX_build_thresholds(out) == 0
    return [int(v) for v in out]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def residency(gb, x):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(x, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(x._h, C.byref(w)) == 0
    return w.value


def check_matrix(gb, t, I, J, X, nrows, ncols, op, expect_device=True, model=True):
    """Device build == host build == model; returns (device matrix, its plan)."""
    typ = getattr(gb, t); dup = getattr(typ, op) if op else None
    I = np.ascontiguousarray(I, np.uint64); J = np.ascontiguousarray(J, np.uint64); X = np.ascontiguousarray(X, typ._np)
    with route("1"):
        D = gb.Matrix.from_arrays(I, J, X, nrows, ncols, typ, dup=dup)
        plan = gb.last_kernel_plan()
    if expect_device:
        assert plan.startswith("build<type=" + t + ",dup=" + (op or "none") + ","), plan
        assert residency(gb, D) == 2, "a device build leaves the container in HBM only"
    else:
        assert "build<" not in plan, plan
    with route("0"):
        H = gb.Matrix.from_arrays(I, J, X, nrows, ncols, typ, dup=dup)
        assert "build<" not in gb.last_kernel_plan()
    drp, dci, dx = D.to_csr(); hrp, hci, hx = H.to_csr()
    assert np.array_equal(drp, hrp) and np.array_equal(dci, hci) and bits_equal(dx, hx), (t, op, len(I), plan)
    if model:
        rows, cols, vals = bm.build(t, I, J, X, nrows, ncols, op)
        assert np.array_equal(drp, bm.rowptr(rows, nrows)) and np.array_equal(dci, cols.astype(np.uint32)) and bits_equal(dx, vals), (t, op, len(I), plan)
    return D, plan


def check_vector(gb, t, I, X, size, op):
    typ = getattr(gb, t); dup = getattr(typ, op) if op else None
    I = np.ascontiguousarray(I, np.uint64); X = np.ascontiguousarray(X, typ._np)
    with route("1"):
        d = gb.Vector.from_arrays(I, X, size, typ, dup=dup)
        plan = gb.last_kernel_plan()
    assert plan.startswith("build<type=" + t) and residency(gb, d) == 2, plan
    with route("0"):
        h = gb.Vector.from_arrays(I, X, size, typ, dup=dup)
    dx, dp = d.to_dense_arrays(); hx, hp = h.to_dense_arrays()
    assert np.array_equal(dp, hp) and bits_equal(dx, hx), (t, op, len(I))
    rows, _, vals = bm.build(t, I, None, X, size, 1, op)
    want_p = np.zeros(size, np.uint8); want_p[rows.astype(np.int64)] = 1
    want_x = np.zeros(size, typ._np); want_x[rows.astype(np.int64)] = vals
    assert np.array_equal(dp, want_p) and bits_equal(dx, want_x), (t, op, len(I))
    return d, plan, len(rows)


def values(t, rng, n):
    if t == "BOOL": return rng.integers(0, 2, n).astype(np.bool_)
    if om.is_fp(t): return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 17, n)).astype(om.NP[t])
    info = np.iinfo(om.NP[t])
    return rng.integers(info.min, info.max, n, dtype=om.NP[t], endpoint=True)


def tuples(rng, n, nrows, ncols, dup_share=0.05):
    """n tuples, about dup_share of them on the position of another one, in random order."""
    flat = rng.integers(0, nrows * ncols, n).astype(np.uint64)
    k = int(n * dup_share)
    if k: flat[rng.choice(n, k, replace=False)] = flat[rng.integers(0, n, k)]
    return flat // np.uint64(ncols), flat % np.uint64(ncols)


def with_run(t, rng, length, run_values=None, before=40, after=40, nrows=97, ncols=89, run_at=None):
    """Singletons and one run of `length` tuples on one position, shuffled over the input (the run keeps the relative order of run_values)."""
    npos = before + after + 1
    flat = np.sort(rng.choice(np.arange(1, nrows * ncols - 1), size=npos, replace=False)) if run_at is None else None
    if run_at == "first": flat = np.concatenate([[0], np.sort(rng.choice(np.arange(1, nrows * ncols), size=npos - 1, replace=False))]); before = 0
    if run_at == "last": flat = np.concatenate([np.sort(rng.choice(nrows * ncols - 1, size=npos - 1, replace=False)), [nrows * ncols - 1]]); before = npos - 1
    rv = values(t, rng, length) if run_values is None else np.asarray(run_values, om.NP[t])
    total = npos - 1 + length
    slots = np.sort(rng.choice(total, length, replace=False))         # where the run's members stand in the input, in their own order
    rest = np.setdiff1d(np.arange(total), slots)
    pos = np.zeros(total, np.uint64); X = np.zeros(total, om.NP[t])
    pos[slots] = flat[before]; X[slots] = rv
    pos[rest] = rng.permutation(np.delete(flat, before)); X[rest] = values(t, rng, npos - 1)
    return pos // np.uint64(ncols), pos % np.uint64(ncols), X, nrows, ncols


# ---- sizes x value widths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,op", [("BOOL", "LOR"), ("INT16", "PLUS"), ("FP32", "PLUS"), ("INT64", "MIN"), ("FP64", "PLUS")])
def test_sizes_and_value_widths(gb, gpu, t, op):
    rng = np.random.default_rng(11)
    for n in (0, 1, 255, 256, 257, GRID_ROUND + 300):
        dim = max(4, int(np.sqrt(4 * n)) + 1)
        I, J = tuples(rng, n, dim, dim)
        _, plan = check_matrix(gb, t, I, J, values(t, rng, n), dim, dim, op)
        if n > 256: assert "sorted=0" in plan and "fold=serial" in plan, plan
        if n in (257, GRID_ROUND + 300):
            K = I * np.uint64(dim) + J
            _, _, nv = check_vector(gb, t, K, values(t, rng, n), dim * dim, op)


# ---- run lengths ------------------------------------------------------------------------------------------------------------------
def test_run_lengths(gb, gpu):
    _, serial, serial_max = thresholds(gb)
    rng = np.random.default_rng(12)
    for length in (1, 2, serial, serial + 1, 64, 65, 129, serial_max):
        for t, op, fold_long in (("FP64", "PLUS", "serial"), ("INT64", "PLUS", "wave"), ("FP32", "MAX", "wave"), ("INT32", "MINUS", "serial")):
            I, J, X, nr, nc = with_run(t, rng, length)
            _, plan = check_matrix(gb, t, I, J, X, nr, nc, op)
            want = "fold=none" if length == 1 else ("fold=" + fold_long if length > serial else "fold=serial")
            assert want in plan, (length, t, op, plan)


def test_run_beyond_the_serial_limit(gb, gpu):
    _, serial, serial_max = thresholds(gb)
    rng = np.random.default_rng(13)
    I, J, X, nr, nc = with_run("FP64", rng, serial_max + 1)
    check_matrix(gb, "FP64", I, J, X, nr, nc, "PLUS", expect_device=False)      # not exactly associative: the whole call keeps the host route
    I, J, X, nr, nc = with_run("INT64", rng, serial_max + 1)
    _, plan = check_matrix(gb, "INT64", I, J, X, nr, nc, "PLUS")
    assert "fold=wave" in plan, plan


# ---- run placement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last"])
def test_run_at_the_ends(gb, gpu, where):
    rng = np.random.default_rng(14)
    for length in (3, 70):
        I, J, X, nr, nc = with_run("FP64", rng, length, run_at=where)
        check_matrix(gb, "FP64", I, J, X, nr, nc, "PLUS")
        check_matrix(gb, "INT16", I, J, values("INT16", rng, len(I)), nr, nc, "SECOND")


def test_run_across_a_workgroup_boundary_of_the_sorted_order(gb, gpu):
    rng = np.random.default_rng(15)
    for length, before in ((20, 250), (100, 200), (300, 500)):          # sorted positions 250..269, 200..299, 500..799
        I, J, X, nr, nc = with_run("FP64", rng, length, before=before, after=300, nrows=211, ncols=199)
        check_matrix(gb, "FP64", I, J, X, nr, nc, "PLUS")
        check_matrix(gb, "FP64", I, J, X, nr, nc, "FIRST")


@pytest.mark.parametrize("t,op", [("INT32", "PLUS"), ("FP64", "SECOND")])
def test_all_tuples_on_one_position(gb, gpu, t, op):
    rng = np.random.default_rng(16)
    n = 10000
    X = values(t, rng, n)
    D, plan = check_matrix(gb, t, np.full(n, 5), np.full(n, 7), X, 9, 11, op)
    assert D.nvals == 1 and "fold=wave" in plan
    d, _, nv = check_vector(gb, t, np.full(n, 3), X, 8, op)
    assert d.nvals == 1


# ---- order ------------------------------------------------------------------------------------------------------------------------
def test_every_input_order_of_a_cancelling_sum(gb, gpu):
    seen = set()
    for order in itertools.permutations(range(4)):
        X = np.array([[1e16, 1.0, -1e16, 1.0][k] for k in order] + [2.5])
        D, _ = check_matrix(gb, "FP64", [3, 3, 3, 3, 0], [1, 1, 1, 1, 2], X, 4, 4, "PLUS")
        seen.add(float(D.to_csr()[2][1]))
    assert seen >= {0.0, 1.0}


def test_selectors_take_the_element_the_input_order_names(gb, gpu):
    rng = np.random.default_rng(17)
    for t in ("FP64", "INT32", "UINT8"):
        run = (np.arange(200) + 1).astype(om.NP[t])                   # 200 distinct values
        I, J, X, nr, nc = with_run(t, rng, 200, run_values=run)
        for op, want in (("FIRST", run[0]), ("SECOND", run[-1]), ("ANY", None)):
            D, plan = check_matrix(gb, t, I, J, X, nr, nc, op)
            assert "fold=wave" in plan
            if want is not None:
                ri, rj = [(int(i), int(j)) for i, j in zip(I, J) if np.sum((I == i) & (J == j)) == 200][0]      # the run's position
                rp, ci, x = D.to_csr()
                at = rp[ri] + np.flatnonzero(ci[rp[ri]:rp[ri + 1]] == rj)
                assert len(at) == 1 and x[at[0]] == want, (t, op)


def test_nan_in_min_max_runs(gb, gpu):
    rng = np.random.default_rng(18)
    for t in ("FP32", "FP64"):
        for length in (3, 40, 130):
            run = (rng.standard_normal(length) * 100).astype(om.NP[t]); run[run == 0] = 1
            run[rng.integers(0, length)] = np.nan
            for op in ("MIN", "MAX"):
                I, J, X, nr, nc = with_run(t, rng, length, run_values=run)
                check_matrix(gb, t, I, J, X, nr, nc, op)
        allnan = np.full(5, np.nan, om.NP[t])
        I, J, X, nr, nc = with_run(t, rng, 5, run_values=allnan)
        check_matrix(gb, t, I, J, X, nr, nc, "MIN")


# ---- keys -------------------------------------------------------------------------------------------------------------------------
def test_key_layouts(gb, gpu):
    rng = np.random.default_rng(19)
    for nrows, ncols, key in ((1, 1, "u32"), (1, 300, "u32"), (300, 1, "u32"), (1 << 16, 1 << 16, "u32"), ((1 << 16) + 1, 1 << 16, "u64"), (1 << 16, (1 << 16) + 1, "u64")):
        n = 400
        I, J = tuples(rng, n, nrows, ncols) if nrows * ncols > 1 else (np.zeros(n, np.uint64), np.zeros(n, np.uint64))
        I[:3] = nrows - 1; J[:3] = ncols - 1; I[3] = 0; J[3] = 0      # the extreme index, as a run of three, and the origin
        _, plan = check_matrix(gb, "FP64", I, J, values("FP64", rng, n), nrows, ncols, "PLUS")
        assert "key=" + key in plan, (nrows, ncols, plan)


def test_the_largest_column_dimension(gb, gpu):
    """ncols = GRB_DIM_DEVICE_MAX with an entry in the last column (cbits = 32, 64-bit keys).  The same number of ROWS would need a 16 GiB row pointer on both
    routes (tens of seconds of host time on the twin): the row side of the packing at that dimension is checked by tests/build_keys_check.cpp."""
    I = [2, 0, 2, 1]; J = [DIM_MAX - 1, 5, DIM_MAX - 1, DIM_MAX - 2]
    D, plan = check_matrix(gb, "INT64", I, J, [7, 8, 9, 10], 3, DIM_MAX, "PLUS")
    assert "key=u64" in plan
    rp, ci, x = D.to_csr()
    assert rp.tolist() == [0, 1, 2, 3] and ci.tolist() == [5, DIM_MAX - 2, DIM_MAX - 1] and x.tolist() == [8, 10, 16]


def test_the_largest_dimensions(gb, gpu):
    """nrows = ncols = GRB_DIM_DEVICE_MAX with entries at (dim - 1, dim - 1): rbits = cbits = 32, the extreme 64-bit key, and a row pointer of 2^32 - 15 words
    (16 GiB) written by the per-row bisection.  Device only: a host twin would build that row pointer on one thread.  Checked against the result worked out
    by hand: nvals, the plan, col / val through export_CSR, and the row pointer compared in HBM (exported to a device tensor, never brought to the host)."""
    torch = pytest.importorskip("torch")
    last = DIM_MAX - 1
    I = np.array([last, 5, last, 0, last, 5], np.uint64); J = np.array([last, 7, last, 0, 3, 7], np.uint64); X = np.array([1, 2, 4, 8, 16, 32], np.int64)
    with route("1"):
        D = gb.Matrix.from_arrays(I, J, X, DIM_MAX, DIM_MAX, gb.INT64, dup=gb.INT64.PLUS)
        plan = gb.last_kernel_plan()
    assert plan.startswith("build<type=INT64,dup=PLUS,key=u64,sorted=0,fold=serial,rows=search>"), plan
    assert residency(gb, D) == 2 and D.nvals == 4
    ci, x = np.zeros(4, np.uint32), np.zeros(4, np.int64)
    rp = torch.empty(DIM_MAX + 1, dtype=torch.int32, device="cuda")
    assert gb.lib.GrBX_Matrix_export_CSR(D._h, C.c_void_p(rp.data_ptr()), None, None, 1) == 0
    assert gb.lib.GrBX_Matrix_export_CSR(D._h, None, _p(ci), _p(x), 0) == 0
    assert ci.tolist() == [0, 7, 3, last] and x.tolist() == [8, 34, 16, 5]
    # rows 0, 5 and dim - 1 hold 1, 1 and 2 entries: rowptr is 0 | 1 x5 | 2 up to row dim - 1 | 4
    assert rp[0].item() == 0 and bool((rp[1:6] == 1).all()) and bool((rp[6:DIM_MAX] == 2).all()) and rp[DIM_MAX].item() == 4
    del rp, D
    torch.cuda.empty_cache()
    with route("1"):                                                  # the same length as a vector: the last index present, a duplicate on it
        v = gb.Vector.from_arrays(np.array([last, 9, last], np.uint64), np.array([True, False, True]), DIM_MAX, gb.BOOL, dup=gb.BOOL.LOR)
        assert gb.last_kernel_plan().startswith("build<type=BOOL,dup=LOR,key=u32")
    assert residency(gb, v) == 2 and v.nvals == 2 and v[last] is True and v[9] is False
    from pygraphblas_amd.base import NoValue
    with pytest.raises(NoValue):
        v[last - 1]


def test_signed_zeros_in_min_max_runs(gb, gpu):
    """MIN / MAX of +0.0 and -0.0: C's fmin / fmax may return either zero, and the host's and the device's do not promise the same one (tests/operator_model.py
    accepts both).  So here, and only here, the device result is compared with the host route by VALUE (0.0 == -0.0) with every other bit pattern still exact:
    runs of zeros of both signs among larger / smaller values, at a lane's length, a wave tree's and beyond one chunk."""
    _, serial, _ = thresholds(gb)
    rng = np.random.default_rng(24)
    for t in ("FP32", "FP64"):
        for length in (2, serial, serial + 1, 64, 130):
            for op, other in (("MIN", 3.5), ("MAX", -3.5)):
                run = np.where(rng.integers(0, 3, length) == 0, other, np.where(rng.integers(0, 2, length) == 0, 0.0, -0.0)).astype(om.NP[t])
                run[0], run[-1] = 0.0, -0.0
                I, J, X, nr, nc = with_run(t, rng, length, run_values=run)
                typ = getattr(gb, t)
                with route("1"):
                    D = gb.Matrix.from_arrays(I, J, X, nr, nc, typ, dup=getattr(typ, op))
                    assert gb.last_kernel_plan().startswith("build<")
                with route("0"):
                    H = gb.Matrix.from_arrays(I, J, X, nr, nc, typ, dup=getattr(typ, op))
                (drp, dci, dx), (hrp, hci, hx) = D.to_csr(), H.to_csr()
                zero = (hx == 0)
                assert np.array_equal(drp, hrp) and np.array_equal(dci, hci) and np.array_equal(dx == 0, zero) and bits_equal(dx[~zero], hx[~zero]), (t, op, length)
                assert int(zero.sum()) >= 1


def test_leading_and_trailing_empty_rows(gb, gpu):
    rng = np.random.default_rng(20)
    I, J = tuples(rng, 500, 200, 50); I += np.uint64(400)
    _, plan = check_matrix(gb, "FP32", I, J, values("FP32", rng, 500), 1000, 50, "PLUS")       # rows 400..599 of 1000
    assert "rows=heads" in plan
    I5 = np.array([70000, 70000, 70003, 99990, 70001], np.uint64)
    D, plan = check_matrix(gb, "FP32", I5, [1, 0, 2, 3, 1], values("FP32", rng, 5), 100000, 4, "PLUS")      # rows far outnumber entries: bisected
    assert "rows=search" in plan
    rp = D.to_csr()[0]
    assert rp[70000] == 0 and rp[70001] == 2 and rp[70002] == 3 and rp[70004] == 4 and rp[99991] == 5 and rp[-1] == 5 and not rp[:70001].any()


# ---- sorted fast path -------------------------------------------------------------------------------------------------------------
def test_sorted_fast_path(gb, gpu):
    rng = np.random.default_rng(21)
    n, dim = 1500, 300
    flat = np.sort(rng.choice(dim * dim, n, replace=False)).astype(np.uint64)
    X = values("FP64", rng, n)
    _, plan = check_matrix(gb, "FP64", flat // dim, flat % dim, X, dim, dim, None)
    assert "sorted=1" in plan and "fold=none" in plan
    eq = flat.copy(); eq[-1] = eq[-2]
    _, plan = check_matrix(gb, "FP64", eq // dim, eq % dim, X, dim, dim, "PLUS")
    assert "sorted=0" in plan
    for boundary in (64, 256, 512, 1024):                             # increasing inside every wave- and workgroup-sized chunk, one step down across a boundary
        sw = flat.copy(); sw[boundary:] = flat[boundary - 1:-1]; sw[boundary - 1] = flat[-1]
        assert np.all(np.diff(sw[:boundary].astype(np.int64)) > 0) and np.all(np.diff(sw[boundary:].astype(np.int64)) > 0) and sw[boundary] < sw[boundary - 1]
        _, plan = check_matrix(gb, "FP64", sw // dim, sw % dim, X, dim, dim, None)
        assert "sorted=0" in plan, (boundary, plan)
    d, plan, _ = check_vector(gb, "INT16", flat, values("INT16", rng, n), dim * dim, None)
    assert "sorted=1" in plan


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(gb, gpu):
    X = np.arange(1.0, 7.0)
    good_I = np.array([1, 2, 3, 4, 5, 6], np.uint64); J = np.zeros(6, np.uint64)
    oob = good_I.copy(); oob[4] = (1 << 32) + 3
    dupl = good_I.copy(); dupl[5] = 1
    both = oob.copy(); both[5] = 1
    with route("1"):
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
        dJ, dX = dev(J), dev(X)
        ptr = lambda tns: C.c_void_p(tns.data_ptr())
        def mat_at1(c, I, dup):                                       # the same tuples as device arrays (location = 1): read where they are
            dI = dev(I); torch.cuda.synchronize()
            return gb.lib.GrBX_Matrix_build_at(c._h, ptr(dI), ptr(dJ), ptr(dX), C.c_uint64(6), dup, 1)
        def vec_at1(c, I, dup):
            dI = dev(I); torch.cuda.synchronize()
            return gb.lib.GrBX_Vector_build_at(c._h, ptr(dI), ptr(dX), C.c_uint64(6), dup, 1)
        for make, build in ((lambda: gb.Matrix.sparse(gb.FP64, 10, 10), lambda c, I, dup: gb.lib.GrBX_Matrix_build_at(c._h, _p(I), _p(J), _p(X), C.c_uint64(6), dup, 0)),
                            (lambda: gb.Vector.sparse(gb.FP64, 10), lambda c, I, dup: gb.lib.GrBX_Vector_build_at(c._h, _p(I), _p(X), C.c_uint64(6), dup, 0)),
                            (lambda: gb.Matrix.sparse(gb.FP64, 10, 10), mat_at1), (lambda: gb.Vector.sparse(gb.FP64, 10), vec_at1)):
            c = make()
            assert build(c, oob, None) == INDEX_OUT_OF_BOUNDS and c.nvals == 0
            assert build(c, both, None) == INDEX_OUT_OF_BOUNDS and c.nvals == 0, "bounds come before duplicates"
            assert build(c, dupl, None) == INVALID_VALUE and c.nvals == 0
            assert build(c, dupl, C.c_void_p(gb.FP64.PLUS.get_op())) == 0 and c.nvals == 5 and gb.last_kernel_plan().startswith("build<")
            before = sorted(c)
            assert build(c, good_I, None) == OUTPUT_NOT_EMPTY and sorted(c) == before
            c.clear()
            assert build(c, good_I, None) == 0 and c.nvals == 6


# ---- residency and use ------------------------------------------------------------------------------------------------------------
def test_built_containers_feed_products(gb, gpu):
    rng = np.random.default_rng(22)
    n, dim = 5000, 300
    I, J = tuples(rng, n, dim, dim)
    X = rng.integers(1, 5, n).astype(np.float64)
    D, _ = check_matrix(gb, "FP64", I, J, X, dim, dim, "PLUS")
    with route("0"):
        H = gb.Matrix.from_arrays(I, J, X, dim, dim, gb.FP64, dup=gb.FP64.PLUS)
    vi = rng.choice(dim, 120, replace=False); vx = rng.integers(1, 5, 120).astype(np.float64)
    d, _, nv = check_vector(gb, "FP64", vi, vx, dim, "PLUS")
    assert residency(gb, d) == 2 and d.nvals == nv == 120
    # the count is the fold's, recorded with the image (VecFacts::image_replaced(nvals, true)), not counted on demand: GxB_Matrix_diag skips its scan ("full=1")
    # only for a vector whose count is KNOWN and equals its size — with an unknown count the plan would read full=0
    full, _, _ = check_vector(gb, "FP64", np.concatenate([np.arange(dim), vi]), np.concatenate([np.ones(dim), vx]), dim, "PLUS")
    os.environ["GRB_MI355X_DIAG"] = "1"
    try:
        gb.Matrix.from_diag(full)
        assert gb.last_kernel_plan().startswith("diag_matrix<k=0,full=1>"), gb.last_kernel_plan()
    finally:
        os.environ.pop("GRB_MI355X_DIAG", None)
    with route("0"):
        h = gb.Vector.from_arrays(vi.astype(np.uint64), vx, dim, gb.FP64, dup=gb.FP64.PLUS)
    for a, b in ((D.mxv(d), H.mxv(h)), (d.vxm(D), h.vxm(H))):
        ax, ap = a.to_dense_arrays(); bx, bp = b.to_dense_arrays()
        assert np.array_equal(ap, bp) and bits_equal(ax, bx)


def test_from_tensors(gb, gpu):
    torch = pytest.importorskip("torch")
    from pygraphblas_amd import rmat
    src, dst = rmat.edges_torch(12, "cuda")
    V = torch.ones(src.numel(), dtype=torch.float64, device="cuda")
    n = 1 << 12
    with route("1"):
        A = gb.Matrix.from_tensors(src, dst, V, n, n, dup=gb.FP64.PLUS)
        plan = gb.last_kernel_plan()
        v = gb.Vector.from_tensors(src, V, n, gb.FP64, dup=gb.FP64.PLUS)
        vplan = gb.last_kernel_plan()
    assert plan.startswith("build<type=FP64,dup=PLUS") and vplan.startswith("build<") and residency(gb, A) == 2 and residency(gb, v) == 2
    si, di = src.cpu().numpy().astype(np.uint64), dst.cpu().numpy().astype(np.uint64)
    with route("0"):
        H = gb.Matrix.from_arrays(si, di, np.ones(len(si)), n, n, gb.FP64, dup=gb.FP64.PLUS)
        h = gb.Vector.from_arrays(si, np.ones(len(si)), n, gb.FP64, dup=gb.FP64.PLUS)
    assert all(bits_equal(a, b) for a, b in zip(A.to_csr(), H.to_csr()))
    assert all(bits_equal(a, b) for a, b in zip(v.to_dense_arrays(), h.to_dense_arrays()))
    with route("0"):                                                  # device tensors on the host route: downloaded once, same result
        A0 = gb.Matrix.from_tensors(src, dst, V, n, n, dup=gb.FP64.PLUS)
    assert residency(gb, A0) == 1 and all(bits_equal(a, b) for a, b in zip(A0.to_csr(), H.to_csr()))


# ---- the threshold ----------------------------------------------------------------------------------------------------------------
def test_threshold(gb, gpu):
    dev_min = thresholds(gb)[0]
    rng = np.random.default_rng(23)
    with route(None):
        for n, device in ((dev_min - 1, False), (dev_min, True)):
            dim = int(np.sqrt(4 * n)) + 1
            I, J = tuples(rng, n, dim, dim)
            A = gb.Matrix.from_arrays(I, J, values("FP64", rng, n), dim, dim, gb.FP64, dup=gb.FP64.PLUS)
            assert ("build<" in gb.last_kernel_plan()) == device and residency(gb, A) == (2 if device else 1), n
