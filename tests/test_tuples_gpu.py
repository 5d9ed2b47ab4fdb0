"""extractTuples in HBM (grb_tuples.hip; GrBX_Matrix_extractTuples_at / GrBX_Vector_extractTuples_at with location 1; Matrix.to_tensors / Vector.to_tensors): bit for
bit against a numpy model of the layout (I = repeat(arange(nrows), diff(rowptr)), J = colidx, X = values; flatnonzero(present)) and against today's host route
(to_arrays of a dup).  Operands are imported straight into HBM; the plan string and residency 2 before and after are asserted.  Sizes come from
GrBX_tuples_geometry: T = entries per tile, G = grid cap x tile."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAT_PLAN = "tuples<on=matrix,i=1,j=1,x=1> k_tuples_csr"


def geometry(gb):
    out = (C.c_uint64 * 3)()
    assert gb.lib.GrBX_tuples_geometry(out) == 0
    return int(out[0]), int(out[1]), int(out[2])


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def host(t):
    """a tensor as numpy; int64 words as the unsigned words of the C ABI (same bits)"""
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def same_tuples(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), what


def values_of(rng, typ, n):
    """n values of a type with its awkward bit patterns in them: NaNs with payloads, both zeros, infinities, the extremes"""
    dt = np.dtype(typ._np)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if dt.kind == "f":
        u = np.dtype("u%d" % dt.itemsize)
        x = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)      # every bit pattern: NaN payloads, denormals, infinities
        special = np.array([-0.0, 0.0, np.nan, -np.nan, np.inf], dt).view(u)
        x[: min(n, len(special))] = special[: min(n, len(special))]
        if n > 6:
            x[5] = np.array([0x7FC00001 if dt.itemsize == 4 else 0x7FF8000000000123], u)[0]      # a quiet NaN with a payload
            x[6] = np.array([0xFFC12345 if dt.itemsize == 4 else 0xFFF0000000000001], u)[0]      # ... negative, and a signalling one
        return x.view(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def csr_from_lengths(rng, lengths, ncols, sort=True):
    rowptr = np.zeros(len(lengths) + 1, np.int64)
    rowptr[1:] = np.cumsum(lengths)
    col = np.empty(int(rowptr[-1]), np.uint32)
    for r, k in enumerate(lengths):
        if k:
            col[rowptr[r]:rowptr[r + 1]] = np.sort(rng.choice(ncols, int(k), replace=False)) if ncols <= 1 << 22 else np.sort(rng.integers(0, ncols, int(k)))
    return rowptr.astype(np.uint32), col


def model_tuples(nrows, rowptr, col, val):
    return (np.repeat(np.arange(nrows, dtype=np.uint64), np.diff(rowptr.astype(np.int64))), col.astype(np.uint64), val)


def check_matrix(gb, typ, nrows, ncols, rowptr, col, val, what):
    A = gb.Matrix.from_csr(typ, nrows, ncols, rowptr, col, val)
    assert residency(gb, A) == 2, what
    out = A.to_tensors()
    plan = gb.last_kernel_plan()
    assert residency(gb, A) == 2, what                              # expanded where it lives: no host mirror was built
    got = tuple(host(t) for t in out)
    if len(col):
        assert plan == MAT_PLAN, (what, plan)
    assert all(t.is_contiguous() and t.device.type == "cuda" for t in out)
    same_tuples(got, model_tuples(nrows, rowptr, col, val), what + " vs model")
    same_tuples(got, A.dup().to_arrays(), what + " vs host route")
    return A, out


# ---- matrices ----------------------------------------------------------------------------------------------------------------------
def test_matrix_entry_counts_at_the_tile_edges(gb, gpu):
    T, _, cap = geometry(gb)
    rng = np.random.default_rng(1)
    for nvals in (0, 1, T - 1, T, T + 1):
        nrows = 37
        lengths = rng.multinomial(nvals, np.ones(nrows) / nrows)
        rowptr, col = csr_from_lengths(rng, lengths, 5000)
        check_matrix(gb, gb.FP64, nrows, 5000, rowptr, col, values_of(rng, gb.FP64, nvals), f"nvals={nvals}")


def test_matrix_past_one_grid_round(gb, gpu):
    """G + 1 entries: the first workgroup takes a second tile, which holds one entry.  One-byte values keep the case small."""
    T, _, cap = geometry(gb)
    nvals = cap * T + 1
    rng = np.random.default_rng(2)
    nrows, ncols = 3001, 1 << 20
    lengths = rng.multinomial(nvals, rng.dirichlet(np.ones(nrows) * 0.3))
    rowptr = np.zeros(nrows + 1, np.int64); rowptr[1:] = np.cumsum(lengths)
    col = (np.arange(nvals, dtype=np.int64) - np.repeat(rowptr[:-1], lengths)).astype(np.uint32)      # 0, 1, 2, ... inside every row
    assert lengths.max() < ncols
    check_matrix(gb, gb.INT8, nrows, ncols, rowptr.astype(np.uint32), col, values_of(rng, gb.INT8, nvals), "G+1")


def test_matrix_long_row_and_empty_rows(gb, gpu):
    T, _, _ = geometry(gb)
    rng = np.random.default_rng(3)
    gap = 2 * T + 3
    shapes = {
        "one long row between single-entry rows": [1, 1, 3 * T + 1, 1, 1],
        "empty rows in the middle": [5, 1] + [0] * gap + [1, T + 7],
        "empty rows at the start": [0] * gap + [3, 1, 700],
        "empty rows at the end": [T, 1, 2] + [0] * gap,
        "empty rows everywhere": [0] * gap + [1] + [0] * gap + [2 * T] + [0] * gap,
        "one row": [T + 9],
        "one row, one entry": [1],
    }
    for what, lengths in shapes.items():
        ncols = 4 * T
        rowptr, col = csr_from_lengths(rng, lengths, ncols)
        check_matrix(gb, gb.FP32, len(lengths), ncols, rowptr, col, values_of(rng, gb.FP32, len(col)), what)


def test_matrix_columns_at_the_top_of_the_range(gb, gpu):
    """ncols = 0xFFFFFFF0 and columns up to 0xFFFFFFEF: J is the column zero-extended, never sign-extended."""
    ncols = 0xFFFFFFF0
    rng = np.random.default_rng(4)
    lengths = [3, 0, 700, 1]
    rowptr = np.zeros(5, np.uint32); rowptr[1:] = np.cumsum(lengths)
    col = np.concatenate([np.array([0, 0x7FFFFFFF, 0x80000000], np.uint32), np.arange(ncols - 700, ncols, dtype=np.int64).astype(np.uint32), np.array([ncols - 1], np.uint32)])
    _, (I, J, V) = check_matrix(gb, gb.INT32, 4, ncols, rowptr, col, values_of(rng, gb.INT32, len(col)), "top columns")
    assert int(J.max()) == ncols - 1 and int(J.min()) == 0 and int(J[2]) == 0x80000000


@pytest.mark.parametrize("tname", ["BOOL", "INT8", "UINT16", "FP32", "FP64", "INT64"])
def test_matrix_every_value_width(gb, gpu, tname):
    T, _, _ = geometry(gb)
    typ = getattr(gb, tname)
    rng = np.random.default_rng(5)
    nrows = 211
    for nvals in (2 * T + 13, 15, 17):                                # (15 / 17: fewer / one more than the values of a 16-byte word of one-byte values)
        lengths = rng.multinomial(nvals, np.ones(nrows) / nrows)
        rowptr, col = csr_from_lengths(rng, lengths, 3000)
        check_matrix(gb, typ, nrows, 3000, rowptr, col, values_of(rng, typ, nvals), f"{tname} nvals={nvals}")


def raw_extract(gb, A, I, J, X, cap):
    import torch
    torch.cuda.synchronize()                                          # the fills of the output tensors ran on torch's stream, the library has its own
    nn = C.c_uint64(cap)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    info = gb.lib.GrBX_Matrix_extractTuples_at(p(I), p(J), p(X), C.byref(nn), A._h, 1)
    return info, nn.value


def test_matrix_null_streams_capacity_and_alignment(gb, gpu):
    import torch
    T, _, _ = geometry(gb)
    rng = np.random.default_rng(6)
    nrows, nvals = 97, 2 * T + 5
    lengths = rng.multinomial(nvals, np.ones(nrows) / nrows)
    rowptr, col = csr_from_lengths(rng, lengths, 9000)
    for typ, tdt in ((gb.FP64, torch.float64), (gb.UINT8, torch.uint8), (gb.INT16, torch.int16)):
        val = values_of(rng, typ, nvals)
        A = gb.Matrix.from_csr(typ, nrows, 9000, rowptr, col, val)
        want = model_tuples(nrows, rowptr, col, val)
        new = lambda dt, off=0: torch.full((nvals + off,), 77, dtype=dt, device="cuda")[off:]
        # each stream NULL in turn: the others are what they always are, the plan names what was written
        for mask in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0)):
            I, J, X = (new(torch.int64) if mask[0] else None), (new(torch.int64) if mask[1] else None), (new(tdt) if mask[2] else None)
            assert raw_extract(gb, A, I, J, X, nvals) == (0, nvals)
            assert gb.last_kernel_plan() == f"tuples<on=matrix,i={mask[0]},j={mask[1]},x={mask[2]}> k_tuples_csr"
            for t, w in zip((I, J, X), want):
                if t is not None:
                    same_tuples((host(t),), (w,), f"{typ.__name__} mask={mask}")
        # all NULL: nvals alone, no launch
        assert raw_extract(gb, A, None, None, None, 0) == (0, nvals) and gb.last_kernel_plan() == "tuples<on=matrix,i=0,j=0,x=0>"
        # capacity too small: refused, nothing written
        I, J, X = new(torch.int64), new(torch.int64), new(tdt)
        assert raw_extract(gb, A, I, J, X, nvals - 1) == (11, nvals - 1)
        assert bool((I == 77).all()) and bool((J == 77).all()) and bool((X == 77).all())
        # outputs that are 8-byte but not 16-byte aligned (a slice [1:]), every mix of aligned and not
        for offs in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
            I, J, X = new(torch.int64, offs[0]), new(torch.int64, offs[1]), new(tdt, offs[2])
            assert I.data_ptr() % 16 == (8 if offs[0] else 0) and X.data_ptr() % 16 == (X.element_size() if offs[2] else 0)
            assert raw_extract(gb, A, I, J, X, nvals) == (0, nvals)
            same_tuples((host(I), host(J), host(X)), want, f"{typ.__name__} offsets={offs}")
        assert residency(gb, A) == 2


def test_matrix_location_and_null_n_on_the_device(gb, gpu):
    A = gb.Matrix.from_csr(gb.FP64, 2, 2, np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.array([1.0, 2.0]))
    nn = C.c_uint64(2)
    assert gb.lib.GrBX_Matrix_extractTuples_at(None, None, None, C.byref(nn), A._h, 2) == 5
    assert gb.lib.GrBX_Matrix_extractTuples_at(None, None, None, None, A._h, 1) == 4
    v = gb.Vector.from_dense_array(np.ones(3), gb.FP64)
    assert gb.lib.GrBX_Vector_extractTuples_at(None, None, C.byref(nn), v._h, 3) == 5
    assert gb.lib.GrBX_Vector_extractTuples_at(None, None, None, v._h, 1) == 4


def random_hbm_matrix(gb, rng, typ, n, nvals, ncols=None):
    ncols = ncols or n
    lengths = rng.multinomial(nvals, np.ones(n) / n)
    rowptr, col = csr_from_lengths(rng, lengths, ncols)
    dt = np.dtype(typ._np)
    val = (rng.integers(1, 9, nvals)).astype(dt)
    return gb.Matrix.from_csr(typ, n, ncols, rowptr, col, val)


def check_against_host_route(gb, Cm, what):
    """a matrix some operation produced: to_tensors against the host route's order and bytes, rows ascending and columns ascending inside a row"""
    assert residency(gb, Cm) == 2, what
    I, J, V = (host(t) for t in Cm.to_tensors())
    assert gb.last_kernel_plan() == MAT_PLAN and residency(gb, Cm) == 2, what
    same_tuples((I, J, V), Cm.dup().to_arrays(), what)
    key = I.astype(np.float64) * float(Cm.ncols) + J.astype(np.float64)
    assert len(I) > 0 and np.all(np.diff(key) > 0), what


def test_matrices_from_named_producers(gb, gpu):
    rng = np.random.default_rng(7)
    A = random_hbm_matrix(gb, rng, gb.FP64, 600, 9000)
    B = random_hbm_matrix(gb, rng, gb.FP64, 600, 9000)
    check_against_host_route(gb, A.mxm(B, gb.FP64.PLUS_TIMES), "unmasked mxm, default mode")      # the hash SpGEMM: rows leave its tables in slot order and are sorted
    check_against_host_route(gb, A.mxm(B, gb.FP64.PLUS_TIMES, mask=A), "masked mxm")
    L = random_hbm_matrix(gb, rng, gb.INT64, 3000, 60000)
    check_against_host_route(gb, L.mxm(L, gb.INT64.PLUS_PAIR), "unmasked mxm, larger")
    K1 = random_hbm_matrix(gb, rng, gb.INT32, 40, 300, 50)
    K2 = random_hbm_matrix(gb, rng, gb.INT32, 30, 200, 20)
    check_against_host_route(gb, K1.kronecker(K2, gb.INT32.TIMES), "kronecker")


def test_queued_edits_are_flushed_by_the_call(gb, gpu):
    import torch
    rng = np.random.default_rng(8)
    nrows, ncols, nvals = 50, 400, 1500
    lengths = rng.multinomial(nvals, np.ones(nrows) / nrows)
    rowptr, col = csr_from_lengths(rng, lengths, ncols)
    val = rng.random(nvals)
    A = gb.Matrix.from_csr(gb.FP64, nrows, ncols, rowptr, col, val)
    model = {(int(i), int(j)): x for i, j, x in zip(*model_tuples(nrows, rowptr, col, val))}
    free = next((3, j) for j in range(ncols) if (3, j) not in model)
    gone, over = next(iter(model)), list(model)[700]
    A[free[0], free[1]] = 42.5; model[free] = 42.5
    del A[gone[0], gone[1]]; del model[gone]
    A[over[0], over[1]] = -7.25; model[over] = -7.25
    assert residency(gb, A) == 2
    I = torch.empty(nvals + 1, dtype=torch.int64, device="cuda"); J = torch.empty_like(I); X = torch.empty(nvals + 1, dtype=torch.float64, device="cuda")
    info, n = raw_extract(gb, A, I, J, X, nvals + 1)                  # the edits are still queued: this call applies them
    plan = gb.last_kernel_plan()
    assert info == 0 and n == len(model) == nvals
    assert plan.startswith("edit<on=matrix,") and "tuples<on=matrix,i=1,j=1,x=1> k_tuples_csr" in plan, plan
    keys = sorted(model)
    want = (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64), np.array([model[k] for k in keys]))
    same_tuples((host(I[:n]), host(J[:n]), host(X[:n])), want, "after the flush")
    assert residency(gb, A) == 2
    same_tuples(tuple(host(t) for t in A.to_tensors()), A.dup().to_arrays(), "after the flush vs host route")


def test_batch_matrix_held_as_bitmaps(gb, gpu):
    """2 x 65536: the batch form of eWiseAdd leaves its result as a bitmap alone; the call makes the CSR on demand, as the other consumers do."""
    rng = np.random.default_rng(9)
    ncols = 65536
    dense = np.zeros((2, 2, ncols), np.int32)
    ops = []
    for k in range(2):
        lengths = [3000, 41]
        rowptr, col = csr_from_lengths(rng, lengths, ncols)
        val = rng.integers(1, 100, len(col)).astype(np.int32)
        dense[k, 0, col[:3000]] = val[:3000]; dense[k, 1, col[3000:]] = val[3000:]
        ops.append(gb.Matrix.from_csr(gb.INT32, 2, ncols, rowptr, col, val))
    S = ops[0].eadd(ops[1], gb.INT32.PLUS)
    assert residency(gb, S) == 2
    I, J, V = (host(t) for t in S.to_tensors())
    assert "tuples<on=matrix,i=1,j=1,x=1> k_tuples_csr" in gb.last_kernel_plan() and residency(gb, S) == 2
    total = dense[0] + dense[1]
    wi, wj = np.nonzero((dense[0] != 0) | (dense[1] != 0))
    same_tuples((I, J, V), (wi.astype(np.uint64), wj.astype(np.uint64), total[wi, wj]), "bitmap batch matrix vs model")
    same_tuples((I, J, V), S.dup().to_arrays(), "bitmap batch matrix vs host route")


# ---- vectors -----------------------------------------------------------------------------------------------------------------------
def import_vector(gb, typ, val, present):
    """straight into HBM from GPU tensors (device=True): no host mirror; present = None: a full vector"""
    import torch
    tv = torch.from_numpy(val.view(np.dtype("i%d" % val.dtype.itemsize))).cuda() if len(val) else torch.zeros(1, dtype=torch.uint8, device="cuda")      # (the bytes: any dtype of that width)
    tp = torch.from_numpy(present).cuda() if present is not None and len(present) else None
    torch.cuda.synchronize()
    v = gb.Vector.from_dense_array((tv.data_ptr(), len(val)), typ, present=tp.data_ptr() if tp is not None else None, device=True)
    assert residency(gb, v) == 2
    return v


def check_vector(gb, typ, val, present, what, full=False):
    v = import_vector(gb, typ, val, None if full else present)
    out = v.to_tensors()
    plan = gb.last_kernel_plan()
    assert residency(gb, v) == 2, what
    idx = np.flatnonzero(present)
    if len(idx):
        # (to_tensors asks nvals first, which counts a bitmap whose count is unknown: once the facts record says "all present" the count pass is skipped)
        kernels = "k_tuples_iota" if full or len(idx) == len(present) else "k_tuples_count k_tuples_scatter"
        assert plan == "tuples<on=vector,i=1,j=0,x=1> " + kernels, (what, plan)
    got = tuple(host(t) for t in out)
    same_tuples(got, (idx.astype(np.uint64), val[idx]), what + " vs model")
    same_tuples(got, v.dup().to_arrays(), what + " vs host route")
    (only_i,) = v.to_tensors(values=False)
    assert np.array_equal(host(only_i), idx.astype(np.uint64)), what
    if len(idx):
        assert gb.last_kernel_plan().startswith("tuples<on=vector,i=1,j=0,x=0> "), what
    return v


def vector_sizes(gb):
    _, VT, cap = geometry(gb)
    return [0, 1, 63, 64, 65, VT - 1, VT, VT + 1, cap * VT + 1]


@pytest.mark.parametrize("tname", ["FP64", "INT8"])
def test_vector_sizes_and_densities(gb, gpu, tname):
    typ = getattr(gb, tname)
    rng = np.random.default_rng(10)
    for n in vector_sizes(gb):
        val = values_of(rng, typ, n)
        pats = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8), "random": (rng.random(n) < 0.3).astype(np.uint8)}
        if n:
            first = np.zeros(n, np.uint8); first[0] = 1; last = np.zeros(n, np.uint8); last[n - 1] = 1
            pats.update({"first only": first, "last only": last})
        for kind, present in pats.items():
            if n > 100000 and kind not in ("random", "last only"):  # (past one grid round: the second round's positions are what matters)
                continue
            check_vector(gb, typ, val, present, f"{tname} n={n} {kind}")
        check_vector(gb, typ, val, np.ones(n, np.uint8), f"{tname} n={n} full (iota)", full=True)


@pytest.mark.parametrize("tname", ["BOOL", "UINT16", "FP32", "INT64"])
def test_vector_every_value_width(gb, gpu, tname):
    typ = getattr(gb, tname)
    _, VT, _ = geometry(gb)
    rng = np.random.default_rng(11)
    n = 3 * VT + 77
    val = values_of(rng, typ, n)
    check_vector(gb, typ, val, (rng.random(n) < 0.5).astype(np.uint8), tname)
    check_vector(gb, typ, val, np.ones(n, np.uint8), tname + " full", full=True)


def test_vector_presence_bytes_that_are_not_one(gb, gpu):
    _, VT, _ = geometry(gb)
    rng = np.random.default_rng(12)
    n = 2 * VT + 5
    present = rng.choice(np.array([0, 0, 1, 2, 0x80, 0xFF], np.uint8), n)
    check_vector(gb, gb.FP32, values_of(rng, gb.FP32, n), present, "presence bytes 2 / 0x80 / 0xFF")


def test_vector_unaligned_outputs_and_capacity(gb, gpu):
    import torch
    _, VT, _ = geometry(gb)
    rng = np.random.default_rng(13)
    n = 2 * VT + 9
    val = values_of(rng, gb.FP64, n)
    for full in (False, True):
        present = np.ones(n, np.uint8) if full else (rng.random(n) < 0.6).astype(np.uint8)
        v = import_vector(gb, gb.FP64, val, None if full else present)
        idx = np.flatnonzero(present); nv = len(idx)
        for off in (0, 1):
            I = torch.full((nv + off,), 77, dtype=torch.int64, device="cuda")[off:]; X = torch.full((nv + off,), 77.0, dtype=torch.float64, device="cuda")[off:]
            torch.cuda.synchronize()                                  # (the fills ran on torch's stream)
            nn = C.c_uint64(nv - 1)
            assert gb.lib.GrBX_Vector_extractTuples_at(C.c_void_p(I.data_ptr()), C.c_void_p(X.data_ptr()), C.byref(nn), v._h, 1) == 11 and nn.value == nv - 1
            assert bool((I == 77).all()) and bool((X == 77.0).all())
            nn = C.c_uint64(nv)
            assert gb.lib.GrBX_Vector_extractTuples_at(C.c_void_p(I.data_ptr()), C.c_void_p(X.data_ptr()), C.byref(nn), v._h, 1) == 0 and nn.value == nv
            same_tuples((host(I), host(X)), (idx.astype(np.uint64), val[idx]), f"full={full} off={off}")
            nn = C.c_uint64(0)
            assert gb.lib.GrBX_Vector_extractTuples_at(None, None, C.byref(nn), v._h, 1) == 0 and nn.value == nv


def test_pending_deferred_chain_and_queued_vector_edits(gb, gpu):
    _, VT, _ = geometry(gb)
    rng = np.random.default_rng(14)
    n = 2 * VT + 3
    a, b = rng.random(n), rng.random(n)
    pa, pb = (rng.random(n) < 0.5).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
    u, v = import_vector(gb, gb.FP64, a, pa), import_vector(gb, gb.FP64, b, pb)
    w = u.eadd(v, gb.FP64.PLUS)                                       # non-blocking mode: queued, not run
    I, X = (host(t) for t in w.to_tensors())
    assert residency(gb, w) == 2
    idx = np.flatnonzero(pa | pb)
    want = np.where(pa & pb, a + b, np.where(pa, a, b))[idx]
    same_tuples((I, X), (idx.astype(np.uint64), want), "deferred chain")
    same_tuples((I, X), w.dup().to_arrays(), "deferred chain vs host route")
    # queued element edits of an HBM-only vector: the raw call applies them
    import torch
    hole = int(np.flatnonzero(pa == 0)[0]); there = int(np.flatnonzero(pa)[0])
    u[hole] = 9.5
    del u[there]
    pa2 = pa.copy(); pa2[hole] = 1; pa2[there] = 0; a2 = a.copy(); a2[hole] = 9.5
    nv = int(pa2.sum())
    I = torch.empty(nv, dtype=torch.int64, device="cuda"); X = torch.empty(nv, dtype=torch.float64, device="cuda")
    nn = C.c_uint64(nv)
    assert gb.lib.GrBX_Vector_extractTuples_at(C.c_void_p(I.data_ptr()), C.c_void_p(X.data_ptr()), C.byref(nn), u._h, 1) == 0 and nn.value == nv
    plan = gb.last_kernel_plan()
    assert plan.startswith("edit<on=vector,") and "tuples<on=vector,i=1,j=0,x=1> k_tuples_count k_tuples_scatter" in plan, plan
    same_tuples((host(I), host(X)), (np.flatnonzero(pa2).astype(np.uint64), a2[np.flatnonzero(pa2)]), "queued vector edits")
    assert residency(gb, u) == 2


def test_host_resident_containers_are_uploaded(gb, gpu):
    """A container that lives on the host mirror only: uploaded first, so the call is total (and what was built in HBM is the same tuples)."""
    I0 = np.array([0, 0, 2, 5], np.uint64); J0 = np.array([1, 3, 0, 5], np.uint64); X0 = np.array([1.5, -0.0, 3.0, np.inf])
    A = gb.Matrix.from_arrays(I0, J0, X0, 6, 6, gb.FP64)
    assert residency(gb, A) == 1
    same_tuples(tuple(host(t) for t in A.to_tensors()), (I0, J0, X0), "host-resident matrix")
    assert gb.last_kernel_plan() == MAT_PLAN
    v = gb.Vector.from_arrays(I0 + J0 * np.uint64(7), X0, 50, gb.FP64)
    order = np.argsort(I0 + J0 * np.uint64(7))
    same_tuples(tuple(host(t) for t in v.to_tensors()), ((I0 + J0 * np.uint64(7))[order], X0[order]), "host-resident vector")


# ---- round trips and the layout exports --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvals", [700, 30000])
def test_round_trip_through_from_tensors(gb, gpu, nvals):
    rng = np.random.default_rng(15)
    nrows, ncols = 900, 1200
    lengths = rng.multinomial(nvals, rng.dirichlet(np.ones(nrows)))
    lengths = np.minimum(lengths, ncols)
    rowptr, col = csr_from_lengths(rng, lengths, ncols)
    val = values_of(rng, gb.FP32, len(col))
    A = gb.Matrix.from_csr(gb.FP32, nrows, ncols, rowptr, col, val)
    B = gb.Matrix.from_tensors(*A.to_tensors(), nrows, ncols)
    assert B.type is gb.FP32
    same_tuples(B.to_csr(), A.to_csr(), "matrix round trip")
    same_tuples(B.to_csr(), (rowptr, col, val), "matrix round trip vs the import")
    rp, ci, x = A.to_csr_tensors()
    assert rp.device.type == "cuda" and str(rp.dtype) == "torch.int32" and str(ci.dtype) == "torch.int32"
    same_tuples((rp.cpu().numpy(), ci.cpu().numpy(), x.cpu().numpy()), (rowptr, col, val), "to_csr_tensors")
    n = 5 * nvals
    present = (rng.random(n) < 0.2).astype(np.uint8)
    vv = values_of(rng, gb.INT16, n)
    v = import_vector(gb, gb.INT16, vv, present)
    u = gb.Vector.from_tensors(*v.to_tensors(), n)
    assert u.type is gb.INT16
    ux, up = u.to_dense_arrays(); vx, vp = v.to_dense_arrays()
    assert np.array_equal(up != 0, vp != 0) and np.array_equal(ux[up != 0], vx[vp != 0]) and np.array_equal(up != 0, present != 0)
    dx, dp = v.to_dense_tensors()
    assert dx.device.type == "cuda" and str(dp.dtype) == "torch.uint8" and str(dx.dtype) == "torch.int16"
    assert np.array_equal(dp.cpu().numpy(), vp) and np.array_equal(dx.cpu().numpy()[present != 0], vv[present != 0])
