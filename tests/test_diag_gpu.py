"""Diagonals on the device: grb_diag.hip behind GxB_Matrix_diag (Matrix.from_diag, Matrix.identity) and GxB_Vector_diag (Matrix.vector_diag), and Matrix.diag.

Both operations copy and cast values and sum nothing, so every comparison is exact equality.  Two references, neither the code under test:
  * a numpy restatement written here: entry r of v lands at (r, r + k) for k >= 0 and at (r + |k|, r) for k < 0; diagonal position r of A is its entry
    (r, r + k) or (r + |k|, r); values take C casts (numpy `astype`, BOOL as x != 0) and are kept inside the target type's range;
  * the host route of the same call (GRB_MI355X_DIAG=0): the code every earlier version ran.
A vector view with an odd byte offset cannot be made through the public surface (every import copies into a fresh allocation), so that operand state has
no case here; the kernels' entry-by-entry path is still taken by the last partial group of every size that is no multiple of four.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [("FP64", "FP64"), ("FP32", "INT32"), ("INT64", "FP32"), ("BOOL", "UINT8"), ("INT8", "INT64")]      # (operand type, output type)
SIZES = [0, 1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]          # the scan's and the four-per-lane pack's boundaries
KS = [0, 1, -1, 5, -5]
CONTENTS = ["empty", "first", "last", "every second", "all"]
SHAPES = [(1, 1), (7, 5), (5, 7), (64, 64), (65, 300), (300, 65), (1025, 1025)]
DIMENSION_MISMATCH, NULL_POINTER = 8, 4


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


def hook(value):
    return env(GRB_MI355X_DIAG=value)


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def values(rng, gb, name, n):
    """Values of the operand type that stay inside the range of the type they are cast to (PAIRS), fractions and negative numbers included."""
    dt = getattr(gb, name)._np
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    if name == "INT8":
        return rng.integers(-128, 128, n).astype(dt)
    if name == "INT64":
        return rng.integers(-(1 << 40), 1 << 40, n).astype(dt)        # (FP32 rounds them: the same round-to-nearest-even in numpy and on the device)
    return (rng.standard_normal(n) * 1000.0).astype(dt)               # FP32 -> INT32 truncates toward zero, |x| far below 2^31


def cast(x, gb, name):
    dt = getattr(gb, name)._np
    x = np.asarray(x)
    return (x != 0) if name == "BOOL" else x.astype(dt)


def content(kind, n):
    if kind == "empty" or n == 0:
        return np.zeros(0, np.uint64)
    if kind == "first":
        return np.array([0], np.uint64)
    if kind == "last":
        return np.array([n - 1], np.uint64)
    return np.arange(0, n, 2 if kind == "every second" else 1, dtype=np.uint64)


def make_vector(gb, state, name, n, idx, x):
    T = getattr(gb, name)
    if state == "host":
        return gb.Vector.from_arrays(idx, x, n, T)
    dense, present = np.zeros(n, T._np), np.zeros(n, np.uint8)          # "hbm": imported straight into HBM, no host mirror
    dense[idx.astype(np.int64)] = x
    present[idx.astype(np.int64)] = 1
    v = gb.Vector.from_dense_array(dense, T, present=present)
    assert residency(gb, v) == 2
    return v


def matrix_diag(gb, v, k, cname, C_out=None):
    n = v.size + abs(k)
    out = gb.Matrix.sparse(getattr(gb, cname), n, n) if C_out is None else C_out
    info = gb.lib.GxB_Matrix_diag(out._h, v._h, C.c_int64(k), None)
    assert info == 0, info
    return out


def vector_diag(gb, A, k, vname, v_out=None):
    m, n = A.nrows, A.ncols
    length = min(m, n - k) if 0 <= k < n else (min(m + k, n) if -m < k < 0 else 0)
    out = gb.Vector.sparse(getattr(gb, vname), length) if v_out is None else v_out
    info = gb.lib.GxB_Vector_diag(out._h, A._h, C.c_int64(k), None)
    assert info == 0, info
    return out


def model_matrix_diag(gb, idx, x, k, cname):
    return idx + np.uint64(max(-k, 0)), idx + np.uint64(max(k, 0)), cast(x, gb, cname)


def model_vector_diag(gb, I, J, X, k, vname):
    on = (J.astype(np.int64) - I.astype(np.int64)) == k
    return np.minimum(I[on], J[on]), cast(X[on], gb, vname)


def clear_plan(gb):
    """The host route leaves the plan empty."""
    with hook(0):
        gb.Matrix.from_diag(gb.Vector.sparse(gb.BOOL, 1))
    assert gb.last_kernel_plan() == ""


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and g.dtype == e.dtype and np.array_equal(g, e), f"{what}: got {g[:12]} expected {e[:12]} (lengths {g.shape} / {e.shape})"


# ---- from_diag ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["host", "hbm"])
@pytest.mark.parametrize("vname,cname", PAIRS)
def test_from_diag_matches_the_model_and_the_host_route(gb, gpu, vname, cname, state):
    """Every size, diagonal and content: the device route (forced for the small host-resident operands, chosen by residency for the HBM-only ones)
    gives the model's tuples and the host route's."""
    rng = np.random.default_rng(11)
    for n in SIZES:
        for kind in CONTENTS:
            idx = content(kind, n)
            x = values(rng, gb, vname, len(idx))
            for k in KS:
                what = f"{vname}->{cname} n={n} k={k} {kind} {state}"
                with hook(1 if state == "host" else None):
                    v = make_vector(gb, state, vname, n, idx, x)
                    Cm = matrix_diag(gb, v, k, cname)
                    plan = gb.last_kernel_plan()
                assert plan.startswith(f"diag_matrix<k={k},full=") and plan.endswith("> k_diag_fill"), (what, plan)
                if len(idx) < n:
                    assert ",full=0>" in plan, (what, plan)
                assert residency(gb, Cm) == 2, what
                if state == "hbm":
                    assert residency(gb, v) == 2, what                  # not downloaded
                assert Cm.shape == (n + abs(k), n + abs(k)) and Cm.type is getattr(gb, cname)
                got = Cm.to_arrays()
                same(got, model_matrix_diag(gb, idx, x, k, cname), what)
                with hook(0):
                    Ch = matrix_diag(gb, gb.Vector.from_arrays(idx, x, n, getattr(gb, vname)), k, cname)
                    assert "diag_" not in gb.last_kernel_plan(), what
                same(got, Ch.to_arrays(), what + " (host route)")


@pytest.mark.parametrize("vname,cname", PAIRS)
def test_from_diag_of_a_lazily_filled_dense_vector(gb, gpu, vname, cname):
    """`Vector.dense` in non-blocking mode is a note on the vector until something reads it: the route completes it and takes the all-present path (no scan)."""
    fill = {"FP64": 2.5, "FP32": -7.75, "INT64": (1 << 40) + 1, "BOOL": True, "INT8": -128}[vname]
    for n in SIZES:
        for k in KS:
            with hook(None):
                v = gb.Vector.dense(getattr(gb, vname), n, fill)
                Cm = matrix_diag(gb, v, k, cname)
                plan = gb.last_kernel_plan()
            if n:                                                      # (an empty vector has nothing to defer: host-resident, no entries, host route)
                assert plan == f"diag_matrix<k={k},full=1> k_diag_fill", plan
                assert residency(gb, v) == 2 and residency(gb, Cm) == 2
            idx = np.arange(n, dtype=np.uint64)
            same(Cm.to_arrays(), model_matrix_diag(gb, idx, np.full(n, fill, getattr(gb, vname)._np), k, cname), f"{vname}->{cname} n={n} k={k}")


@pytest.mark.parametrize("route", [0, 1])
def test_from_diag_replaces_what_the_output_held(gb, gpu, route):
    """C's earlier entries and its pending setElement edits are gone: C becomes exactly the diagonal matrix, on both routes."""
    rng = np.random.default_rng(5)
    for n, k in [(1, 0), (65, 1), (257, -5)]:
        dim = n + abs(k)
        idx = content("every second", n)
        x = values(rng, gb, "FP32", len(idx))
        for c_state in ("host", "hbm"):
            flat = np.sort(rng.choice(dim * dim, size=min(dim * dim, 3 * dim), replace=False))
            Cm = gb.Matrix.from_arrays((flat // dim).astype(np.uint64), (flat % dim).astype(np.uint64), np.ones(len(flat), np.int32), dim, dim, gb.INT32)
            if c_state == "hbm":
                Cm = Cm.apply(gb.INT32.AINV)
            Cm[dim - 1, 0] = 99                                       # a pending edit
            with hook(route):
                matrix_diag(gb, gb.Vector.from_arrays(idx, x, n, gb.FP32), k, "INT32", C_out=Cm)
                assert ("diag_matrix<" in gb.last_kernel_plan()) == bool(route)
            same(Cm.to_arrays(), model_matrix_diag(gb, idx, x, k, "INT32"), f"n={n} k={k} C {c_state} route {route}")


# ---- vector_diag -------------------------------------------------------------------------------------------------------------
def structured_matrix(rng, nrows, ncols, k):
    """Rows built around diagonal k, cycling through: no entries; only the diagonal entry; the diagonal entry first / last / in the middle of nine (the
    bisected length); the diagonal entry absent between its two neighbours; 64 and 65 entries with and without it; up to 8 random entries (the scanned length)."""
    I, J = [], []
    for i in range(nrows):
        j = i + k
        inside = 0 <= j < ncols
        kind = i % 9
        cols = set()
        if kind == 1 and inside:
            cols = {j}
        elif kind == 2 and inside:
            cols = set(range(j, min(ncols, j + 4)))
        elif kind == 3 and inside:
            cols = set(range(max(0, j - 3), j + 1))
        elif kind == 4 and inside:
            cols = set(range(max(0, j - 4), min(ncols, j + 5)))
        elif kind == 5:
            cols = {c for c in (j - 1, j + 1) if 0 <= c < ncols}
        elif kind in (6, 7):
            cols = set(rng.choice(ncols, size=min(ncols, 64 + (kind - 6)), replace=False).tolist())
            if inside and i % 2:
                cols.discard(j)
            elif inside:
                cols.add(j)
        elif kind == 8:
            cols = set(rng.choice(ncols, size=min(ncols, int(rng.integers(1, 9))), replace=False).tolist())
        for c in sorted(cols):
            I.append(i); J.append(c)
    return np.array(I, np.uint64), np.array(J, np.uint64)


def make_matrix(gb, state, name, nrows, ncols, I, J, X):
    T = getattr(gb, name)
    if state == "host":
        return gb.Matrix.from_arrays(I, J, X, nrows, ncols, T)
    rowptr = np.zeros(nrows + 1, np.uint32)
    np.add.at(rowptr, I.astype(np.int64) + 1, 1)
    A = gb.Matrix.from_csr(T, nrows, ncols, np.cumsum(rowptr, dtype=np.uint32), J.astype(np.uint32), X)      # imported straight into HBM
    assert residency(gb, A) == 2
    return A


def diagonals_of(nrows, ncols):
    return sorted({0, 1, -1, 4, -4, ncols - 1, -(nrows - 1), ncols, -nrows})      # ... the last diagonal on each side and the one beyond it (length 0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("aname,vname", PAIRS)
def test_vector_diag_matches_the_model_and_the_host_route(gb, gpu, aname, vname, shape):
    nrows, ncols = shape
    rng = np.random.default_rng(23)
    for k in diagonals_of(nrows, ncols):
        I, J = structured_matrix(rng, nrows, ncols, k)
        X = values(rng, gb, aname, len(I))
        exp = model_vector_diag(gb, I, J, X, k, vname)
        with hook(0):
            vh = vector_diag(gb, gb.Matrix.from_arrays(I, J, X, nrows, ncols, getattr(gb, aname)), k, vname)
            assert "diag_" not in gb.last_kernel_plan()
        same(vh.to_arrays(), exp, f"{aname}->{vname} {shape} k={k} host route")
        for state in ("host", "hbm"):
            what = f"{aname}->{vname} {shape} k={k} {state}"
            with hook(1 if state == "host" else None):
                A = make_matrix(gb, state, aname, nrows, ncols, I, J, X)
                v = vector_diag(gb, A, k, vname)
                assert gb.last_kernel_plan() == f"diag_vector<k={k}> k_diag_read", (what, gb.last_kernel_plan())
            assert residency(gb, v) == 2, what
            if state == "hbm":
                assert residency(gb, A) == 2, what                      # not downloaded
            assert v.type is getattr(gb, vname)
            same(v.to_arrays(), exp, what)


def test_vector_diag_hub_rows(gb, gpu):
    """Rows of 5 000 entries (13 probes of the bisection), with and without the diagonal entry, beside short ones."""
    rng = np.random.default_rng(31)
    nrows, ncols = 24, 6000
    for k in (0, -1, 4, 2500):
        I, J = [], []
        for i in range(nrows):
            j = i + k
            if i % 4 == 3:
                cols = {c for c in (j - 1, j, j + 1) if 0 <= c < ncols}
            else:
                cols = set(rng.choice(ncols, size=5000, replace=False).tolist())
                if 0 <= j < ncols:
                    cols.add(j) if i % 2 else cols.discard(j)
            for c in sorted(cols):
                I.append(i); J.append(c)
        I, J = np.array(I, np.uint64), np.array(J, np.uint64)
        X = values(rng, gb, "FP64", len(I))
        with hook(None):
            v = vector_diag(gb, make_matrix(gb, "hbm", "FP64", nrows, ncols, I, J, X), k, "FP64")
            assert gb.last_kernel_plan().startswith("diag_vector<")
        same(v.to_arrays(), model_vector_diag(gb, I, J, X, k, "FP64"), f"hub rows k={k}")


@pytest.mark.parametrize("route", [0, 1])
def test_vector_diag_replaces_what_the_output_held(gb, gpu, route):
    rng = np.random.default_rng(7)
    nrows, ncols, k = 65, 300, 4
    I, J = structured_matrix(rng, nrows, ncols, k)
    X = values(rng, gb, "INT8", len(I))
    for v_state in ("host", "hbm"):
        old = np.arange(0, 65, 3, dtype=np.uint64)
        v = make_vector(gb, v_state, "INT64", 65, old, np.full(len(old), -1, np.int64))
        with hook(route):
            vector_diag(gb, gb.Matrix.from_arrays(I, J, X, nrows, ncols, gb.INT8), k, "INT64", v_out=v)
            assert ("diag_vector<" in gb.last_kernel_plan()) == bool(route)
        same(v.to_arrays(), model_vector_diag(gb, I, J, X, k, "INT64"), f"v {v_state} route {route}")


def test_vector_diag_of_a_bitmap_only_batch_matrix_takes_the_host_route(gb, gpu):
    """A 64 x 65536 batch matrix that lives as a bitmap alone has no CSR to read: the host route serves it, hook or not."""
    for value, k in ((None, 0), (1, -3)):
        half = gb.Matrix.dense(gb.FP32, 64, 65536, 1.25)
        A = half.eadd(half, gb.FP32.PLUS)                             # the batch form of eWiseAdd leaves its result as a bitmap alone (a fresh one per call: the host route
                                                                      # leaves a host mirror behind, and with it a matrix like any other)
        with hook(value):
            v = vector_diag(gb, A, k, "FP32")
            assert "diag_" not in gb.last_kernel_plan(), gb.last_kernel_plan()
        n = 64 - max(-k, 0)
        same(v.to_arrays(), (np.arange(n, dtype=np.uint64), np.full(n, 2.5, np.float32)), f"batch matrix k={k}")


# ---- routing -----------------------------------------------------------------------------------------------------------------
def test_routing_by_size_and_hook(gb, gpu):
    """100 entries, host-resident, hook unset: the host route (empty plan).  The hook set to 1: the device route and the same tuples.  From the threshold on
    the device route is taken without the hook."""
    rng = np.random.default_rng(3)
    idx = np.arange(100, dtype=np.uint64)
    x = values(rng, gb, "FP64", 100)
    mk = lambda: gb.Vector.from_arrays(idx, x, 100, gb.FP64)
    with hook(None):
        Dh = gb.Matrix.from_diag(mk(), 2)
        assert gb.last_kernel_plan() == ""
        dh = Dh.vector_diag(2)
        assert gb.last_kernel_plan() == ""
        assert residency(gb, Dh) == 1 and residency(gb, dh) == 1
    with hook(1):
        Dd = gb.Matrix.from_diag(mk(), 2)
        assert gb.last_kernel_plan().startswith("diag_matrix<k=2,")
        dd = gb.Matrix.from_arrays(*Dh.to_arrays(), 102, 102, gb.FP64).vector_diag(2)
        assert gb.last_kernel_plan().startswith("diag_vector<k=2>")
    same(Dd.to_arrays(), Dh.to_arrays(), "from_diag, both routes")
    same(dd.to_arrays(), dh.to_arrays(), "vector_diag, both routes")
    same(dd.to_arrays(), (idx, x), "round trip")
    mat_min, vec_min = C.c_uint64(0), C.c_uint64(0)
    assert gb.lib.GrBX_diag_thresholds(C.byref(mat_min), C.byref(vec_min)) == 0
    with hook(None):
        n = mat_min.value
        big = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.ones(n, np.float32), n, gb.FP32)
        gb.Matrix.from_diag(big)
        assert gb.last_kernel_plan().startswith("diag_matrix<k=0,"), gb.last_kernel_plan()
        n = vec_min.value
        A = gb.Matrix.from_arrays(np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64), np.ones(n, np.float32), n, n, gb.FP32)
        d = A.vector_diag()
        assert gb.last_kernel_plan().startswith("diag_vector<k=0>"), gb.last_kernel_plan()
        assert d.nvals == n


# ---- round trips and the Python surface ----------------------------------------------------------------------------------------
def test_from_diag_then_vector_diag_is_the_vector(gb, gpu):
    rng = np.random.default_rng(13)
    for n in SIZES:
        idx = np.sort(rng.choice(n, size=n // 2 + (n % 2), replace=False)).astype(np.uint64) if n else np.zeros(0, np.uint64)
        x = values(rng, gb, "INT64", len(idx))
        for k in KS:
            with hook(None):
                v = make_vector(gb, "hbm", "INT64", n, idx, x)
                back = gb.Matrix.from_diag(v, k).vector_diag(k)
                assert gb.last_kernel_plan().startswith("diag_vector<")
            assert back.size == n
            same(back.to_arrays(), (idx, x), f"n={n} k={k}")


def test_identity_on_both_sides_of_the_threshold(gb, gpu):
    mat_min, vec_min = C.c_uint64(0), C.c_uint64(0)
    assert gb.lib.GrBX_diag_thresholds(C.byref(mat_min), C.byref(vec_min)) == 0
    for n in (mat_min.value - 1, mat_min.value):
        idx = np.arange(n, dtype=np.uint64)
        clear_plan(gb)
        with hook(None):
            Id = gb.Matrix.identity(gb.FP32, n)
            plan = gb.last_kernel_plan()
        assert (plan == "diag_matrix<k=0,full=1> k_diag_fill") == (n >= mat_min.value), (n, plan)
        assert Id.type is gb.FP32 and Id.shape == (n, n)
        same(Id.to_arrays(), gb.Matrix.from_arrays(idx, idx, np.ones(n, np.float32), n, n, gb.FP32).to_arrays(), f"identity {n}")
    Id = gb.Matrix.identity(gb.INT8, mat_min.value, one=-3)
    same(Id.to_arrays(), (np.arange(mat_min.value, dtype=np.uint64),) * 2 + (np.full(mat_min.value, -3, np.int8),), "identity with a value")


def test_matrix_diag_is_select_diag(gb, gpu):
    rng = np.random.default_rng(17)
    flat = np.sort(rng.choice(40 * 50, size=700, replace=False))
    A = gb.Matrix.from_arrays((flat // 50).astype(np.uint64), (flat % 50).astype(np.uint64), values(rng, gb, "FP64", 700), 40, 50, gb.FP64)
    for thunk in (None, 2, -3):
        D = A.diag() if thunk is None else A.diag(thunk)
        same(D.to_arrays(), A.select("DIAG", thunk).to_arrays(), f"diag({thunk})")
        I, J, X = A.to_arrays()
        on = (J.astype(np.int64) - I.astype(np.int64)) == (thunk or 0)
        same(D.to_arrays(), (I[on], J[on], X[on]), f"diag({thunk}) against the tuples")


# ---- errors: the same on both routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
def test_errors_on_both_routes(gb, gpu, route):
    v = gb.Vector.from_lists([0, 2], [3, 4], 3, gb.INT64)
    A = gb.Matrix.from_lists([0, 1, 2], [0, 1, 2], [1, 2, 3], 3, 4, gb.INT64)
    mdiag = lambda Cm, vec, k: gb.lib.GxB_Matrix_diag(Cm._h if Cm is not None else None, vec._h if vec is not None else None, C.c_int64(k), None)
    vdiag = lambda vec, Am, k: gb.lib.GxB_Vector_diag(vec._h if vec is not None else None, Am._h if Am is not None else None, C.c_int64(k), None)
    with hook(route):
        for dim in (3, 5):                                            # size(v) + |k| = 4
            assert mdiag(gb.Matrix.sparse(gb.INT64, dim, dim), v, -1) == DIMENSION_MISMATCH
        assert mdiag(gb.Matrix.sparse(gb.INT64, 4, 5), v, 1) == DIMENSION_MISMATCH
        for length, k in ((2, 0), (4, 0), (3, 2), (1, 4), (3, -3)):   # the diagonals have 3, 3, 2, 0 and 0 positions
            assert vdiag(gb.Vector.sparse(gb.INT64, length), A, k) == DIMENSION_MISMATCH
        assert mdiag(None, v, 0) == NULL_POINTER
        assert mdiag(gb.Matrix.sparse(gb.INT64, 3, 3), None, 0) == NULL_POINTER
        assert vdiag(None, A, 0) == NULL_POINTER
        assert vdiag(gb.Vector.sparse(gb.INT64, 3), None, 0) == NULL_POINTER
        for k in (-(1 << 63), (1 << 63) - 1):                         # far outside: a length of 0, a dimension no matrix has
            assert vdiag(gb.Vector.sparse(gb.INT64, 0), A, k) == 0
            assert mdiag(gb.Matrix.sparse(gb.INT64, 3, 3), v, k) == DIMENSION_MISMATCH
