"""Index-list extract on the device (grb_extract.hip behind GrB_Matrix_extract / GrB_Col_extract / GrB_Vector_extract).

Three references, none of them the code under test:
  * T = op(A)(I, J) from scipy fancy indexing / numpy (repeats in a list give exactly GraphBLAS's answer);
  * `C<M, replace> = accum(C, T)` from a dict model written here from the C API rule (Z = accum ? C u T with accum on the
    intersection : T; then the masked write of Z into C), casts by numpy `astype` on values small enough to be exact in every type;
  * the forced host route (GRB_MI355X_EXTRACT=0): the map-based code every earlier version ran.
Values are moved as bytes and an accumulator is applied once per entry, so every comparison is bit-exact, floating point included.
"""
import contextlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
KINDS = ["all", "range", "stride", "backwards", "increasing", "shuffled", "repeats", "empty", "single"]
LIST_KINDS = ("increasing", "shuffled", "repeats", "single")
MASKS = [None, "valued", "structural", "complemented", "structural+complemented"]
ACCUMS = [None, "PLUS", "SECOND", "MIN"]


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


def typ(gb, name):
    return getattr(gb, name)


def npdt(gb, name):
    return np.dtype(typ(gb, name)._np)


def values(rng, gb, name, n):
    """0 .. 5 (BOOL: 0 / 1), explicit zeros included: exact in all eleven types, sums of two stay below 2^7."""
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    return rng.integers(0, 6, n).astype(npdt(gb, name))


def pick(kind, d, rng):
    """(argument for the Python surface, the positions it names) for one index kind over a dimension of d >= 1."""
    if kind == "all":
        return None, list(range(d))
    if kind in ("range", "stride", "backwards"):
        a, b = sorted(int(x) for x in rng.integers(0, d, 2))
        s = int(rng.integers(1, 5))
        if kind == "range":
            return slice(a, b), list(range(a, b + 1))                  # the reference's slices include their stop
        if kind == "stride":
            return slice(a, b, s), list(range(a, b + 1, s))
        return slice(b, a, -s), list(range(b, a - 1, -s))
    if kind == "increasing":
        k = int(rng.integers(1, d + 1))
        lst = np.sort(rng.choice(d, size=k, replace=False))
        return (lst.astype(np.int32) if k % 2 else [int(x) for x in lst]), [int(x) for x in lst]      # an ndarray of another dtype, or a list
    if kind == "shuffled":
        k = int(rng.integers(1, d + 1))
        lst = [int(x) for x in rng.permutation(d)[:k]]
        return lst, lst
    if kind == "repeats":
        k = int(rng.integers(2, d + 8))
        lst = [int(x) for x in rng.integers(0, d, k)]
        lst[-1] = lst[0]
        return lst, lst
    if kind == "empty":
        return [], []
    i = int(rng.integers(0, d))
    return [i], [i]


def random_tuples(rng, gb, name, nrows, ncols, density):
    total = nrows * ncols
    nnz = min(total, int(round(total * density)))
    flat = np.sort(rng.choice(total, size=nnz, replace=False)) if total else np.zeros(0, np.int64)
    I, J = (np.divmod(flat, ncols) if total else (flat, flat))
    return I.astype(np.uint64), J.astype(np.uint64), values(rng, gb, name, nnz)


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_T(I, J, X, nrows, ncols, t0, rows, cols):
    """op(A)(rows, cols) as {(a, b): value}: scipy carries 1-based positions into X, so explicit zeros survive."""
    S = sp.csr_matrix((np.arange(1, len(X) + 1, dtype=np.int64), (I.astype(np.int64), J.astype(np.int64))), shape=(nrows, ncols))
    if t0:
        S = S.T.tocsr()
    sub = S[np.asarray(rows, np.int64)][:, np.asarray(cols, np.int64)].tocoo()
    return {(int(a), int(b)): X[int(p) - 1] for a, b, p in zip(sub.row, sub.col, sub.data)}


def accum_op(name, a, b):
    if name == "SECOND":
        return b
    if a.dtype == np.bool_:
        return (a | b) if name == "PLUS" else (a & b)
    return (a + b).astype(a.dtype) if name == "PLUS" else min(a, b)


def model_write_back(C, cdt, T, M, mask_kind, accum, replace):
    """C<M, replace> = accum(C, T) on dicts (C API 1.3, the mask / accumulate / replace rule)."""
    Tc = {p: np.asarray(v).astype(cdt)[()] for p, v in T.items()}
    if accum:
        Z = dict(C)
        for p, t in Tc.items():
            Z[p] = accum_op(accum, Z[p], t) if p in Z else t
    else:
        Z = Tc
    comp = mask_kind is not None and "complemented" in mask_kind
    structural = mask_kind is not None and "structural" in mask_kind

    def allows(p):
        if M is None:
            return not comp
        return ((p in M) and (structural or bool(M[p]))) != comp
    out = {p: v for p, v in C.items() if not allows(p) and not replace}
    out.update({p: v for p, v in Z.items() if allows(p)})
    return out


def as_sorted(d, cdt, vector=False):
    keys = sorted(d)
    X = np.array([d[k] for k in keys], dtype=cdt) if keys else np.zeros(0, cdt)
    if vector:
        return np.array([k[0] for k in keys], np.uint64), X
    return np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64), X


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and np.array_equal(g, e), f"{what}: got {g[:12]} expected {e[:12]} (lengths {g.shape} / {e.shape})"


def descriptor(gb, mask_kind, replace, t0):
    d = None
    parts = []
    if replace:
        parts.append(gb.descriptor.R)
    if mask_kind and "structural" in mask_kind:
        parts.append(gb.descriptor.S)
    if mask_kind and "complemented" in mask_kind:
        parts.append(gb.descriptor.C)
    if t0:
        parts.append(gb.descriptor.T0)
    for p in parts:
        d = p if d is None else (d & p)
    return d


def make_case(i, rng):
    """The i-th configuration: index kinds, types and options cycle so that every value of each is met many times."""
    c = {"atype": TYPES[i % 11], "rk": KINDS[i % 9], "ck": KINDS[(i // 9) % 9], "mask": MASKS[(i // 2) % 5], "accum": ACCUMS[(i // 3) % 4],
         "replace": (i // 5) % 2 == 1, "t0": (i // 7) % 2 == 1, "prefill": (i // 4) % 3 != 0}
    c["ctype"] = c["atype"] if i % 3 else TYPES[(i * 7 + 3) % 11]
    c["mtype"] = ["BOOL", "INT8", "FP32"][i % 3]
    big = i % 16 == 0
    c["nrows"], c["ncols"] = (int(rng.integers(200, 301)), int(rng.integers(100, 201))) if big else (int(rng.integers(1, 40)), int(rng.integers(1, 30)))
    c["density"] = 0.05 if big else float(rng.choice([0.1, 0.4, 1.0]))
    return c


# ---- 1. which route ---------------------------------------------------------------------------------------------------------
def test_route_and_plan(gb, gpu):
    rng = np.random.default_rng(1)
    I, J, X = random_tuples(rng, gb, "INT32", 50, 40, 0.2)
    A = gb.Matrix.from_arrays(I, J, X, 50, 40, gb.INT32)
    u = gb.Vector.from_arrays(np.arange(0, 40, 2, dtype=np.uint64), np.arange(20, dtype=np.int32), 40, gb.INT32)
    ones = gb.Vector.from_arrays(np.arange(40, dtype=np.uint64), np.ones(40, np.int32), 40, gb.INT32)
    calls = [("extract_matrix", lambda: A.extract_matrix([3, 1, 2], slice(0, 9))), ("extract_col", lambda: A.extract_col(2)), ("extract_col", lambda: A.extract_row(2)),
             ("extract_vector", lambda: u.extract([5, 4, 4]))]
    for name, call in calls:
        with env(GRB_MI355X_EXTRACT=1):
            A.mxv(ones, semiring=gb.INT32.PLUS_TIMES)              # some other plan in between
            call()
            assert gb.last_kernel_plan().startswith(name), (name, gb.last_kernel_plan())
        with env(GRB_MI355X_EXTRACT=0):
            A.mxv(ones, semiring=gb.INT32.PLUS_TIMES)
            call()
            assert not gb.last_kernel_plan().startswith("extract_"), (name, gb.last_kernel_plan())
    with env(GRB_MI355X_EXTRACT=None):                            # a small host-resident matrix keeps the host route
        A.mxv(ones, semiring=gb.INT32.PLUS_TIMES)
        A.extract_matrix([3, 1, 2], slice(0, 9))
        assert not gb.last_kernel_plan().startswith("extract_")
    with env(GRB_MI355X_EXTRACT=1):                               # the plan names the column shape, the row sort and the transpose
        A.extract_matrix(None, None)
        assert "cols=all" in gb.last_kernel_plan() and "rowsort=0" in gb.last_kernel_plan()
        A.extract_matrix(None, slice(3, 20, 2))
        assert "cols=range" in gb.last_kernel_plan()
        A.extract_matrix(None, [1, 5, 9])
        assert "cols=table,rowsort=0,transpose=0" in gb.last_kernel_plan()
        A.extract_matrix(None, [9, 5, 5])
        assert "cols=table,rowsort=1" in gb.last_kernel_plan()
        A.extract_matrix([1, 2], [9, 5, 5], desc=gb.descriptor.T0)
        assert "transpose=1" in gb.last_kernel_plan()


def test_route_by_size_and_residency(gb, gpu):
    """Unset variable: an R-MAT-18 matrix (3.6e6 entries, host mirror valid, on the device after an mxv) and a device-only matrix take the device route."""
    from pygraphblas_amd import rmat
    scale = 18
    n = 1 << scale
    rp, col = rmat.csr_numpy(scale, seed=42)
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    A = gb.Matrix.from_arrays(rows, col.astype(np.uint64), np.ones(len(col), np.float32), n, n, gb.FP32)
    x = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.ones(n, np.float32), n, gb.FP32)
    with env(GRB_MI355X_EXTRACT=None):
        A.mxv(x, semiring=gb.FP32.PLUS_TIMES)
        sub = A.extract_matrix(slice(0, n // 2 - 1), slice(0, n // 2 - 1))
        assert gb.last_kernel_plan().startswith("extract_matrix"), gb.last_kernel_plan()
        S = sp.csr_matrix((np.ones(len(col), np.float32), col.astype(np.int64), rp.astype(np.int64)), shape=(n, n))[: n // 2, : n // 2]
        assert sub.nvals == S.nnz
        # a small matrix that lives in HBM only (the result of the call above, sliced again) is not brought to the host for it
        tiny = sub.extract_matrix([5, 3], None)
        assert gb.last_kernel_plan().startswith("extract_matrix")
        tiny2 = tiny.extract_matrix(None, slice(0, 99))
        assert gb.last_kernel_plan().startswith("extract_matrix")
        exp = S[[5, 3]][:, :100].tocoo()
        order = np.lexsort((exp.col, exp.row))
        same(tiny2.to_arrays(), (exp.row[order].astype(np.uint64), exp.col[order].astype(np.uint64), exp.data[order]), "device-only chain")
        r = A.extract_row(0)
        assert gb.last_kernel_plan().startswith("extract_col")
        assert r.nvals == int(rp[1] - rp[0])
        w = r.extract(slice(0, 999))                                 # r lives in HBM only
        assert gb.last_kernel_plan().startswith("extract_vector")
        assert w.nvals == int(np.count_nonzero(col[rp[0]:rp[1]] < 1000))


# ---- 2. parity: both routes and the model -----------------------------------------------------------------------------------------
def run_matrix_case(gb, c, rng, bisect=False):
    atype, ctype = c["atype"], c["ctype"]
    nr, nc = c["nrows"], c["ncols"]
    I, J, X = random_tuples(rng, gb, atype, nr, nc, c["density"])
    onr, onc = (nc, nr) if c["t0"] else (nr, nc)
    rarg, rows = pick(c["rk"], onr, rng)
    carg, cols = pick(c["ck"], onc, rng)
    m, n = len(rows), len(cols)
    CI, CJ, CX = random_tuples(rng, gb, ctype, m, n, 0.3 if c["prefill"] else 0.0)
    MI, MJ, MX = random_tuples(rng, gb, c["mtype"], m, n, 0.5) if c["mask"] else (None, None, None)
    cdt = npdt(gb, ctype)
    T = model_T(I, J, X, nr, nc, c["t0"], rows, cols)
    Cd = {(int(a), int(b)): x for a, b, x in zip(CI, CJ, CX)}
    Md = {(int(a), int(b)): x for a, b, x in zip(MI, MJ, MX)} if c["mask"] else None
    exp = as_sorted(model_write_back(Cd, cdt, T, Md, c["mask"], c["accum"], c["replace"]), cdt)
    got = {}
    for route in (0, 1):
        A = gb.Matrix.from_arrays(I, J, X, nr, nc, typ(gb, atype))
        C = gb.Matrix.from_arrays(CI, CJ, CX, m, n, typ(gb, ctype))
        M = gb.Matrix.from_arrays(MI, MJ, MX, m, n, typ(gb, c["mtype"])) if c["mask"] else None
        acc = getattr(typ(gb, ctype), c["accum"]) if c["accum"] else None
        with env(GRB_MI355X_EXTRACT=route, GRB_MI355X_EXTRACT_BISECT=1 if bisect else None):
            out = A.extract_matrix(rarg, carg, out=C, mask=M, accum=acc, desc=descriptor(gb, c["mask"], c["replace"], c["t0"]))
            plan = gb.last_kernel_plan()
        assert out is C
        if route == 1:
            assert plan.startswith("extract_matrix"), plan
            # under T0 the kernels extract A(J, I): their column map is built from the ROW argument
            if bisect and (c["rk"] if c["t0"] else c["ck"]) in LIST_KINDS and m and n and len(X):
                assert "cols=bisect" in plan, plan
        got[route] = C.to_arrays()
        same(got[route], exp, f"route {route} vs model, case {c}")
    same(got[1], got[0], f"device route vs host route, case {c}")


@pytest.mark.parametrize("block", range(8))
def test_parity_matrix(gb, gpu, block):
    rng = np.random.default_rng(1000 + block)
    for i in range(block * 81, block * 81 + 81):                    # 648 cases: every (row kind, column kind) pair eight times
        run_matrix_case(gb, make_case(i, rng), rng)


def run_vector_case(gb, c, rng, from_matrix):
    atype, ctype = c["atype"], c["ctype"]
    cdt = npdt(gb, ctype)
    if from_matrix:
        nr, nc = c["nrows"], c["ncols"]
        I, J, X = random_tuples(rng, gb, atype, nr, nc, c["density"])
        length, width = (nc, nr) if c["t0"] else (nr, nc)           # op(A) is length x width; column j of it
        j = int(rng.integers(0, width))
        if c["t0"]:
            line = {int(b): x for a, b, x in zip(I, J, X) if int(a) == j}      # row j of A
        else:
            line = {int(a): x for a, b, x in zip(I, J, X) if int(b) == j}      # column j of A
    else:
        length = c["nrows"] * 3
        k = int(round(length * c["density"]))
        UI = np.sort(rng.choice(length, size=k, replace=False)).astype(np.uint64)
        UX = values(rng, gb, atype, k)
        line = {int(a): x for a, x in zip(UI, UX)}
    iarg, idx = pick(c["rk"], length, rng)
    m = len(idx)
    T = {(k_, 0): line[s] for k_, s in enumerate(idx) if s in line}
    WI = np.sort(rng.choice(m, size=int(round(m * 0.3)), replace=False)).astype(np.uint64) if (c["prefill"] and m) else np.zeros(0, np.uint64)
    WX = values(rng, gb, ctype, len(WI))
    MI = MX = None
    if c["mask"]:
        MI = np.sort(rng.choice(m, size=int(round(m * 0.5)), replace=False)).astype(np.uint64) if m else np.zeros(0, np.uint64)
        MX = values(rng, gb, c["mtype"], len(MI))
    Wd = {(int(a), 0): x for a, x in zip(WI, WX)}
    Md = {(int(a), 0): x for a, x in zip(MI, MX)} if c["mask"] else None
    exp = as_sorted(model_write_back(Wd, cdt, T, Md, c["mask"], c["accum"], c["replace"]), cdt, vector=True)
    got = {}
    for route in (0, 1):
        w = gb.Vector.from_arrays(WI, WX, m, typ(gb, ctype))
        M = gb.Vector.from_arrays(MI, MX, m, typ(gb, c["mtype"])) if c["mask"] else None
        acc = getattr(typ(gb, ctype), c["accum"]) if c["accum"] else None
        with env(GRB_MI355X_EXTRACT=route):
            if from_matrix:
                A = gb.Matrix.from_arrays(I, J, X, nr, nc, typ(gb, atype))
                A.extract_col(j, iarg, out=w, mask=M, accum=acc, desc=descriptor(gb, c["mask"], c["replace"], c["t0"]))
            else:
                u = gb.Vector.from_arrays(UI, UX, length, typ(gb, atype))
                u.extract(iarg, out=w, mask=M, accum=acc, desc=descriptor(gb, c["mask"], c["replace"], False))
            plan = gb.last_kernel_plan()
        if route == 1:
            assert plan.startswith("extract_col" if from_matrix else "extract_vector"), plan
        got[route] = w.to_arrays()
        same(got[route], exp, f"route {route} vs model, case {c}")
    same(got[1], got[0], f"device route vs host route, case {c}")


@pytest.mark.parametrize("block", range(4))
def test_parity_col(gb, gpu, block):
    rng = np.random.default_rng(2000 + block)
    for i in range(block * 99, block * 99 + 99):                    # 396 cases, both orientations (t0 cycles)
        run_vector_case(gb, make_case(i, rng), rng, True)


@pytest.mark.parametrize("block", range(3))
def test_parity_vector(gb, gpu, block):
    rng = np.random.default_rng(3000 + block)
    for i in range(block * 99, block * 99 + 99):                    # 297 cases
        run_vector_case(gb, make_case(i, rng), rng, False)


# ---- 4. the bisection instead of the table ------------------------------------------------------------------------------------
def test_parity_matrix_bisect(gb, gpu):
    rng = np.random.default_rng(4000)
    for i in range(0, 648, 5):                                      # 130 of test_parity_matrix's configurations
        run_matrix_case(gb, make_case(i, rng), rng, bisect=True)


# ---- 3. skew and size ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat20(gb, gpu):
    from pygraphblas_amd import rmat
    scale = 20
    n = 1 << scale
    rp, col = rmat.csr_numpy(scale, seed=42)
    vals = (np.arange(len(col), dtype=np.int64) % 251 + 1).astype(np.float32)
    S = sp.csr_matrix((vals, col.astype(np.int64), rp.astype(np.int64)), shape=(n, n))
    A = gb.Matrix.from_csr(gb.FP32, n, n, rp, col, vals)            # lives in HBM only
    return n, S, A


def compare_with_scipy(sub, exp, what):
    exp = exp.tocsr()
    exp.sort_indices()
    assert (sub.nrows, sub.ncols) == exp.shape
    ei = np.repeat(np.arange(exp.shape[0], dtype=np.uint64), np.diff(exp.indptr))
    same(sub.to_arrays(), (ei, exp.indices.astype(np.uint64), exp.data), what)


def selections(n, S):
    rng = np.random.default_rng(7)
    deg = np.diff(S.indptr)
    hubs = np.argsort(-deg, kind="stable")[:64]
    nb = np.unique(np.concatenate([S.indices[S.indptr[h]:S.indptr[h + 1]] for h in hubs[:4]] + [hubs]))
    sample = np.sort(rng.choice(n, size=n // 10, replace=False))
    shuffled = rng.permutation(sample)
    shuffled[rng.choice(len(shuffled), size=len(shuffled) // 100, replace=False)] = shuffled[0]
    return {"range": (slice(0, n // 2 - 1), np.arange(n // 2)), "sorted sample": (sample, sample), "shuffled with repeats": (shuffled, shuffled),
            "hubs and neighbours": (nb, nb)}, hubs, deg


@pytest.mark.parametrize("which", ["range", "sorted sample", "shuffled with repeats", "hubs and neighbours"])
def test_rmat20_induced_subgraph(gb, gpu, rmat20, which):
    n, S, A = rmat20
    sel, hubs, deg = selections(n, S)
    arg, idx = sel[which]
    if which == "hubs and neighbours":
        assert int((deg[hubs] >= 4096).sum()) >= 1 and set(hubs.tolist()) <= set(idx.tolist()), "hub rows of >= 4096 entries must be selected: the long-row path"
    with env(GRB_MI355X_EXTRACT=None):
        sub = A.extract_matrix(arg, arg)
        plan = gb.last_kernel_plan()
    assert plan.startswith("extract_matrix"), plan
    exp = S[idx][:, idx].tocsr()
    # the result is a usable device matrix: a product straight away, then all tuples
    x = (np.arange(len(idx)) % 7 + 1).astype(np.float32)
    xv = gb.Vector.from_arrays(np.arange(len(idx), dtype=np.uint64), x, len(idx), gb.FP32)
    y = sub.mxv(xv, semiring=gb.FP32.PLUS_TIMES)
    yi, yx = y.to_arrays()
    ye = exp.astype(np.float64) @ x.astype(np.float64)
    rows_with = np.flatnonzero(np.diff(exp.indptr))
    assert np.array_equal(yi, rows_with.astype(np.uint64))
    assert np.allclose(yx, ye[rows_with], rtol=1e-5, atol=0)         # FP32 sums of integer-valued terms in another order than scipy's FP64
    compare_with_scipy(sub, exp, which)


def test_rmat20_rows(gb, gpu, rmat20):
    n, S, A = rmat20
    deg = np.diff(S.indptr)
    hub, empty = int(np.argmax(deg)), int(np.flatnonzero(deg == 0)[0])
    for r in (hub, empty):
        v = A.extract_row(r)
        assert gb.last_kernel_plan().startswith("extract_col"), gb.last_kernel_plan()
        same(v.to_arrays(), (S.indices[S.indptr[r]:S.indptr[r + 1]].astype(np.uint64), S.data[S.indptr[r]:S.indptr[r + 1]]), f"row {r}")
    # a column of the by-row matrix, under a list: no transpose is built
    c = int(S.indices[S.indptr[hub]])
    idx = np.arange(0, n, 3)
    v = A.extract_col(c, idx)
    col = np.asarray(S[:, [c]].todense()).ravel()[idx]
    same(v.to_arrays(), (np.flatnonzero(col).astype(np.uint64), col[np.flatnonzero(col)]), "column under a list")


# ---- 5. errors: the same exception classes on both routes ------------------------------------------------------------------
def test_errors_unchanged(gb, gpu):
    rng = np.random.default_rng(5)
    I, J, X = random_tuples(rng, gb, "INT64", 20, 10, 0.3)
    seen = {}
    for route in (0, 1):
        A = gb.Matrix.from_arrays(I, J, X, 20, 10, gb.INT64)
        u = gb.Vector.from_arrays(np.arange(10, dtype=np.uint64), np.arange(10, dtype=np.int64), 10, gb.INT64)
        calls = {
            "matrix row index out of range": lambda: A.extract_matrix([1, 20], None),
            "matrix column range out of range": lambda: A.extract_matrix(None, slice(2, 10)),
            "matrix backwards range out of range": lambda: A.extract_matrix(slice(25, 3, -2), None),
            "matrix wrong output shape": lambda: A.extract_matrix([1, 2], None, out=gb.Matrix.sparse(gb.INT64, 3, 10)),
            "matrix mask shape": lambda: A.extract_matrix([1, 2], None, mask=gb.Matrix.sparse(gb.BOOL, 2, 9)),
            "col index out of range": lambda: A.extract_col(10),
            "col list out of range": lambda: A.extract_col(1, [0, 20]),
            "col wrong output size": lambda: A.extract_col(1, [0, 2], out=gb.Vector.sparse(gb.INT64, 3)),
            "col mask size": lambda: A.extract_col(1, [0, 2], mask=gb.Vector.sparse(gb.BOOL, 3)),
            "row index out of range": lambda: A.extract_row(20),
            "vector index out of range": lambda: u.extract([3, 10]),
            "vector wrong output size": lambda: u.extract([3, 4], out=gb.Vector.sparse(gb.INT64, 5)),
            "vector mask size": lambda: u.extract([3, 4], mask=gb.Vector.sparse(gb.BOOL, 5)),
        }
        with env(GRB_MI355X_EXTRACT=route):
            for name, call in calls.items():
                with pytest.raises(Exception) as e:
                    call()
                seen.setdefault(name, []).append((e.type, str(e.value)))
    for name, (host, device) in seen.items():
        assert host[0] is device[0], (name, host, device)
        assert host[0].__module__.startswith("pygraphblas_amd"), (name, host)      # a GraphBLAS error of the package, not a Python accident


# ---- 6. the reference's own slicing examples ----------------------------------------------------------------------------------
def _index(spec):
    if spec is None or isinstance(spec, (int, list)):
        return spec
    return slice(*spec["slice"])


def test_reference_slicing_examples(gb, gpu):
    with open(os.path.join(HERE, "golden", "reference_extract_vectors.json")) as f:
        doc = json.load(f)
    assert len(doc["cases"]) >= 20
    for route in (0, 1):
        with env(GRB_MI355X_EXTRACT=route):
            for case in doc["cases"]:
                src, T = case["input"], typ(gb, case["input"]["type"])
                where = f"{case['source']} on route {route}"
                if "J" in src:
                    A = gb.Matrix.from_arrays(np.array(src["I"], np.uint64), np.array(src["J"], np.uint64), np.array(src["V"], T._np), src["nrows"], src["ncols"], T)
                else:
                    A = gb.Vector.from_arrays(np.array(src["I"], np.uint64), np.array(src["V"], T._np), src["size"], T)
                for step in case["steps"]:                            # each step slices the result of the one before
                    op = step["op"]
                    if op == "getitem":
                        key = [slice(None) if k is None else _index(k) for k in step["key"]]      # `:` in a subscript
                        A = A[key[0]] if len(key) == 1 else A[key[0], key[1]]
                    elif op == "extract_matrix":
                        A = A.extract_matrix(_index(step["rows"]), _index(step["cols"]))
                    elif op == "extract_col":
                        A = A.extract_col(step["j"])
                    elif op == "extract_row":
                        A = A.extract_row(step["i"])
                    else:
                        A = A.extract(_index(step["index"]))
                e = case["expect"]
                if "J" in e:
                    assert (A.nrows, A.ncols) == (e["nrows"], e["ncols"]), where
                    same(A.to_arrays(), (np.array(e["I"], np.uint64), np.array(e["J"], np.uint64), np.array(e["V"], A.type._np)), where)
                else:
                    assert A.size == e["size"], where
                    same(A.to_arrays(), (np.array(e["I"], np.uint64), np.array(e["V"], A.type._np)), where)
