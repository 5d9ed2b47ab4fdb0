"""Element edits and resize of containers that live in HBM only (grb_edit.hip behind setElement / removeElement / resize, the queue in grb_edit_ops.cpp).

The model is a Python dict replayed edit by edit; values are small integers, so every comparison is exact.  Containers are imported straight into HBM
(`from_csr` / `from_dense_array` copy host arrays into fresh device allocations: no host mirror) or are the output of an operation, and residency 2 is asserted
before anything is edited.

Queues of 1, 7 and 3 000 edits: the edit classes of the list below are 15 records, so they are queued one record at a time (every class as a queue of its
own), in queues of 7 (same-coordinate pairs kept together), and once inside one queue of 3 000 (the classes, then random edits).  After every queue: the
touched coordinates are read BEFORE anything flushed (the queue answers), residency is still 2, `nvals` (a flush point) equals the model and the plan string
starts with `edit<`; after the last queue `to_arrays()` and reads of touched and untouched coordinates equal the model.

The long-row shape is 3 000 x 8 000: a row of 5 000 entries does not fit 3 000 columns.  The 3-entry fill state comes twice: imported like the others, and
as the result of `w.assign_scalar(1, mask=q)` on an empty w and a short q made from lists — that vector lives in HBM only AND carries the `small_idx` list the
tiny-push path of vxm consumes on a matrix of 2^20 entries or more (test_vector_with_a_small_list).  After a resize to 0 rows or to size 0 no
product or reduction follows (there is nothing to combine)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TYPES = ["BOOL", "INT16", "FP32", "FP64"]                        # one per value width


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


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def typed(name, x):
    return bool(x & 1) if name == "BOOL" else x


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------

def base_model(shape, name):
    """{(i, j): value} of the shapes of the issue; deterministic."""
    rng = np.random.default_rng(11)
    if shape == "empty":
        return {}, 5, 5
    if shape == "one":
        return {}, 1, 1
    nr, nc = 3000, (8000 if shape == "long" else 3000)
    lens = rng.integers(0, 27, nr)
    lens[:4] = (60, 0, 1, 60)
    lens[5], lens[7], lens[nr - 1] = 0, 1, 3                     # an empty row, a row with one entry
    model = {}
    for i in range(nr):
        cols = rng.choice(2998, size=int(lens[i]), replace=False) + 1          # columns 1 .. 2998: (0, 0) and the last column start absent
        for j in cols:
            model[(i, int(j))] = typed(name, int(rng.integers(1, 50)))
    if shape == "long":
        for j in rng.choice(7998, size=5000, replace=False) + 1:
            model[(9, int(j))] = typed(name, int(rng.integers(1, 50)))
    return model, nr, nc


def import_matrix(gb, name, model, nr, nc):
    T = getattr(gb, name)
    keys = sorted(model)
    rows = np.array([k[0] for k in keys], np.int64)
    rp = np.zeros(nr + 1, np.uint32)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp).astype(np.uint32)
    A = gb.Matrix.from_csr(T, nr, nc, rp, np.array([k[1] for k in keys], np.uint32), np.array([model[k] for k in keys], T._np))
    assert residency(gb, A) == 2
    return A


def edit_classes(model, nr, nc, name):
    """The classes of the issue as groups of records (a group stays in one queue): ('set', i, j, x) / ('del', i, j)."""
    rows = {}
    for (i, j) in model:
        rows.setdefault(i, []).append(j)
    stored = sorted(model)
    groups = []
    if stored:
        groups.append([("set", *stored[len(stored) // 2], 51)])                               # overwrite
    empty = [i for i in range(nr) if i not in rows]
    if empty:
        groups.append([("set", empty[0], nc // 2, 52)])                                       # insert into an empty row
    full = [i for i in sorted(rows) if min(rows[i]) > 0 and max(rows[i]) < nc - 1 and len(rows[i]) > 1]
    if full:
        i = full[len(full) // 3]
        groups.append([("set", i, min(rows[i]) - 1, 53)])                                     # before the first entry of a row
        groups.append([("set", i, max(rows[i]) + 1, 54)])                                     # after the last
    groups.append([("set", 0, 0, 55)])
    groups.append([("set", nr - 1, nc - 1, 56)])
    if len(stored) > 10:
        groups.append([("del", *stored[len(stored) // 3])])                                   # a stored entry
    absent = next((i, j) for i in range(nr - 1, -1, -1) for j in range(nc - 1, -1, -1) if (i, j) not in model and (i, j) != (nr - 1, nc - 1))  if nr * nc > 1 else None
    if absent:
        groups.append([("del", *absent)])                                                     # an absent entry
    single = [i for i in sorted(rows) if len(rows[i]) == 1]
    if single:
        groups.append([("del", single[0], rows[single[0]][0])])                               # a row's only entry
    a = (nr // 2, nc // 3)
    groups.append([("set", *a, 57), ("del", *a)])                                             # set then delete
    b = stored[len(stored) // 5] if stored else (nr - 1, 0)
    groups.append([("del", *b), ("set", *b, 58)])                                             # delete then set
    c = (nr // 3, nc // 2)
    groups.append([("set", *c, 59), ("set", *c, 60)])                                         # two sets of one coordinate
    return groups


def apply_records(A, model, records, name):
    for r in records:
        if r[0] == "set":
            A[r[1], r[2]] = typed(name, r[3])
            model[(r[1], r[2])] = typed(name, r[3])
        else:
            del A[r[1], r[2]]
            model.pop((r[1], r[2]), None)


def check_after_queue(gb, A, model, records, device):
    for r in records:                                            # read before any flush: the queue answers
        assert A.get(r[1], r[2]) == model.get((r[1], r[2])), r
    if device:
        assert residency(gb, A) == 2
        assert A.nvals == len(model)
        assert residency(gb, A) == 2
        assert gb.last_kernel_plan().startswith("edit<on=matrix,"), gb.last_kernel_plan()
    else:
        assert residency(gb, A) == 1                             # GRB_MI355X_EDIT=0: the host mirror took over, as before
        assert A.nvals == len(model)


def check_contents(A, model, nr, nc, touched):
    assert A.shape == (nr, nc) and A.nvals == len(model)
    rng = np.random.default_rng(3)
    for (i, j) in list(touched)[:40] + [(int(rng.integers(nr)), int(rng.integers(nc))) for _ in range(20 if nr and nc else 0)] + sorted(model)[:: max(1, len(model) // 20)]:
        assert A.get(i, j) == model.get((i, j)), (i, j)
    I, J, X = A.to_arrays()
    keys = sorted(model)
    assert np.array_equal(I, np.array([k[0] for k in keys], np.uint64)) and np.array_equal(J, np.array([k[1] for k in keys], np.uint64))
    assert np.array_equal(X, np.array([model[k] for k in keys], X.dtype))


def queues_of(groups, size):
    """The groups as queues of at most `size` records (a group is never split; size 1: its records one by one, in order)."""
    if size == 1:
        return [[r] for g in groups for r in g]
    out, cur = [], []
    for g in groups:
        if len(cur) + len(g) > size:
            out.append(cur); cur = []
        cur = cur + g
    return out + [cur]


def random_records(rng, model, nr, nc, n):
    stored = sorted(model)
    recs = []
    for _ in range(n):
        how = int(rng.integers(4))
        if how == 0 and stored:
            i, j = stored[int(rng.integers(len(stored)))]
        elif how == 1 and recs:
            i, j = recs[int(rng.integers(len(recs)))][1:3]
        else:
            i, j = int(rng.integers(nr)), int(rng.integers(nc))
        recs.append(("del", i, j) if rng.integers(3) == 0 else ("set", i, j, int(rng.integers(1, 50))))
    return recs


def run_matrix_case(gb, name, shape, size, device=True):
    model, nr, nc = base_model(shape, name)
    A = import_matrix(gb, name, model, nr, nc)
    groups = edit_classes(model, nr, nc, name)
    if size == 3000:
        recs = [r for g in groups for r in g]
        queues = [recs + random_records(np.random.default_rng(17), model, nr, nc, 3000 - len(recs))]
        assert len(queues[0]) == 3000
    else:
        queues = queues_of(groups, size)
    touched = []
    for q in queues:
        apply_records(A, model, q, name)
        touched += [(r[1], r[2]) for r in q]
        check_after_queue(gb, A, model, q, device)
    check_contents(A, model, nr, nc, touched)


@pytest.mark.parametrize("size", [1, 7, 3000])
@pytest.mark.parametrize("shape", ["empty", "one", "square", "long"])
@pytest.mark.parametrize("name", TYPES)
def test_matrix_edit_queues(gb, name, shape, size):
    run_matrix_case(gb, name, shape, size)


@pytest.mark.parametrize("name,shape,size", [("FP64", "square", 7), ("BOOL", "long", 3000), ("INT16", "empty", 1), ("FP32", "square", 3000)])
def test_matrix_edits_on_the_host_route(gb, name, shape, size):
    """GRB_MI355X_EDIT=0: today's route, the same contents, residency 1."""
    with env(GRB_MI355X_EDIT="0"):
        run_matrix_case(gb, name, shape, size, device=False)


def test_output_of_an_operation_is_edited_in_hbm(gb):
    model, nr, nc = base_model("square", "FP64")
    A = import_matrix(gb, "FP64", model, nr, nc)
    B = A.apply(gb.FP64.AINV)                                     # lives in HBM only
    assert residency(gb, B) == 2
    neg = {k: -v for k, v in model.items()}
    recs = [("set", 5, 5, 3), ("del", *sorted(model)[100]), ("set", *sorted(model)[200], 4)]
    apply_records(B, neg, recs, "FP64")
    check_after_queue(gb, B, neg, recs, True)
    check_contents(B, neg, nr, nc, [(r[1], r[2]) for r in recs])


def products(gb, A, model, nr, nc):
    """A.mxv(1) and 1.vxm(A) against the row and column sums of the model (small integers: exact in FP64)."""
    want_r, want_c = np.zeros(nr), np.zeros(nc)
    for (i, j), x in model.items():
        want_r[i] += x; want_c[j] += x
    ur, uc = gb.Vector.dense(gb.FP64, nc, fill=1.0), gb.Vector.dense(gb.FP64, nr, fill=1.0)
    w = A.mxv(ur, semiring=gb.FP64.PLUS_TIMES)
    x, p = w.to_dense_arrays()
    assert np.array_equal(p != 0, want_r != 0) and np.array_equal(np.where(p != 0, x, 0.0), want_r)
    w = uc.vxm(A, semiring=gb.FP64.PLUS_TIMES)
    x, p = w.to_dense_arrays()
    assert np.array_equal(p != 0, want_c != 0) and np.array_equal(np.where(p != 0, x, 0.0), want_c)


def test_derived_data_is_not_stale_after_an_edit(gb):
    """Plans and the transpose cache exist before the edit; both products see the edit, value-only and structural."""
    model, nr, nc = base_model("square", "FP64")
    A = import_matrix(gb, "FP64", model, nr, nc)
    products(gb, A, model, nr, nc)
    products(gb, A, model, nr, nc)
    stored = sorted(model)
    recs = [("set", *stored[k], 40 + k % 9) for k in range(0, len(stored), 997)]                 # overwrites only
    apply_records(A, model, recs, "FP64")
    assert residency(gb, A) == 2
    products(gb, A, model, nr, nc)                               # the product is the flush point
    assert residency(gb, A) == 2
    A.nvals
    recs = [("set", 5, 100, 7), ("del", *stored[50]), ("set", 2999, 2999, 9), ("del", *stored[-1]), ("set", *stored[10], 3)]
    apply_records(A, model, recs, "FP64")
    products(gb, A, model, nr, nc)
    assert residency(gb, A) == 2 and A.nvals == len(model)
    products(gb, A, model, nr, nc)


RESIZES = [(1500, 3000), (3000, 1500), (1000, 2000), (4000, 5000), (3000, 3000), (0, 3000)]     # rows, columns, both, grow both, unchanged, no rows


@pytest.mark.parametrize("dims", RESIZES)
@pytest.mark.parametrize("name", TYPES)
def test_matrix_resize_in_hbm(gb, name, dims):
    model, nr, nc = base_model("square", name)
    A = import_matrix(gb, name, model, nr, nc)
    A[7, 2999] = typed(name, 5); model[(7, 2999)] = typed(name, 5)            # a queued edit: the resize applies it first
    A.resize(*dims)
    assert gb.last_kernel_plan().startswith("resize<on=matrix,rows=%d,cols=%d>" % dims), gb.last_kernel_plan()
    want = {k: v for k, v in model.items() if k[0] < dims[0] and k[1] < dims[1]}
    assert residency(gb, A) == 2 and A.shape == dims and A.nvals == len(want) and residency(gb, A) == 2
    if dims[0] and name == "FP64":
        products(gb, A, want, *dims)
        assert residency(gb, A) == 2
    check_contents(A, want, dims[0], dims[1], [(7, 2999)] if 7 < dims[0] and 2999 < dims[1] else [])


def test_resize_beyond_the_device_range_takes_the_host_route(gb):
    model, nr, nc = base_model("square", "FP32")
    A = import_matrix(gb, "FP32", model, nr, nc)
    A.resize()                                                   # the reference's default: 2^60 x 2^60
    assert A.shape == (1 << 60, 1 << 60) and residency(gb, A) == 1 and A.nvals == len(model)
    I, J, X = A.to_arrays()
    keys = sorted(model)
    assert list(zip(I.tolist(), J.tolist())) == keys and X.tolist() == [model[k] for k in keys]
    v = import_vector(gb, "FP32", {3: 1, 99999: 2}, 100000)
    v.resize()
    assert v.size == 1 << 60 and residency(gb, v) == 1 and v.to_lists() == [[3, 99999], [1.0, 2.0]]


# ---- vectors ------------------------------------------------------------------------------------------------------------------------------

N = 100000


def import_vector(gb, name, model, n):
    T = getattr(gb, name)
    dense, present = np.zeros(n, T._np), np.zeros(n, np.uint8)
    for i, x in model.items():
        dense[i] = x; present[i] = 1
    v = gb.Vector.from_dense_array(dense, T, present=present)
    assert residency(gb, v) == 2
    return v


def vector_model(fill, name):
    rng = np.random.default_rng(23)
    if fill == "three":
        idx = [10, 50000, N - 2]
    elif fill == "half":
        idx = np.sort(rng.choice(N - 2, size=N // 2, replace=False) + 1).tolist()
    else:
        idx = range(N)
    return {int(i): typed(name, 1 + (int(i) * 7) % 40) for i in idx}


def check_vector(v, model, n):
    assert v.size == n and v.nvals == len(model)
    x, p = v.to_dense_arrays()
    want_p = np.zeros(n, bool); want_x = np.zeros(n, x.dtype)
    for i, val in model.items():
        want_p[i] = True; want_x[i] = val
    assert np.array_equal(p != 0, want_p) and np.array_equal(np.where(want_p, x, 0), want_x)


def reduce_of(gb, v, name):
    return v.reduce_bool() if name == "BOOL" else v.reduce_int() if name == "INT16" else v.reduce_float()


def model_reduce(model, name):
    return any(model.values()) if name == "BOOL" else sum(model.values())


@pytest.fixture(scope="module")
def mask_operands(gb):
    """u (50 ones) and A (50 x N, about 2 000 entries) of `u.vxm(A, mask=v)`, and the column sums of A."""
    rng = np.random.default_rng(29)
    flat = np.sort(rng.choice(50 * N, size=2000, replace=False))
    I, J = np.divmod(flat, N)
    J[:4] = (0, 10, 11, N - 1)                                   # the columns the edits touch are among them
    X = rng.integers(1, 9, len(flat)).astype(np.float64)
    order = np.lexsort((J, I))
    A = gb.Matrix.from_arrays(I[order].astype(np.uint64), J[order].astype(np.uint64), X[order], 50, N, gb.FP64, dup=gb.FP64.PLUS)
    sums = np.zeros(N)
    np.add.at(sums, J, X)
    return gb.Vector.dense(gb.FP64, 50, fill=1.0), A, sums


def check_as_mask(gb, v, model, mask_operands):
    u, A, sums = mask_operands
    w = u.vxm(A, semiring=gb.FP64.PLUS_TIMES, mask=v)
    x, p = w.to_dense_arrays()
    allow = np.zeros(N, bool)
    for i, val in model.items():
        allow[i] = bool(val)
    want = np.where(allow, sums, 0.0)
    assert np.array_equal(p != 0, want != 0) and np.array_equal(np.where(p != 0, x, 0.0), want)


VECTOR_EDITS = [("set", 0, 41), ("set", 10, 42), ("del", 11), ("del", 50000), ("set", N - 1, 43), ("set", 777, 44), ("del", 777), ("del", N - 2), ("set", N - 2, 45),
                ("set", 31, 46), ("set", 31, 47), ("del", 0), ("set", 0, 48)]


def apply_vector_records(v, model, records, name):
    for r in records:
        if r[0] == "set":
            v[r[1]] = typed(name, r[2]); model[r[1]] = typed(name, r[2])
        else:
            del v[r[1]]; model.pop(r[1], None)


@pytest.mark.parametrize("fill", ["three", "half", "full"])
@pytest.mark.parametrize("name", TYPES)
def test_vector_edits(gb, mask_operands, name, fill):
    model = vector_model(fill, name)
    v = import_vector(gb, name, model, N)
    assert reduce_of(gb, v, name) == model_reduce(model, name) and v.nvals == len(model)
    check_as_mask(gb, v, model, mask_operands)
    apply_vector_records(v, model, VECTOR_EDITS, name)
    for r in VECTOR_EDITS:                                       # read before any flush
        assert v.get(r[1]) == model.get(r[1]), r
    assert residency(gb, v) == 2
    assert v.nvals == len(model) and residency(gb, v) == 2
    assert gb.last_kernel_plan().startswith("edit<on=vector,"), gb.last_kernel_plan()
    assert reduce_of(gb, v, name) == model_reduce(model, name)
    check_as_mask(gb, v, model, mask_operands)
    apply_vector_records(v, model, [("del", 10), ("set", 12, 3)], name)        # a second queue, flushed by the product
    check_as_mask(gb, v, model, mask_operands)
    assert residency(gb, v) == 2
    check_vector(v, model, N)


def test_vector_edits_on_the_host_route(gb):
    with env(GRB_MI355X_EDIT="0"):
        for name, fill in (("FP64", "half"), ("BOOL", "three")):
            model = vector_model(fill, name)
            v = import_vector(gb, name, model, N)
            apply_vector_records(v, model, VECTOR_EDITS, name)
            assert residency(gb, v) == 1
            check_vector(v, model, N)


def test_vector_edit_with_a_deferred_chain_pending(gb):
    """w is the output of queued element-wise work when the edit arrives: the chain completes first, then the edit is queued for the device."""
    a, b = vector_model("half", "FP64"), vector_model("full", "FP64")
    va, vb = import_vector(gb, "FP64", a, N), import_vector(gb, "FP64", b, N)
    w = va.emult(vb, gb.FP64.PLUS)
    w = w.apply_second(gb.FP64.TIMES, 2.0)
    model = {i: 2.0 * (a[i] + b[i]) for i in a}
    recs = [("set", 0, 5), ("del", sorted(a)[3]), ("set", sorted(a)[4], 6)]
    apply_vector_records(w, model, recs, "FP64")
    for r in recs:
        assert w.get(r[1]) == model.get(r[1])
    assert residency(gb, w) == 2
    check_vector(w, model, N)
    assert residency(gb, w) == 2


@pytest.mark.parametrize("n", [50000, 150000, N, 0, 3000])
@pytest.mark.parametrize("name", TYPES)
def test_vector_resize_in_hbm(gb, name, n):
    model = vector_model("half", name)
    v = import_vector(gb, name, model, N)
    v[N - 1] = typed(name, 9); model[N - 1] = typed(name, 9)     # a queued edit: the resize applies it first
    v.resize(n)
    assert gb.last_kernel_plan().startswith("resize<on=vector,rows=%d," % n), gb.last_kernel_plan()
    want = {i: x for i, x in model.items() if i < n}
    assert residency(gb, v) == 2 and v.size == n
    if n:
        assert reduce_of(gb, v, name) == model_reduce(want, name)
    if n == 3000:                                                # followed by a product
        m, nr, nc = base_model("square", "FP64")
        A = import_matrix(gb, "FP64", m, nr, nc)
        w = v.vxm(A, semiring=gb.FP64.PLUS_TIMES)
        cols = np.zeros(nc)
        for (i, j), x in m.items():
            cols[j] += x * want.get(i, 0)
        x, p = w.to_dense_arrays()
        assert np.array_equal(np.where(p != 0, x, 0.0), cols)
    check_vector(v, want, n)
    assert residency(gb, v) == 2


# ---- a matrix large enough for the overwrite in place and the device lookup (>= 2^16 entries), and for the tiny push of vxm (>= 2^20) ----------------

@pytest.fixture(scope="module")
def big_matrix(gb):
    """100 000 x 100 000, FP64, about 1.2 million entries (small integers) as CSR arrays, and the matrix in HBM only."""
    rng = np.random.default_rng(31)
    keys = np.unique(rng.integers(0, N * N, 1_250_000))
    rows, col = np.divmod(keys, N)
    rp = np.zeros(N + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp)
    val = rng.integers(1, 9, len(keys)).astype(np.float64)
    assert len(keys) >= 1 << 20
    A = gb.Matrix.from_csr(gb.FP64, N, N, rp.astype(np.uint32), col.astype(np.uint32), val)
    assert residency(gb, A) == 2
    return A, rp, col, val


def test_overwrite_in_place_and_device_lookup_with_a_queue(gb):
    """About 70 000 entries: with an empty queue an overwrite is stored in place (no `edit<` plan) and a read is a device lookup; with edits queued the
    overwrite of a stored entry joins the queue, so delete / set / delete of one stored coordinate keep their order."""
    rng = np.random.default_rng(37)
    nr = nc = 3000
    keys = np.unique(rng.integers(0, nr * nc, 72000))
    model = {(int(k // nc), int(k % nc)): int(rng.integers(1, 50)) for k in keys}
    assert len(model) >= 1 << 16
    A = import_matrix(gb, "FP64", model, nr, nc)
    stored = sorted(model)
    a, b, c = stored[100], stored[20000], stored[-5]
    A.apply(gb.FP64.AINV)                                        # (an operation of its own: the plan string is that operation's now)
    before = gb.last_kernel_plan()
    assert not before.startswith("edit<")
    A[a] = 77; model[a] = 77                                     # empty queue, stored entry: in place
    assert residency(gb, A) == 2 and gb.last_kernel_plan() == before                       # no flush ran
    assert A[a] == 77 and A.get(0, 0) == model.get((0, 0)) and residency(gb, A) == 2      # device lookups
    absent = next((i, 5) for i in range(nr) if (i, 5) not in model)
    A[absent] = 5; model[absent] = 5                             # a new position: queued
    A[b] = 78; model[b] = 78                                     # stored, but the queue is not empty: queued behind it
    del A[c]; A[c] = 79; del A[c]; model.pop(c)                  # one stored coordinate three times
    assert A[b] == 78 and A.get(*c) is None and A[absent] == 5  # the queue answers
    assert residency(gb, A) == 2
    assert A.get(*stored[7]) == model[stored[7]]                 # not in the queue: flush, then the device lookup
    assert gb.last_kernel_plan().startswith("edit<on=matrix,set=1,ins=1,del=1>"), gb.last_kernel_plan()
    assert residency(gb, A) == 2 and A.nvals == len(model)
    A[c] = 80; model[c] = 80                                     # absent now, empty queue: queued as an insert
    assert A[c] == 80 and A[a] == 77 and A.get(*b) == 78 and residency(gb, A) == 2
    check_contents(A, model, nr, nc, [a, b, c, absent])


def test_vector_with_a_small_list(gb, big_matrix):
    """`w.assign_scalar(1, mask=q)` on an empty w and a short q made from lists leaves w in HBM only WITH its entries as a list (small_idx): the operand the tiny
    push of vxm takes without counting.  Edits must not leave a stale list behind: nvals, reduce, w as operand and as mask of vxm, before and after."""
    A, rp, col, val = big_matrix
    ones = gb.Vector.dense(gb.FP64, N, fill=1.0)
    colsum = np.zeros(N)
    np.add.at(colsum, col, val)

    def check(w, model):
        want = np.zeros(N)
        for i, x in model.items():
            np.add.at(want, col[rp[i]:rp[i + 1]], x * val[rp[i]:rp[i + 1]])
        out = w.vxm(A, semiring=gb.FP64.PLUS_TIMES)              # operand: the rows of its entries
        x, p = out.to_dense_arrays()
        assert np.array_equal(p != 0, want != 0) and np.array_equal(np.where(p != 0, x, 0.0), want), gb.last_kernel_plan()
        assert w.nvals == len(model) and w.reduce_float() == sum(model.values())
        allow = np.zeros(N, bool)
        allow[list(model)] = True
        out = ones.vxm(A, semiring=gb.FP64.PLUS_TIMES, mask=w)   # mask
        x, p = out.to_dense_arrays()
        want = np.where(allow, colsum, 0.0)
        assert np.array_equal(p != 0, want != 0) and np.array_equal(np.where(p != 0, x, 0.0), want)
        assert residency(gb, w) == 2

    rows = [int(r) for r in np.flatnonzero(np.diff(rp) > 0)[[3, 500, 9000, 40000, 77777]]]      # rows with entries
    w = gb.Vector.sparse(gb.FP64, N)
    q = gb.Vector.from_lists(rows[:3], [True, True, True], N, gb.BOOL)
    w.assign_scalar(1.0, mask=q)
    assert residency(gb, w) == 2
    model = {i: 1.0 for i in rows[:3]}
    check(w, model)
    check(w, model)                                              # (the second product finds the transpose cache and the plans of the first)
    w[rows[3]] = 2.0; model[rows[3]] = 2.0                       # a new entry
    del w[rows[0]]; model.pop(rows[0])                           # a listed entry goes
    w[rows[1]] = 3.0; model[rows[1]] = 3.0                       # a listed entry changes
    assert w.get(rows[0]) is None and w[rows[3]] == 2.0 and residency(gb, w) == 2
    check(w, model)
    w[rows[4]] = 4.0; model[rows[4]] = 4.0
    del w[rows[3]]; model.pop(rows[3])
    check(w, model)                                              # the product is the flush point this time
    check_vector(w, model, N)
