"""Index lists that lie in HBM: torch tensors and vectors as I / J of extract and assign (grb_index.hip behind the GrBX_*_at and GrBX_*_Vector entry points).

The reference of every case is the SAME call with the list as a numpy array — the route pinned by test_extract_gpu.py / test_assign_gpu.py — and the result must
be bit-identical (to_arrays, values compared as bytes); the vector cases are compared with numpy fancy indexing as well.  The sizes of the parse-kernel cases come
from the kernel's own geometry (GrBX_index_geometry)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

GXB_RANGE = 0x7FFFFFFFFFFFFFFF
MASKS = [None, "valued", "structural+complemented"]
VALUE_TYPES = ["FP64", "INT8", "BOOL", "UINT16"]                    # one per value width
EXTRACT_KINDS = ["increasing", "shuffled", "repeats", "empty", "single"]
OTHERS = ["all", "range", "list"]                                   # what faces a device list on the other side of a matrix form
ASSIGN_KINDS = ["increasing", "shuffled", "empty", "single"]        # (a repeat in an assign list keeps the host route: test_assign_with_a_repeat_*)


def info_code(gb, name):
    return gb._capi.constants[name]


def geometry(gb):
    out = (C.c_uint64 * 2)()
    assert gb.lib.GrBX_index_geometry(out) == 0
    return int(out[0]), int(out[1])


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want, what):
    g, w = got.to_arrays(), want.to_arrays()
    assert len(g) == len(w), what
    for a, b in zip(g, w):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (what, a[:8], b[:8], a.shape, b.shape)


def dev(a, offset=0):
    """an int64 list as a GPU tensor; offset 1: a view t[1:] of a tensor that starts 16-byte aligned, so the list itself is only 8-byte aligned"""
    import torch
    a = np.asarray(a, np.int64)
    t = torch.from_numpy(np.concatenate([np.zeros(offset, np.int64), a, np.zeros(2, np.int64)])).cuda()      # (two spare words: an empty list still has an address)
    assert t.data_ptr() % 16 == 0
    return t[offset:offset + len(a)]


def ptr(t):
    return C.c_void_p(t.data_ptr())


def values(rng, gb, name, n):
    if name == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    if name.startswith("FP"):
        return rng.standard_normal(n).astype(getattr(gb, name)._np)
    return rng.integers(0, 6, n).astype(getattr(gb, name)._np)


def pick(kind, d, rng):
    if kind == "increasing":
        return np.sort(rng.choice(d, size=int(rng.integers(2, d + 1)), replace=False)).astype(np.int64)
    if kind == "shuffled":
        return rng.permutation(d)[: int(rng.integers(2, d + 1))].astype(np.int64)
    if kind == "repeats":
        lst = rng.integers(0, d, int(rng.integers(2, d + 8))).astype(np.int64)
        lst[-1] = lst[0]
        return lst
    if kind == "empty":
        return np.zeros(0, np.int64)
    return rng.integers(0, d, 1).astype(np.int64)


def descriptor(gb, mask_kind, replace, t0):
    d = None
    parts = ([gb.descriptor.R] if replace else []) + ([gb.descriptor.S, gb.descriptor.C] if mask_kind == "structural+complemented" else []) + ([gb.descriptor.T0] if t0 else [])
    for p in parts:
        d = p if d is None else (d & p)
    return d


def random_matrix(rng, gb, name, nrows, ncols, nnz):
    flat = np.sort(rng.choice(nrows * ncols, size=min(nnz, nrows * ncols), replace=False))
    I, J = np.divmod(flat, ncols)
    return gb.Matrix.from_arrays(I.astype(np.uint64), J.astype(np.uint64), values(rng, gb, name, len(flat)), nrows, ncols, getattr(gb, name))


def random_vector(rng, gb, name, n, fill=0.5):
    I = np.sort(rng.choice(n, size=int(n * fill), replace=False)).astype(np.uint64) if n else np.zeros(0, np.uint64)
    return gb.Vector.from_arrays(I, values(rng, gb, name, len(I)), n, getattr(gb, name))


def hbm_matrix(gb, A):
    """a copy of A that lives in HBM only"""
    I, J, X = A.to_arrays()
    S = sp.csr_matrix((np.arange(len(X)), (I.astype(np.int64), J.astype(np.int64))), shape=(A.nrows, A.ncols))
    B = gb.Matrix.from_csr(A.type, A.nrows, A.ncols, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), X[S.data])
    assert residency(gb, B) == 2
    return B


def hbm_vector(gb, v):
    x, p = v.to_dense_arrays()
    w = gb.Vector.from_dense_array(x, v.type, present=p)
    assert residency(gb, w) == 2
    return w


def strictly_increasing(a):
    return bool(np.all(a[1:] > a[:-1]))


# ---- 1. the parse kernel at its edges ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(gb, gpu):
    """u = 0, 1, 2, ... as a dense INT32 vector one grid round and seven positions long, living in HBM only"""
    per_wg, cap = geometry(gb)
    per_round = per_wg * cap
    dim = per_round + 7
    assert dim == 2 ** 21 + 7 and per_wg == 512, "the parse kernel's geometry changed: look at the edges of this file again"
    uval = np.arange(dim, dtype=np.int32) * 3 - 7
    u = gb.Vector.from_dense_array(uval, gb.INT32)
    assert residency(gb, u) == 2
    return {"dim": dim, "per_round": per_round, "per_wg": per_wg, "u": u, "uval": uval}


def extract_at(gb, u, t, n, out=None):
    w = gb.Vector.sparse(u.type, n) if out is None else out
    info = gb.lib.GrBX_Vector_extract_at(w._h, None, None, u._h, ptr(t), C.c_uint64(n), None, C.c_int(1))
    return info, w


@pytest.mark.parametrize("offset", [0, 1])
def test_parse_kernel_lengths(gb, big, offset):
    rng = np.random.default_rng(10 + offset)
    dim, u, uval = big["dim"], big["u"], big["uval"]
    past_round = big["per_round"] + 5
    assert past_round > big["per_wg"] * geometry(gb)[1], "one length must take the kernel past a grid round"
    for n in [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, past_round]:
        for kind in ("increasing", "shuffled", "repeats"):
            if kind == "increasing":
                L = np.sort(rng.choice(dim, size=n, replace=False)).astype(np.int64)
            elif kind == "shuffled":
                L = rng.permutation(dim)[:n].astype(np.int64)
                if n >= 2 and L[0] < L[1]:
                    L[[0, 1]] = L[[1, 0]]
            else:
                L = rng.integers(0, dim, n).astype(np.int64)
                if n >= 2:
                    L[-1] = L[0]
            what = (n, kind, offset)
            t = dev(L, offset)
            if n == 0:
                t = dev(np.zeros(1), offset)                          # (an empty tensor has no address: n = 0 of a list that has one)
            assert (t.data_ptr() % 16 == 8) == (offset == 1)
            info, w = extract_at(gb, u, t, n)
            assert info == 0, what
            plan = gb.last_kernel_plan()
            assert plan.startswith("extract_vector<index=list@hbm>"), (what, plan)
            if n:
                assert ("k_index_parse<increasing=%d>" % strictly_increasing(L)) in plan, (what, plan)      # no sort / sort downstream hangs on this flag
            assert residency(gb, u) == 2 and (n == 0 or residency(gb, w) == 2), what
            ref = u.extract(L.astype(np.uint64))
            assert "@hbm" not in gb.last_kernel_plan() and "k_index_parse" not in gb.last_kernel_plan()
            same(w, ref, what)
            gi, gx = w.to_arrays()
            assert np.array_equal(gi, np.arange(n, dtype=np.uint64)) and np.array_equal(gx, uval[L]), what


def defect_positions(big, n):
    pw, pr = big["per_wg"], big["per_round"]
    return sorted({1, 2, 63, 64, 65, 127, 128, 129, pw - 1, pw, pw + 1, pr - 1, pr, pr + 1, n - 2, n - 1})


@pytest.mark.parametrize("offset", [0, 1])
def test_one_defect_anywhere_clears_the_increasing_flag(gb, big, offset):
    """an increasing list with ONE equal or descending neighbour pair (k - 1, k): at k = 1, across lanes, waves, workgroups, the grid round, and the last pair"""
    u, uval, dim = big["u"], big["uval"], big["dim"]
    n = big["per_round"] + 5
    base = np.arange(n, dtype=np.int64) + 1                            # (values 1 .. n < dim)
    info, w = extract_at(gb, u, dev(base, offset), n)
    assert info == 0 and "k_index_parse<increasing=1>" in gb.last_kernel_plan()
    for k in defect_positions(big, n):
        for defect in ("equal", "descending"):
            L = base.copy()
            if defect == "equal":
                L[k] = L[k - 1]
            else:
                L[[k - 1, k]] = L[[k, k - 1]]
            info, w = extract_at(gb, u, dev(L, offset), n)
            assert info == 0 and "k_index_parse<increasing=0>" in gb.last_kernel_plan(), (k, defect, offset, gb.last_kernel_plan())
            gi, gx = w.to_arrays()
            assert np.array_equal(gx, uval[L]), (k, defect, offset)


def test_defects_in_a_column_list_sort_the_rows_as_the_host_list_does(gb, big):
    rng = np.random.default_rng(12)
    n = big["per_round"] + 5
    ncols = big["dim"]
    nnz = 3000
    flat = np.sort(rng.choice(4 * ncols, size=nnz, replace=False))
    I, J = np.divmod(flat, ncols)
    S = sp.csr_matrix((np.arange(nnz), (I, J)), shape=(4, ncols))
    A = gb.Matrix.from_csr(gb.INT32, 4, ncols, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), np.arange(nnz, dtype=np.int32))
    base = np.arange(n, dtype=np.int64) + 1
    rowsort = lambda: gb.last_kernel_plan().split("rowsort=")[1][0]
    for k in [None, 1, 64, 128, big["per_wg"], big["per_round"], n - 1]:
        for defect in ("equal", "descending"):
            L = base.copy()
            if k is not None:
                if defect == "equal":
                    L[k] = L[k - 1]
                else:
                    L[[k - 1, k]] = L[[k, k - 1]]
            ref = A.extract_matrix(None, L.astype(np.uint64))
            want = rowsort()
            got = A.extract_matrix(None, dev(L))
            plan = gb.last_kernel_plan()
            assert rowsort() == want == ("0" if k is None else "1") and "columns=list@hbm" in plan and ("k_index_parse<increasing=%d>" % (k is None)) in plan, (k, defect, plan)
            assert residency(gb, A) == 2 and residency(gb, got) == 2
            same(got, ref, (k, defect))                                # (to_arrays is the stored order: the columns inside every row agree)


# ---- 2. bounds ---------------------------------------------------------------------------------------------------------------
def test_one_bad_index_anywhere_is_out_of_bounds_and_writes_nothing(gb, big):
    u, dim = big["u"], big["dim"]
    n = big["per_round"] + 5
    base = np.arange(n, dtype=np.int64)
    wval = np.arange(10, dtype=np.int32) + 100
    w = gb.Vector.from_dense_array(wval, gb.INT32, present=(np.arange(10) % 3 != 0).astype(np.uint8))      # (the wrong size on purpose: out of bounds is reported before a dimension mismatch)
    for offset in (0, 1):
        for k in (0, 64, big["per_round"] - 1, big["per_round"], n - 1):
            for bad in (dim, 2 ** 32, 2 ** 32 + 5, -1):
                L = base.copy()
                L[k] = bad
                info, _ = extract_at(gb, u, dev(L, offset), n, out=w)
                assert info == info_code(gb, "GrB_INDEX_OUT_OF_BOUNDS"), (offset, k, bad, info)
                assert residency(gb, w) == 2 and residency(gb, u) == 2
            L = base.copy()
            L[k] = dim - 1
            info, out = extract_at(gb, u, dev(L, offset), n)
            assert info == 0, (offset, k)
            assert np.array_equal(out.to_arrays()[1], big["uval"][L])
    with pytest.raises(gb.base.IndexOutOfBound):
        L = base.copy()
        L[7] = 2 ** 32
        u.extract(dev(L), out=w)
    assert residency(gb, w) == 2
    gi, gx = w.to_arrays()
    keep = np.arange(10) % 3 != 0
    assert np.array_equal(gi, np.arange(10, dtype=np.uint64)[keep]) and np.array_equal(gx, wval[keep])


# ---- 3. every entry point, against the same call with the list on the host ---------------------------------------------------
NR, NC, NNZ = 300, 400, 3000


def other_side(rng, d, how):
    """the index argument of the side that is not in HBM: (argument, number of positions)"""
    if how == "all":
        return None, d
    if how == "range":
        a, b = sorted(int(x) for x in rng.integers(0, d, 2))
        return slice(a, b), b - a + 1
    L = rng.permutation(d)[: int(rng.integers(1, d + 1))].astype(np.uint64)
    return L, len(L)


def mask_for(rng, gb, kind, shape):
    if kind is None:
        return None
    if len(shape) == 1:
        return random_vector(rng, gb, "BOOL", shape[0], 0.6)
    return random_matrix(rng, gb, "BOOL", shape[0], shape[1], max(1, shape[0] * shape[1] // 12))


def both_ways(gb, call, L, what, marker="@hbm"):
    """call(list) builds its own operands from a seed and returns the written container: once with the numpy list, once with the same list in HBM"""
    ref = call(L.astype(np.uint64))
    got = call(dev(L))
    if len(L):                                                         # (an empty tensor has no address: the Python surface passes the empty host list)
        assert marker in gb.last_kernel_plan() and "k_index_parse" in gb.last_kernel_plan(), (what, gb.last_kernel_plan())
    same(got, ref, what)


@pytest.mark.parametrize("tname", VALUE_TYPES)
def test_vector_extract_and_assign(gb, gpu, tname):
    rng = np.random.default_rng(VALUE_TYPES.index(tname))
    typ = getattr(gb, tname)
    n = NC
    for mk in MASKS:
        for acc in (None, "PLUS"):
            for replace in (False, True):
                accum = getattr(typ, acc) if acc else None
                for kind in EXTRACT_KINDS:
                    L = pick(kind, n, rng)
                    seed = int(rng.integers(1 << 30))

                    def call(lst):
                        r = np.random.default_rng(seed)
                        u, w, M = random_vector(r, gb, tname, n), random_vector(r, gb, tname, len(L)), mask_for(r, gb, mk, (len(L),))
                        return u.extract(lst, out=w, mask=M, accum=accum, desc=descriptor(gb, mk, replace, False))
                    both_ways(gb, call, L, ("extract", tname, mk, acc, replace, kind))
                for kind in ASSIGN_KINDS:
                    L = pick(kind, n, rng)
                    seed = int(rng.integers(1 << 30))

                    def call(lst):
                        r = np.random.default_rng(seed)
                        w, u, M = random_vector(r, gb, tname, n), random_vector(r, gb, tname, len(L)), mask_for(r, gb, mk, (n,))
                        w.assign(u, lst, mask=M, accum=accum, desc=descriptor(gb, mk, replace, False))
                        return w
                    both_ways(gb, call, L, ("assign", tname, mk, acc, replace, kind))


@pytest.mark.parametrize("tname", VALUE_TYPES)
def test_col_and_row_forms(gb, gpu, tname):
    rng = np.random.default_rng(20 + VALUE_TYPES.index(tname))
    typ = getattr(gb, tname)
    for mk in MASKS:
        for acc in (None, "PLUS"):
            accum = getattr(typ, acc) if acc else None
            replace = bool(rng.integers(2))
            for t0 in (False, True):                                   # extract_col / extract_row
                length = NC if t0 else NR
                for kind in EXTRACT_KINDS:
                    L = pick(kind, length, rng)
                    seed, j = int(rng.integers(1 << 30)), int(rng.integers(0, NR if t0 else NC))

                    def call(lst):
                        r = np.random.default_rng(seed)
                        A, w, M = random_matrix(r, gb, tname, NR, NC, NNZ), random_vector(r, gb, tname, len(L)), mask_for(r, gb, mk, (len(L),))
                        return A.extract_col(j, lst, out=w, mask=M, accum=accum, desc=descriptor(gb, mk, replace, t0))
                    both_ways(gb, call, L, ("extract_col", tname, mk, acc, replace, t0, kind))
            for is_row in (False, True):
                length = NC if is_row else NR
                for kind in ASSIGN_KINDS:
                    L = pick(kind, length, rng)
                    seed, fixed = int(rng.integers(1 << 30)), int(rng.integers(0, NR if is_row else NC))

                    def call(lst):
                        r = np.random.default_rng(seed)
                        Cm, u, M = random_matrix(r, gb, tname, NR, NC, NNZ), random_vector(r, gb, tname, len(L)), mask_for(r, gb, mk, (length,))
                        (Cm.assign_row if is_row else Cm.assign_col)(fixed, u, lst, mask=M, accum=accum, desc=descriptor(gb, mk, replace, False))
                        return Cm
                    both_ways(gb, call, L, ("assign_row" if is_row else "assign_col", tname, mk, acc, replace, kind))


@pytest.mark.parametrize("tname", VALUE_TYPES)
def test_matrix_forms(gb, gpu, tname):
    rng = np.random.default_rng(40 + VALUE_TYPES.index(tname))
    typ = getattr(gb, tname)
    case = 0
    for mk in MASKS:
        for acc in (None, "PLUS"):
            accum = getattr(typ, acc) if acc else None
            for kinds, form in ((EXTRACT_KINDS, "extract"), (ASSIGN_KINDS, "assign")):
                for kind in kinds:
                    # every pairing the other side can take opposite a list in HBM, each with and without the transpose; replace alternates out of step with all of them
                    for side, other, t0 in [(sd, o, t) for sd, others in (("rows", OTHERS), ("columns", OTHERS), ("both", ["-"])) for o in others for t in (False, True)]:
                        case += 1
                        replace = (case // 2) % 2 == 1
                        nr, nc = (NC, NR) if (t0 and form == "extract") else (NR, NC)      # op(A)'s shape for extract; C's for assign
                        LI, LJ = pick(kind, nr, rng), pick(kind, nc, rng)
                        oi, noi = other_side(rng, nr, other)
                        oj, noj = other_side(rng, nc, other)
                        ni, nj = (len(LI) if side != "columns" else noi), (len(LJ) if side != "rows" else noj)
                        seed = int(rng.integers(1 << 30))
                        what = (form, tname, mk, acc, kind, side, other, replace, t0)

                        def call(hbm):
                            r = np.random.default_rng(seed)
                            as_arg = (lambda a: dev(a)) if hbm else (lambda a: a.astype(np.uint64))
                            I = as_arg(LI) if side != "columns" else oi
                            J = as_arg(LJ) if side != "rows" else oj
                            if form == "extract":
                                A, Cm, M = random_matrix(r, gb, tname, NR, NC, NNZ), random_matrix(r, gb, tname, ni, nj, min(ni * nj, 500)) if ni * nj else gb.Matrix.sparse(typ, ni, nj), mask_for(r, gb, mk, (ni, nj)) if ni * nj else None
                                if M is None and mk is not None:
                                    M = gb.Matrix.sparse(gb.BOOL, ni, nj)
                                return A.extract_matrix(I, J, out=Cm, mask=M, accum=accum, desc=descriptor(gb, mk, replace, t0))
                            Cm, M = random_matrix(r, gb, tname, NR, NC, NNZ), mask_for(r, gb, mk, (NR, NC))
                            ar, ac = (nj, ni) if t0 else (ni, nj)
                            A = random_matrix(r, gb, tname, ar, ac, min(ar * ac, 800)) if ar * ac else gb.Matrix.sparse(typ, ar, ac)
                            Cm.assign_matrix(A, I, J, mask=M, accum=accum, desc=descriptor(gb, mk, replace, t0))
                            return Cm
                        ref = call(False)
                        got = call(True)
                        plan = gb.last_kernel_plan()
                        if (side != "columns" and len(LI)) or (side != "rows" and len(LJ)):
                            assert "list@hbm" in plan and "k_index_parse" in plan, (what, plan)
                        same(got, ref, what)


# ---- 4. residency ------------------------------------------------------------------------------------------------------------
def test_operands_in_hbm_stay_there(gb, gpu):
    rng = np.random.default_rng(50)
    A = hbm_matrix(gb, random_matrix(rng, gb, "FP64", NR, NC, NNZ))
    u = hbm_vector(gb, random_vector(rng, gb, "FP64", NC))
    I, J = dev(rng.permutation(NR)[:120]), dev(np.sort(rng.choice(NC, 90, replace=False)))
    out = A.extract_matrix(I, J)
    assert "rows=list@hbm,columns=list@hbm" in gb.last_kernel_plan() and residency(gb, A) == 2 and residency(gb, out) == 2
    out = A.extract_col(5, I)
    assert "index=list@hbm" in gb.last_kernel_plan() and residency(gb, A) == 2 and residency(gb, out) == 2
    out = u.extract(J)
    assert "index=list@hbm" in gb.last_kernel_plan() and residency(gb, u) == 2 and residency(gb, out) == 2
    w = hbm_vector(gb, random_vector(rng, gb, "FP64", 90))
    u.assign(w, J)
    assert "assign_vector<index=list@hbm" in gb.last_kernel_plan() and residency(gb, u) == 2 and residency(gb, w) == 2
    B = hbm_matrix(gb, random_matrix(rng, gb, "FP64", 120, 90, 700))
    A.assign_matrix(B, I, J)
    assert "rows=list@hbm,cols=list@hbm" in gb.last_kernel_plan() and residency(gb, A) == 2 and residency(gb, B) == 2
    A.assign_row(7, w, J)
    assert "assign_row<index=list@hbm" in gb.last_kernel_plan() and residency(gb, A) == 2 and residency(gb, w) == 2
    w2 = hbm_vector(gb, random_vector(rng, gb, "FP64", 120))
    A.assign_col(7, w2, I)
    assert "assign_col<index=list@hbm" in gb.last_kernel_plan() and residency(gb, A) == 2 and residency(gb, w2) == 2


# ---- 5. fallbacks and refusals -----------------------------------------------------------------------------------------------
def test_assign_with_a_repeat_takes_the_host_route(gb, gpu):
    rng = np.random.default_rng(60)
    L = rng.permutation(NC)[:50].astype(np.int64)
    L[-1] = L[3]                                                       # named twice: the last occurrence wins on the host route
    seed = 61

    def vec(lst):
        r = np.random.default_rng(seed)
        w, u = random_vector(r, gb, "INT32", NC), random_vector(r, gb, "INT32", 50, 1.0)
        w.assign(u, lst)
        return w
    same(vec(dev(L)), vec(L.astype(np.uint64)), "vector assign with a repeat")
    LI = rng.permutation(NR)[:40].astype(np.int64)
    LI[-1] = LI[0]

    def mat(hbm):
        r = np.random.default_rng(seed)
        Cm, A = random_matrix(r, gb, "INT32", NR, NC, NNZ), random_matrix(r, gb, "INT32", 40, 50, 600)
        Cm.assign_matrix(A, dev(LI) if hbm else LI.astype(np.uint64), dev(L) if hbm else L.astype(np.uint64))
        return Cm
    same(mat(True), mat(False), "matrix assign with a repeat")


def test_vector_list_on_the_host_route_leaves_the_plan_alone(gb, gpu):
    rng = np.random.default_rng(62)
    u = random_vector(rng, gb, "FP64", NC, 1.0)
    iv = gb.Vector.from_arrays(np.arange(6, dtype=np.uint64), np.array([5, 9, 9, 2, 5, 1], np.int32), 6, gb.INT32)      # names 5 and 9 twice
    u.extract(iv)
    before = gb.last_kernel_plan()
    assert "@hbm" in before and "k_index_widen" in before
    src = random_vector(rng, gb, "FP64", 6, 1.0)
    for _ in range(3):                                                 # a repeat: the host route, which writes no plan
        w, w_ref = u.dup(), u.dup()
        w.assign(src, iv)
        assert gb.last_kernel_plan() == before
        w_ref.assign(src, np.array([5, 9, 9, 2, 5, 1], np.uint64))
        same(w, w_ref, "assign through a vector with repeats")


def test_hypersparse_operand_takes_the_host_route(gb, gpu):
    big_n = 1 << 40
    idx = np.array([5, 1 << 33, (1 << 39) + 3], np.uint64)
    u = gb.Vector.from_arrays(idx, np.array([1.5, 2.5, 3.5]), big_n, gb.FP64)
    L = np.array([(1 << 39) + 3, 7, 5, 1 << 33, 5], np.int64)
    ref = u.extract(L.astype(np.uint64))
    got = u.extract(dev(L))
    same(got, ref, "hypersparse extract")
    assert got.nvals == 4


def test_refusals(gb, gpu):
    rng = np.random.default_rng(70)
    u = random_vector(rng, gb, "FP64", NC)
    w = gb.Vector.sparse(gb.FP64, 10)
    t = dev(np.arange(10))
    rc = lambda *a: gb.lib.GrBX_Vector_extract_at(*a)
    assert rc(w._h, None, None, u._h, ptr(t), C.c_uint64(GXB_RANGE), None, C.c_int(1)) == info_code(gb, "GrB_INVALID_VALUE")
    assert rc(w._h, None, None, u._h, None, C.c_uint64(10), None, C.c_int(1)) == info_code(gb, "GrB_NULL_POINTER")
    assert rc(w._h, None, None, u._h, ptr(t), C.c_uint64(10), None, C.c_int(2)) == info_code(gb, "GrB_INVALID_VALUE")
    assert w.nvals == 0
    inc = C.c_int(-1)
    assert gb.lib.GrBX_index_parse(ptr(t), C.c_uint64(10), C.c_uint64(NC), C.byref(inc)) == 0 and inc.value == 1
    assert gb.lib.GrBX_index_parse(ptr(t), C.c_uint64(10), C.c_uint64(9), C.byref(inc)) == info_code(gb, "GrB_INDEX_OUT_OF_BOUNDS")
    assert gb.lib.GrBX_index_parse(ptr(t), C.c_uint64(10), C.c_uint64(1 << 33), C.byref(inc)) == info_code(gb, "GrB_INVALID_VALUE")      # (the order test is 32-bit: no answer beyond the device layout)
    assert w.nvals == 0
    A, Cm = random_matrix(rng, gb, "FP64", NR, NC, NNZ), gb.Matrix.sparse(gb.FP64, 10, 10)
    rm = gb.lib.GrBX_Matrix_extract_at
    assert rm(Cm._h, None, None, A._h, ptr(t), C.c_uint64(10), ptr(t), C.c_uint64(GXB_RANGE - 1), None, C.c_int(1), C.c_int(1)) == info_code(gb, "GrB_INVALID_VALUE")
    assert rm(Cm._h, None, None, A._h, ptr(t), C.c_uint64(10), None, C.c_uint64(10), None, C.c_int(1), C.c_int(1)) == info_code(gb, "GrB_NULL_POINTER")
    host_j = np.arange(10, dtype=np.uint64)
    assert rm(Cm._h, None, None, A._h, ptr(t), C.c_uint64(10), host_j.ctypes.data_as(C.c_void_p), C.c_uint64(10), None, C.c_int(1), C.c_int(0)) == 0
    same(Cm, A.extract_matrix(np.arange(10), np.arange(10)), "device rows, host columns through the C entry point")
    # GrB_ALL with location 1, and location 0 being the GrB_ call
    all_ptr = gb._capi.all_indices()
    w2 = gb.Vector.sparse(gb.FP64, NC)
    assert rc(w2._h, None, None, u._h, all_ptr, C.c_uint64(0), None, C.c_int(1)) == 0
    same(w2, u, "GrB_ALL with location 1")
    w3 = gb.Vector.sparse(gb.FP64, 10)
    assert rc(w3._h, None, None, u._h, host_j.ctypes.data_as(C.c_void_p), C.c_uint64(10), None, C.c_int(0)) == 0
    same(w3, u.extract(host_j), "location 0")
    for bad in ("FP32", "BOOL"):
        iv = random_vector(rng, gb, bad, 20, 1.0)
        with pytest.raises(gb.base.DomainMismatch):
            u.extract(iv)
        with pytest.raises(gb.base.DomainMismatch):
            A.extract_matrix(iv, None)
    out = gb.Vector.from_arrays(np.arange(5, dtype=np.uint64), np.arange(5, dtype=np.int64), 5, gb.INT64)
    src = random_vector(rng, gb, "INT64", NC, 1.0)
    with pytest.raises(gb.base.InvalidValue):
        src.extract(out, out=out)
    with pytest.raises(gb.base.InvalidValue):
        out.assign(src.extract(np.arange(5)), out)


# ---- 6. vectors as index lists -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iname", ["INT64", "INT32", "UINT8", "INT16", "UINT64"])
def test_vector_as_index_list(gb, gpu, iname):
    rng = np.random.default_rng(80)
    n = 200 if iname == "UINT8" else 1000
    u = hbm_vector(gb, random_vector(rng, gb, "FP64", n, 0.7))
    pos = np.sort(rng.choice(n, int(0.3 * n), replace=False)).astype(np.uint64)
    val = rng.permutation(n)[: len(pos)].astype(getattr(gb, iname)._np)          # shuffled values, about 30 % of the positions present
    Ivec = hbm_vector(gb, gb.Vector.from_arrays(pos, val, n, getattr(gb, iname)))
    L = Ivec.to_arrays()[1].astype(np.uint64)
    Ivec = hbm_vector(gb, Ivec)
    got = u.extract(Ivec)
    plan = gb.last_kernel_plan()
    assert "index=list@hbm" in plan and "k_tuples_scatter" in plan and "k_index_parse" in plan and residency(gb, Ivec) == 2 and residency(gb, u) == 2, plan
    assert ("k_index_widen" in plan) == (iname not in ("INT64", "UINT64")), plan
    same(got, u.extract(L), "u(Ivec)")
    same(u[Ivec], got, "u[Ivec]")
    # assign: the values are distinct, so the device route takes it
    w = hbm_vector(gb, random_vector(rng, gb, "FP64", n, 0.5))
    w_ref = hbm_vector(gb, w)
    src = random_vector(rng, gb, "FP64", len(L), 0.8)
    w.assign(src, Ivec)
    assert "assign_vector<index=list@hbm" in gb.last_kernel_plan() and residency(gb, w) == 2
    w_ref.assign(src, L)
    same(w, w_ref, "w(Ivec) = src")
    # matrix: rows by vector, all columns; rows and columns by vector; a vector on one side and a tensor on the other
    A = hbm_matrix(gb, random_matrix(rng, gb, "FP64", n, n, 5 * n))
    got = A.extract_matrix(Ivec, None)
    assert "rows=list@hbm" in gb.last_kernel_plan() and residency(gb, A) == 2 and residency(gb, got) == 2
    same(got, A.extract_matrix(L, None), "A(Ivec, :)")
    same(A.extract_matrix(Ivec, Ivec), A.extract_matrix(L, L), "A(Ivec, Ivec)")
    same(A[Ivec, dev(L[:17])], A.extract_matrix(L, L[:17]), "A[Ivec, tensor]")
    same(A.extract_col(3, Ivec), A.extract_col(3, L), "A(Ivec, 3)")


def test_pointer_jump_and_negative_values(gb, gpu):
    rng = np.random.default_rng(81)
    n = 5000
    fv = rng.integers(0, n, n).astype(np.int64)
    f = gb.Vector.from_dense_array(fv, gb.INT64)
    g = f.extract(f)
    plan = gb.last_kernel_plan()
    assert "index=list@hbm" in plan and "k_tuples" not in plan and "k_index_widen" not in plan, plan      # a full 64-bit vector IS the list
    assert residency(gb, f) == 2 and residency(gb, g) == 2
    gi, gx = g.to_arrays()
    assert np.array_equal(gi, np.arange(n, dtype=np.uint64)) and np.array_equal(gx, fv[fv])
    same(g, f.extract(fv.astype(np.uint64)), "f(f)")
    iv = np.arange(50, dtype=np.int32)
    iv[20] = -3
    with pytest.raises(gb.base.IndexOutOfBound):
        f.extract(gb.Vector.from_dense_array(iv, gb.INT32))
    iv[20] = 3
    assert np.array_equal(f.extract(gb.Vector.from_dense_array(iv, gb.INT32)).to_arrays()[1], fv[iv])


# ---- 7. the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface(gb, gpu):
    import torch
    rng = np.random.default_rng(90)
    A = random_matrix(rng, gb, "FP64", NR, NC, NNZ)
    v = random_vector(rng, gb, "FP64", NC)
    Ih, Jh = rng.permutation(NR)[:60].astype(np.int64), rng.permutation(NC)[:70].astype(np.int64)
    It, Jt = dev(Ih), dev(Jh)
    same(v[Jt], v[Jh.astype(np.uint64)], "v[I_t]")
    assert "@hbm" in gb.last_kernel_plan()
    same(A[It, Jt], A[Ih.astype(np.uint64), Jh.astype(np.uint64)], "A[I_t, J_t]")
    assert "rows=list@hbm,columns=list@hbm" in gb.last_kernel_plan()
    same(A[It, 3], A[Ih.astype(np.uint64), 3], "A[I_t, 3]")
    same(A[3, Jt], A[3, Jh.astype(np.uint64)], "A[3, J_t]")
    u = random_vector(rng, gb, "FP64", 70, 0.9)
    v1, v2 = v.dup(), v.dup()
    v1[Jt] = u
    assert "assign_vector<index=list@hbm" in gb.last_kernel_plan()
    v2[Jh.astype(np.uint64)] = u
    same(v1, v2, "v[I_t] = u")
    B = random_matrix(rng, gb, "FP64", 60, 70, 900)
    A1, A2 = A.dup(), A.dup()
    A1[It, Jt] = B
    assert "assign_matrix<rows=list@hbm" in gb.last_kernel_plan()
    A2[Ih.astype(np.uint64), Jh.astype(np.uint64)] = B
    same(A1, A2, "A[I_t, J_t] = B")
    # a CPU tensor behaves as the list
    same(v[torch.from_numpy(Jh)], v[Jh.astype(np.uint64)], "CPU tensor")
    same(A[torch.from_numpy(Ih), Jt], A[Ih.astype(np.uint64), Jh.astype(np.uint64)], "CPU rows, GPU columns")
    with pytest.raises(TypeError):
        v[Jt.to(torch.float32)]
    with pytest.raises(TypeError):
        A.extract_matrix(It.to(torch.int32), None)
    with pytest.raises(ValueError):
        v[dev(np.arange(40))[::2]]
    with pytest.raises(ValueError):
        v.extract(dev(np.arange(40)).reshape(4, 10))
    for bad in (lambda: v.__setitem__(Jt, 2.0), lambda: A.__setitem__((It, Jt), 2.0), lambda: v.assign_scalar(2.0, Jt)):
        with pytest.raises(TypeError, match="scalar assign"):
            bad()


# ---- 8. round trip: a selected vertex set, never on the host -----------------------------------------------------------------
def test_subgraph_of_a_selected_vertex_set(gb, gpu):
    rng = np.random.default_rng(100)
    n = 2000
    Ah = random_matrix(rng, gb, "FP64", n, n, 12 * n)
    I, J, X = Ah.to_arrays()
    S = sp.csr_matrix((X, (I.astype(np.int64), J.astype(np.int64))), shape=(n, n))
    A = hbm_matrix(gb, Ah)
    wv = rng.standard_normal(n)
    w = gb.Vector.from_dense_array(wv, gb.FP64)
    (It,) = w.select(">", 0.25).to_tensors(values=False)
    assert It.is_cuda and 0 < It.numel() < n
    sub = A.extract_matrix(It, It)
    plan = gb.last_kernel_plan()
    assert "rows=list@hbm,columns=list@hbm" in plan and "k_index_parse<increasing=1> k_index_parse<increasing=1>" in plan and "rowsort=0" in plan, plan
    assert residency(gb, A) == 2 and residency(gb, sub) == 2
    keep = np.flatnonzero(wv > 0.25)
    assert np.array_equal(It.cpu().numpy(), keep)
    want = S[keep][:, keep].tocsr()
    want.sort_indices()
    wc = want.tocoo()
    gi, gj, gx = sub.to_arrays()
    assert np.array_equal(gi, wc.row.astype(np.uint64)) and np.array_equal(gj, wc.col.astype(np.uint64)) and np.array_equal(bits(gx), bits(wc.data))
