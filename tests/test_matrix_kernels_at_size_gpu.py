"""The entry-parallel O(nnz) matrix kernels (grb_matops.hip, grb_transpose.hip and the rocPRIM scan / merge / sort wrappers of grb_prims.hip) against the
vectorised numpy model of tests/matrix_model.py, at the smallest sizes where their block structure matters — 3e4 to 1.2e5 entries: more than a hundred
256-thread workgroups and several rocPRIM tiles — and for every value width (1, 2, 4 and 8 bytes, signed and unsigned).

Every comparison is on `to_csr()`: row pointers, columns and values, bit-exact (one exception: FP64 POW, a math-library operator, with the bound of
test_math_library_operators), and the columns must ascend strictly inside each row.  Values follow helpers.rand_values (small integers, floating point on
the 1/8 grid: exact in any order), with entries at the type's extremes for the operators that wrap.

The shapes (entries / 256-thread workgroups; all off the few-long-rows and batch routes: nrows > 64 or ncols < 65536):
  uniform    3000 x 2000, 60 000 entries (235 workgroups, 60 000 % 256 = 96)
  ragged     70 x 60 000: rows of 0, 1, 15, 16, 17, 0, 0, 256, 257, 50 000, 0, 1 entries, random short rows, first and last row empty
  tall       20 000 x 37: the first and last 300 rows and half of the others empty; columns 0-2, 17-21 and 34-36 empty
  mult256    500 x 700 with 256 * 137 entries exactly, and with one more
  pow2       200 x 4096 and 200 x 4097, entries in column 0 and in the last column
  square     1024 x 1024 (the in-place transpose)
  thin       1 x 5000 full, 5000 x 1 full, 300 x 300 with the single entry (299, 299)"""
import functools
import itertools

import numpy as np
import pytest

import matrix_model as MM
import pygraphblas_amd as gb
from pygraphblas_amd import descriptor as D
from helpers import TYPE, rand_values

pytestmark = pytest.mark.gpu

TYPES = ["BOOL", "INT8", "UINT16", "INT32", "FP32", "INT64", "UINT64", "FP64"]
WIDTHS = ["INT8", "UINT16", "FP32", "INT64"]                 # one type per value width
MASK_TYPES = ["BOOL", "INT8", "UINT16", "FP32", "INT64", "FP64"]
NP = MM.NP


# ---- patterns: (nrows, ncols, ascending int64 keys), built once -------------------------------------------------------------------------------------------
def _random_keys(rng, nr, nc, n):
    return np.sort(rng.choice(nr * nc, size=n, replace=False)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def pattern(name, variant=0):
    """The pattern of shape `name`; `variant` > 0 gives an independent second pattern of the same shape and construction."""
    rng = np.random.default_rng(1000 * variant + sum(map(ord, name)))
    if name == "uniform":
        nr, nc = 3000, 2000; n = int(nr * nc * 0.01)
        if n % 256 == 0: n += 1
        keys = _random_keys(rng, nr, nc, n)
    elif name == "ragged":
        nr, nc = 70, 60000
        lens = [0, 1, 15, 16, 17, 0, 0, 256, 257, 50000, 0, 1] + [int(x) for x in rng.integers(0, 300, 57)] + [0]
        lens[12 + 20] = 0; lens[12 + 21] = 0                                        # a run of empty rows among the short ones too
        assert len(lens) == nr and lens[0] == 0 and lens[-1] == 0
        keys = np.concatenate([r * nc + np.sort(rng.choice(nc, size=k, replace=False)) for r, k in enumerate(lens)]).astype(np.int64)
    elif name == "tall":
        nr, nc = 20000, 37
        cols = np.array([c for c in range(nc) if not (c <= 2 or 17 <= c <= 21 or c >= 34)])
        rows = np.arange(300, nr - 300); rows = rows[rng.random(len(rows)) < 0.5]
        keys = np.concatenate([r * nc + np.sort(rng.choice(cols, size=int(k), replace=False)) for r, k in zip(rows, rng.integers(1, 9, len(rows)))]).astype(np.int64)
    elif name in ("mult256", "mult256p1"):
        nr, nc = 500, 700; keys = _random_keys(rng, nr, nc, 256 * 137 + (name == "mult256p1"))
    elif name in ("pow2", "pow2p1"):
        nr, nc = 200, 4096 + (name == "pow2p1")
        inner = _random_keys(rng, nr, nc - 2, 32000)                                # columns 1 .. nc-2
        inner = (inner // (nc - 2)) * nc + inner % (nc - 2) + 1
        edge_rows = np.arange(0, nr, 3)
        keys = np.unique(np.concatenate([inner, edge_rows * nc, edge_rows * nc + nc - 1, [(nr - 1) * nc + nc - 1]])).astype(np.int64)
    elif name == "square":
        nr, nc = 1024, 1024; keys = _random_keys(rng, nr, nc, 31001)
    elif name == "row":
        nr, nc = 1, 5000; keys = np.arange(5000, dtype=np.int64)
    elif name == "col":
        nr, nc = 5000, 1; keys = np.arange(5000, dtype=np.int64)
    elif name == "single":
        nr, nc = 300, 300; keys = np.array([299 * 300 + 299], np.int64)
    else:
        raise ValueError(name)
    return nr, nc, keys


BIG = ["uniform", "ragged", "tall", "mult256", "mult256p1", "pow2", "pow2p1"]
ALL_SHAPES = BIG + ["square", "row", "col", "single"]


def test_the_shapes_are_what_the_kernels_need(gpu):
    """The sizes this file rests on: every large shape spans more than a hundred 256-thread workgroups and stays off the few-long-rows and batch routes."""
    for name in BIG:
        nr, nc, keys = pattern(name)
        assert 3e4 <= len(keys) <= 1.2e5 and len(keys) // 256 > 100 and (nr > 64 or (nc < 65536 and len(keys) < 1 << 18)), (name, len(keys))
    assert len(pattern("uniform")[2]) % 256 != 0 and len(pattern("mult256")[2]) % 256 == 0 and len(pattern("mult256p1")[2]) % 256 == 1
    nr, nc, keys = pattern("ragged"); lens = np.bincount(keys // nc, minlength=nr)
    assert lens[:12].tolist() == [0, 1, 15, 16, 17, 0, 0, 256, 257, 50000, 0, 1] and lens[-1] == 0
    nr, nc, keys = pattern("tall"); used = np.unique(keys % nc); rows = keys // nc
    assert set(used.tolist()) == set(range(3, 17)) | set(range(22, 34)) and rows.min() >= 300 and rows.max() < nr - 300
    for name in ("pow2", "pow2p1"):
        nr, nc, keys = pattern(name); assert (keys % nc == 0).any() and (keys % nc == nc - 1).any() and nc in (4096, 4097)


# ---- values -------------------------------------------------------------------------------------------------------------------------------------------------
def extremes(typ):
    if typ == "BOOL": return np.array([True, False])
    if typ.startswith("FP"):
        f = np.finfo(NP[typ]); return np.array([f.max, -f.max], NP[typ])
    i = np.iinfo(NP[typ]); return np.array([i.min, i.max, i.min + 1, i.max - 1], NP[typ])


def values(rng, typ, n, extreme=False):
    """helpers.rand_values; `extreme`: one entry in 64 at the type's extremes, so that PLUS / MINUS / TIMES wrap (integers) or overflow (floating point)."""
    x = rand_values(rng, typ, n)
    if extreme and n:
        at = rng.random(n) < 1 / 64
        x[at] = rng.choice(extremes(typ), size=int(at.sum()))
    return x


def mat(name, typ, seed=0, variant=0, extreme=False):
    nr, nc, keys = pattern(name, variant)
    return MM.Mat(nr, nc, keys, values(np.random.default_rng([seed, variant, TYPES.index(typ) if typ in TYPES else 99]), typ, len(keys), extreme))


def sub(m, keep):
    return MM.Mat(m.nrows, m.ncols, m.keys[keep], m.vals[keep])


def mask_values(rng, typ, n):
    """About a third of the stored mask values are false; the floating-point ones among them are 0.0 and -0.0, and NaN is among the true ones."""
    if typ == "BOOL": return rng.random(n) < 2 / 3
    if typ.startswith("FP"): return rng.choice(np.array([0.0, -0.0, np.nan, 1.5, -2.0, 0.125], NP[typ]), size=n)
    return rng.choice(np.array([0, 1, 3 if typ[0] == "U" else -3], NP[typ]), size=n)


def mask_over(rng, mtyp, *mats, extra=10000):
    """A mask of type `mtyp` over half of the positions the given matrices hold and `extra` positions none of them may hold."""
    nr, nc = mats[0].nrows, mats[0].ncols
    held = functools.reduce(np.union1d, [m.keys for m in mats])
    keys = np.union1d(held[rng.random(len(held)) < 0.5], rng.integers(0, nr * nc, extra))
    return MM.Mat(nr, nc, keys, mask_values(rng, mtyp, len(keys)))


# ---- the library side ------------------------------------------------------------------------------------------------------------------------------------------
def dev(m):
    T = TYPE[m.typ]
    if m.nvals == 0:
        return gb.Matrix.sparse(T, m.nrows, m.ncols)
    return gb.Matrix.from_arrays(m.rows.astype(np.uint64), m.cols.astype(np.uint64), m.vals, m.nrows, m.ncols, T)


def dev_vec(m):
    T = TYPE[m.typ]
    return gb.Vector.from_arrays(m.keys.astype(np.uint64), m.vals, m.nrows, T) if m.nvals else gb.Vector.sparse(T, m.nrows)


def new(typ, nr, nc):
    return gb.Matrix.sparse(TYPE[typ], nr, nc)


def same_bits(got, exp):
    """Element-wise: the same bits, or both NaN."""
    if got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        return (got.view(u) == exp.view(u)) | (np.isnan(got) & np.isnan(exp))
    return got == exp


def check(M, exp, what):
    assert M.type.__name__ == exp.typ and (M.nrows, M.ncols) == (exp.nrows, exp.ncols), (what, M, exp.typ, exp.nrows, exp.ncols)
    rp, ci, x = M.to_csr(); erp, eci, ex = MM.to_csr(exp)
    assert M.nvals == exp.nvals, f"{what}: {M.nvals} entries, expected {exp.nvals}"
    if not np.array_equal(rp, erp):
        r = int(np.flatnonzero(rp != erp)[0]); raise AssertionError(f"{what}: row pointers differ first at row {r}: {rp[r:r + 4]} vs {erp[r:r + 4]}")
    if len(ci) > 1:
        inside = np.ones(len(ci), bool); starts = rp[:-1][rp[:-1] < len(ci)]; inside[starts] = False          # (positions that do not start a row)
        up = ci[1:].astype(np.int64) > ci[:-1].astype(np.int64)
        assert np.all(up[inside[1:]]), f"{what}: columns do not ascend inside a row, first at entry {int(np.flatnonzero(~up & inside[1:])[0]) + 1}"
    if not np.array_equal(ci, eci):
        p = int(np.flatnonzero(ci != eci)[0]); raise AssertionError(f"{what}: columns differ first at entry {p}: {ci[p:p + 4]} vs {eci[p:p + 4]}")
    assert x.dtype == ex.dtype, what
    ok = same_bits(x, ex)
    if not ok.all():
        p = np.flatnonzero(~ok); raise AssertionError(f"{what}: {len(p)} values differ, first at entries {p[:4].tolist()}: got {x[p[:4]]} expected {ex[p[:4]]}")


def check_vec(w, exp, what):
    """A vector against the model's nrows x 1 matrix."""
    assert w.type.__name__ == exp.typ and w.size == exp.nrows, what
    I, X = w.to_arrays(); o = np.argsort(I, kind="stable"); I, X = I[o], X[o]
    assert np.array_equal(I.astype(np.int64), exp.keys), f"{what}: pattern differs ({len(I)} entries, expected {exp.nvals})"
    ok = same_bits(X, exp.vals)
    if not ok.all():
        p = np.flatnonzero(~ok); raise AssertionError(f"{what}: {len(p)} values differ, first at indices {I[p[:4]].tolist()}: got {X[p[:4]]} expected {exp.vals[p[:4]]}")


@pytest.fixture(scope="module", autouse=True)
def fresh_plan(gpu):
    """A small product first: GrB_mxm starts its plan string afresh, so a route named by an earlier test file cannot be mistaken for one taken here."""
    e = gb.Matrix.from_lists([0], [0], [1], 2, 2, gb.INT64); e.mxm(e, semiring=gb.INT64.PLUS_TIMES)
    assert_generic_route()


def assert_generic_route():
    plan = gb.last_kernel_plan()
    assert not any(s in plan for s in ("ewise_rows<", "ewise_batch<", "mxm_rows<")), plan


def desc_of(replace=False, struct=False, comp=False, t0=False, t1=False):
    name = ("R" if replace else "") + ("S" if struct else "") + ("C" if comp else "") + ("T0" if t0 else "") + ("T1" if t1 else "")
    return getattr(D, name) if name else None


# ---- transpose -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_transpose(gpu, typ):
    """GrB_transpose, the cached transpose behind desc T0, and the transpose of the transpose: every type on `tall` and `ragged` (empty leading, interior and
    trailing columns: the three loops of the row pointers), every shape for INT8 and FP64."""
    T = TYPE[typ]
    for name in (ALL_SHAPES if typ in ("INT8", "FP64") else ["tall", "ragged"]):
        A = mat(name, typ, seed=1); At = MM.transpose(A)
        a = dev(A)
        check(a.transpose(), At, f"transpose {name} {typ}")
        b = dev(A)                                                               # (a fresh handle: the transpose is built for the descriptor)
        check(b.apply(T.IDENTITY, out=new(typ, A.ncols, A.nrows), desc=D.T0), At, f"apply(IDENTITY, T0) {name} {typ}")
        check(b.apply(T.IDENTITY, out=new(typ, A.ncols, A.nrows), desc=D.T0), At, f"apply(IDENTITY, T0) from the cache {name} {typ}")
        check(a.T.T, A, f"A.T.T {name} {typ}")
        check(a.transpose(desc=D.T0), A, f"transpose(T0) {name} {typ}")


# ---- eWiseAdd / eWiseMult ------------------------------------------------------------------------------------------------------------------------------------
def ewise_ops(typ):
    if typ == "BOOL": return ["LOR", "LAND", "LXOR", "FIRST", "SECOND"]
    return ["PLUS", "TIMES", "MIN", "FIRST", "SECOND", "MINUS"]


def operand_pairs(name, typ):
    """(label, A, B): two independent patterns, the same pattern, B a strict subset of A, disjoint patterns, one operand empty, both empty."""
    A = mat(name, typ, seed=2, extreme=True); B = mat(name, typ, seed=3, variant=1, extreme=True)
    rng = np.random.default_rng(5)
    S = MM.Mat(A.nrows, A.ncols, A.keys, values(rng, typ, A.nvals, True))
    E = MM.empty(A.nrows, A.ncols, typ)
    yield "independent", A, B
    yield "same pattern", A, S
    yield "B a strict subset of A", A, sub(S, rng.random(A.nvals) < 0.5)
    yield "disjoint", A, sub(B, ~np.isin(B.keys, A.keys))
    yield "B empty", A, E
    yield "A empty", E, B
    yield "both empty", E, E


@pytest.mark.parametrize("typ", TYPES)
def test_ewise_add_and_mult(gpu, typ):
    """Union and intersection through the one stable merge: every operand pairing on `uniform`, the hub row and its neighbours on `ragged`, a merged length
    that is a multiple of 256 on `mult256`.  PLUS / TIMES / MINUS wrap at the extremes; FIRST / SECOND / MINUS / DIV tell which operand is which — in the
    independent patterns B's entry precedes A's in the merge as often as not."""
    T = TYPE[typ]
    for name in ("uniform", "ragged", "mult256"):
        for label, A, B in operand_pairs(name, typ):
            if name != "uniform" and label not in ("independent", "same pattern", "B a strict subset of A"):
                continue
            a, b = dev(A), dev(B)
            for op in ewise_ops(typ) if name == "uniform" else ewise_ops(typ)[-2:] + ewise_ops(typ)[:1]:
                for union in (True, False):
                    got = (a.eadd if union else a.emult)(b, getattr(T, op))
                    check(got, MM.ewise(op, typ, A, B, union), f"{'eadd' if union else 'emult'} {op} {typ} {name}: {label}")
            assert_generic_route()
            if "INT" in typ and label in ("independent", "same pattern"):            # integer DIV: no zero divisors, no INT_MIN numerator
                lo = np.iinfo(NP[typ]).min
                A2 = MM.Mat(A.nrows, A.ncols, A.keys, np.where(A.vals == lo, NP[typ](7), A.vals)); B2 = MM.Mat(B.nrows, B.ncols, B.keys, np.where(B.vals == 0, NP[typ](3), B.vals))
                a2, b2 = dev(A2), dev(B2)
                for union in (True, False):
                    check((a2.eadd if union else a2.emult)(b2, T.DIV), MM.ewise("DIV", typ, A2, B2, union), f"{'eadd' if union else 'emult'} DIV {typ} {name}: {label}")


@pytest.mark.parametrize("typ", WIDTHS)
def test_ewise_with_transposed_operands(gpu, typ):
    """desc T0, T1 and T0T1 on `uniform` and on `tall` against its transpose, with an operator that tells the operands apart."""
    T = TYPE[typ]
    for name in ("uniform", "tall"):
        P = mat(name, typ, seed=4); Q = mat(name, typ, seed=5, variant=1)
        Pt, Qt = MM.transpose(P), MM.transpose(Q)
        p, q, pt, qt = dev(P), dev(Q), dev(Pt), dev(Qt)
        for union in (True, False):
            exp = MM.ewise("MINUS", typ, P, Q, union)
            for label, x, y, d in (("T0", pt, q, D.T0), ("T1", p, qt, D.T1), ("T0T1", pt, qt, D.T0T1)):
                got = (x.eadd if union else x.emult)(y, T.MINUS, out=new(typ, P.nrows, P.ncols), desc=d)
                check(got, exp, f"{'eadd' if union else 'emult'} MINUS {label} {typ} {name}")
    assert_generic_route()


def test_ewise_pow_through_the_math_library_kernel(gpu):
    """FP64 POW on `uniform`: the MATH = true instantiation of the fill kernel.  Operand ranges and bound of test_math_library_operators (bases in [0.5, 2.5],
    exponents in [0, 0.5], rtol = 1e-12 against np.power) — the one comparison here that is not bit-exact; pattern and passed-through entries are."""
    rng = np.random.default_rng(9)
    nr, nc, ka = pattern("uniform"); _, _, kb0 = pattern("uniform", 1)
    kb = np.union1d(kb0[::2], ka[::3])                                             # a third of A's entries meet one of B's
    A = MM.Mat(nr, nc, ka, 0.5 + 2.0 * rng.random(len(ka))); B = MM.Mat(nr, nc, kb, 0.5 * rng.random(len(kb)))
    a, b = dev(A), dev(B)
    for union in (True, False):
        got = (a.eadd if union else a.emult)(b, gb.FP64.POW)
        exp = MM.ewise("POW", "FP64", A, B, union)
        rp, ci, x = got.to_csr(); erp, eci, ex = MM.to_csr(exp)
        assert np.array_equal(rp, erp) and np.array_equal(ci, eci), union
        both = np.isin(exp.keys, np.intersect1d(ka, kb))
        assert both.sum() >= len(ka) // 3 and np.allclose(x[both], ex[both], rtol=1e-12, atol=0.0), union
        assert np.array_equal(x[~both], ex[~both]), union
        check(got, MM.Mat(nr, nc, exp.keys, x), "pattern and order of POW")


# ---- select ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,typ", [("uniform", "INT8"), ("ragged", "FP64"), ("tall", "UINT16"), ("pow2p1", "INT32")])
def test_select_by_position(gpu, name, typ):
    A = mat(name, typ, seed=6); a = dev(A)
    for k in (0, 1, -1, A.ncols - 1, -(A.nrows - 1), A.ncols + 5, -(A.nrows + 5)):
        for sel in ("TRIL", "TRIU", "DIAG", "OFFDIAG"):
            check(a.select(sel, k), MM.select(sel, k, A), f"select {sel} k={k} {name} {typ}")
    check(a.tril(), MM.select("TRIL", None, A), f"tril() {name}")


def special_operand(name, typ, seed):
    """The operand of the value selects: rand_values, and for floating point NaN, +-inf and both zeros, for the unsigned types values above the signed range."""
    A = mat(name, typ, seed=seed); x = A.vals.copy(); rng = np.random.default_rng(seed + 100)
    at = rng.random(len(x)) < 0.02
    if typ.startswith("FP"):
        x[at] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], NP[typ]), size=int(at.sum()))
    elif typ[0] == "U":
        top = int(np.iinfo(NP[typ]).max); x[at] = rng.choice(np.array([top // 2 + 6, top, top - 1], NP[typ]), size=int(at.sum()))
    return MM.Mat(A.nrows, A.ncols, A.keys, x)


@pytest.mark.parametrize("typ", TYPES)
def test_select_by_value(gpu, typ):
    """NONZERO / EQ_ZERO / GT_ZERO and the six thunk comparisons through the flag scan and the compaction of every value width, on the hub rows of `ragged`
    and on an entry count that is a multiple of 256: a thunk that occurs among the values and one that does not; NaN, infinities and both zeros for floating
    point; a thunk above the signed range for the unsigned types."""
    for name in ("ragged", "mult256"):
        A = special_operand(name, typ, 7); a = dev(A)
        if typ == "BOOL": thunks = [True, False]
        elif typ.startswith("FP"): thunks = [float(A.vals[np.isfinite(A.vals)][5]), 0.3, np.inf, -0.0]
        elif typ[0] == "U": top = int(np.iinfo(NP[typ]).max); thunks = [int(A.vals[5]), 77, top // 2 + 6, top // 2 + 7]
        else: thunks = [int(A.vals[5]), 77, -3]
        assert (A.vals == NP[typ](thunks[0])).any() and (typ == "BOOL" or not (A.vals == NP[typ](thunks[1])).any())
        for sel in ("NONZERO", "EQ_ZERO", "GT_ZERO"):
            check(a.select(sel), MM.select(sel, None, A), f"select {sel} {typ} {name}")
        for sel in ("GT_THUNK", "GE_THUNK", "LT_THUNK", "LE_THUNK", "EQ_THUNK", "NE_THUNK"):
            for t in thunks:
                check(a.select(sel, t), MM.select(sel, t, A), f"select {sel} thunk={t!r} {typ} {name}")
    if typ == "BOOL":                                                            # a thunk that does not occur: false among all-true values
        A = mat("mult256p1", "BOOL", seed=8); A = MM.Mat(A.nrows, A.ncols, A.keys, np.ones(A.nvals, np.bool_)); a = dev(A)
        for sel in ("EQ_THUNK", "NE_THUNK", "GT_THUNK", "LE_THUNK"):
            check(a.select(sel, False), MM.select(sel, False, A), f"select {sel} thunk=False on all-true BOOL")


@pytest.mark.parametrize("typ", WIDTHS)
def test_select_keeps_everything_and_nothing(gpu, typ):
    lowest = -np.inf if typ.startswith("FP") else int(np.iinfo(NP[typ]).min)
    for name in ("uniform", "mult256"):
        A = mat(name, typ, seed=9); a = dev(A)
        everything = a.select("GE_THUNK", lowest); nothing = a.select("LT_THUNK", lowest)
        assert everything.nvals == A.nvals and nothing.nvals == 0
        check(everything, A, f"select that keeps everything {typ} {name}")
        check(nothing, MM.empty(A.nrows, A.ncols, typ), f"select that keeps nothing {typ} {name}")
        check(a.select("OFFDIAG", A.ncols + 1), A, f"positional select that keeps everything {typ} {name}")
        check(a.select("DIAG", A.ncols + 1), MM.empty(A.nrows, A.ncols, typ), f"positional select that keeps nothing {typ} {name}")


# ---- apply, apply with a bound scalar ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_apply_and_bound_scalar(gpu, typ):
    T = TYPE[typ]; s = True if typ == "BOOL" else 5
    for name in ("ragged", "mult256"):
        A = mat(name, typ, seed=10, extreme=typ not in ("BOOL",)); a = dev(A)
        if "INT" in typ and typ[0] == "I":                                        # (-INT_MIN is not a value of the type: keep it out of AINV / ABS)
            A = MM.Mat(A.nrows, A.ncols, A.keys, np.where(A.vals == np.iinfo(NP[typ]).min, NP[typ](-7), A.vals)); a = dev(A)
        for op in ("AINV", "ABS"):
            check(a.apply(getattr(T, op)), MM.apply(op, typ, A), f"apply {op} {typ} {name}")
        check(a.apply_first(s, T.MINUS), MM.bind1st("MINUS", typ, s, A), f"apply_first MINUS {typ} {name}")
        check(a.apply_second(T.MINUS, s), MM.bind2nd("MINUS", typ, A, s), f"apply_second MINUS {typ} {name}")


# ---- reduce to a vector -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_reduce_vector(gpu, typ):
    """The 16-lane row reduction on `ragged` (rows of 0, 1, 15, 16, 17, 256, 257 and 50 000 entries) and, under T0, on its transpose (60 000 rows of at most 70):
    once plain, once with a valued mask, an accumulator and replace into a non-empty vector.  TIMES folds operands from {1, -1, 2} (2 is rare): exact."""
    T = TYPE[typ]; rng = np.random.default_rng(11)
    A = mat("ragged", typ, seed=11)
    P = MM.Mat(A.nrows, A.ncols, A.keys, rng.choice(np.array([1, 1, 1, 1, -1 if typ[0] != "U" else 1, -1 if typ[0] != "U" else 1], NP[typ]), size=A.nvals)) if typ != "BOOL" else A
    if typ != "BOOL":
        P.vals[rng.random(A.nvals) < 0.001] = 2
    a, p = dev(A), dev(P)
    monoids = ["LOR", "LAND", "LXOR"] if typ == "BOOL" else ["PLUS", "MIN", "MAX", "TIMES"]
    acc = "LOR" if typ == "BOOL" else "PLUS"
    for t0 in (False, True):
        n = A.ncols if t0 else A.nrows
        wk = np.flatnonzero(rng.random(n) < 0.5); W = MM.Mat(n, 1, wk, values(rng, typ, len(wk)))
        mk = np.flatnonzero(rng.random(n) < 0.6); M = MM.Mat(n, 1, mk, mask_values(rng, "INT8", len(mk)))
        for mon in monoids:
            S, s = (P, p) if mon == "TIMES" else (A, a)
            Tm = MM.reduce_rows(mon, typ, MM.transpose(S) if t0 else S)
            got = s.reduce_vector(getattr(T, mon + "_MONOID"), out=gb.Vector.sparse(T, n), desc=D.T0 if t0 else None)
            check_vec(got, Tm, f"reduce_vector {mon} {typ} t0={t0}")
            w = dev_vec(W)
            s.reduce_vector(getattr(T, mon + "_MONOID"), out=w, mask=dev_vec(M), accum=getattr(T, acc), desc=desc_of(replace=True, t0=t0))
            check_vec(w, MM.write_back(W, Tm, M, False, False, True, (acc, typ)), f"reduce_vector {mon} {typ} t0={t0} masked, accumulated, replace")


# ---- the write-back ----------------------------------------------------------------------------------------------------------------------------------------------
MASKS = ["none", "valued", "structural"]
ACCUMS = [None, "PLUS", "SECOND", "MIN"]
FULL = list(itertools.product([True, False], MASKS, [False, True], [False, True], ACCUMS))          # (C empty, mask, complemented, replace, accumulator): 96
EIGHT = [(False, "valued", False, False, "PLUS"), (False, "valued", True, False, None), (False, "structural", False, True, "MIN"), (False, "structural", True, True, "SECOND"),
         (True, "valued", True, False, "PLUS"), (False, "none", False, False, "MIN"), (False, "valued", False, True, None), (False, "none", True, True, "PLUS")]


def run_write_back(typ, name, combos, mask_types, what):
    """C<M, replace> = accum(C, B) through `B.apply(IDENTITY, out=C, ...)`: the write-back is all that varies."""
    T = TYPE[typ]; rng = np.random.default_rng(12)
    B = mat(name, typ, seed=12, extreme=True); C0 = mat(name, typ, seed=13, variant=1, extreme=True)
    C0 = MM.Mat(C0.nrows, C0.ncols, np.union1d(C0.keys, B.keys[::3]), values(rng, typ, len(np.union1d(C0.keys, B.keys[::3])), True))      # a third of B's entries meet one of C's
    masks = {mt: mask_over(rng, mt, B, C0) for mt in mask_types}
    b, c0 = dev(B), dev(C0); dmasks = {mt: dev(m) for mt, m in masks.items()}
    E = MM.empty(B.nrows, B.ncols, typ)
    for n, (cempty, mk, comp, replace, acc) in enumerate(combos):
        mt = mask_types[n % len(mask_types)]
        C = E if cempty else C0; c = new(typ, B.nrows, B.ncols) if cempty else c0.dup()
        M, m = (None, None) if mk == "none" else (masks[mt], dmasks[mt])
        if typ == "BOOL": acc = {"PLUS": "LOR", "MIN": "LAND"}.get(acc, acc)
        b.apply(T.IDENTITY, out=c, mask=m, accum=getattr(T, acc) if acc else None, desc=desc_of(replace, mk == "structural", comp))
        exp = MM.write_back(C, B, M, mk == "structural", comp, replace, (acc, typ) if acc else None)
        check(c, exp, f"{what} {typ} {name}: C {'empty' if cempty else 'non-empty'}, mask {mk} ({mt}), complemented={comp}, replace={replace}, accum={acc}")
    assert_generic_route()


@pytest.mark.parametrize("typ", TYPES)
def test_write_back(gpu, typ):
    """The full product of (C empty or not) x (no / valued / structural mask) x complemented x replace x (no accumulator, PLUS, SECOND, MIN) for INT64 and INT8,
    a fixed eight of them for every other type; the mask's type goes round BOOL, INT8, UINT16, FP32, INT64, FP64 — stored zeros, -0.0 and NaN in each."""
    run_write_back(typ, "uniform", FULL if typ in ("INT64", "INT8") else EIGHT, MASK_TYPES, "write-back")


@pytest.mark.parametrize("mtyp", MASK_TYPES)
def test_write_back_under_every_mask_type(gpu, mtyp):
    """A valued mask of each type — about a third of its stored values zero, the floating-point ones with -0.0 (false) and NaN (true) — plain and complemented,
    with and without replace and an accumulator, on the hub rows of `ragged` (every entry searches its row of the mask)."""
    combos = [(ce, "valued", comp, rep, acc) for ce in (False, True) for comp in (False, True) for rep in (False, True) for acc in (None, "PLUS")]
    run_write_back("INT32", "ragged", combos, [mtyp], "valued mask")
    if mtyp.startswith("FP"):                                                    # every stored mask value one of 0.0, -0.0, NaN: the mask is exactly its NaNs
        B = mat("uniform", "INT8", seed=14); rng = np.random.default_rng(14)
        M = MM.Mat(B.nrows, B.ncols, B.keys, rng.choice(np.array([0.0, -0.0, np.nan], NP[mtyp]), size=B.nvals))
        for comp in (False, True):
            c = new("INT8", B.nrows, B.ncols)
            dev(B).apply(gb.INT8.IDENTITY, out=c, mask=dev(M), desc=desc_of(comp=comp))
            check(c, sub(B, np.isnan(M.vals) != comp), f"mask of zeros, negative zeros and NaNs ({mtyp}), complemented={comp}")


@pytest.mark.parametrize("typ", ["INT8", "FP32", "INT64"])
def test_aliased_mask_and_output(gpu, typ):
    """The output may be any input: C<C> = ..., the mask is A, A = A + A, and the transpose in place on a square shape."""
    T = TYPE[typ]
    A = mat("uniform", typ, seed=15); B = mat("uniform", typ, seed=16, variant=1)
    B = MM.Mat(B.nrows, B.ncols, np.union1d(B.keys, A.keys[::2]), values(np.random.default_rng(16), typ, len(np.union1d(B.keys, A.keys[::2]))))
    assert (A.vals == 0).any() and (A.vals != 0).any()
    b = dev(B)
    for comp, replace, acc in ((False, False, None), (True, False, "PLUS"), (False, True, "PLUS"), (True, True, None)):
        c = dev(A)                                                               # C<C> = accum(C, B): the mask is the output
        b.apply(T.IDENTITY, out=c, mask=c, accum=getattr(T, acc) if acc else None, desc=desc_of(replace, False, comp))
        check(c, MM.write_back(A, B, A, False, comp, replace, (acc, typ) if acc else None), f"C<C> complemented={comp} replace={replace} accum={acc} {typ}")
        a = dev(A); c = dev(B)                                                   # the mask is the operand
        a.apply(T.AINV, out=c, mask=a, accum=getattr(T, acc) if acc else None, desc=desc_of(replace, False, comp))
        check(c, MM.write_back(B, MM.apply("AINV", typ, A), A, False, comp, replace, (acc, typ) if acc else None), f"mask is A complemented={comp} replace={replace} accum={acc} {typ}")
        check(a, A, "the operand that was also the mask is unchanged")
    a = dev(A); a.eadd(b, T.MINUS, out=a, mask=a, desc=D.C)                       # operand, mask and output at once
    check(a, MM.write_back(A, MM.ewise("MINUS", typ, A, B, True), A, False, True, False, None), f"A<!A> = A - B {typ}")
    a = dev(A); a.eadd(a, T.PLUS, out=a)
    check(a, MM.ewise("PLUS", typ, A, A, True), f"A = A + A {typ}")
    a = dev(A); a.emult(a, T.MINUS, out=a)
    check(a, MM.ewise("MINUS", typ, A, A, False), f"A = A - A {typ}")
    S = mat("square", typ, seed=17); s = dev(S)
    s.transpose(out=s)
    check(s, MM.transpose(S), f"transpose in place {typ}")
    s.transpose(out=s, mask=s, accum=T.PLUS)                                     # S is now the transpose; S<S> += S'
    St = MM.transpose(S)
    check(s, MM.write_back(St, S, St, False, False, False, ("PLUS", typ)), f"S<S> += S' in place {typ}")


CHAINS = [  # operand type, operator, its type, union, output type, accumulator, its type, (mask type, structural, complemented, replace)
    ("INT8", "PLUS", "FP64", True, "INT16", "MIN", "INT32", None),
    ("UINT16", "TIMES", "INT64", False, "FP32", "PLUS", "FP64", ("INT8", False, True, False)),
    ("FP32", "MINUS", "INT32", True, "INT64", "MAX", "FP64", ("FP32", True, False, True)),
]


@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: f"{c[0]}-{c[2]}.{c[1]}-{c[4]}-{c[6]}.{c[5]}")
def test_typecast_chains(gpu, chain):
    """Operands, operator, accumulator and output of four different types: the operands are cast into the operator's type, its result and C into the
    accumulator's, the accumulated value into C's.  (Every value stays inside every type on its way, so each cast is the plain C conversion.)"""
    atyp, op, otyp, union, ctyp, acc, acctyp, mk = chain
    rng = np.random.default_rng(18)
    A = mat("uniform", atyp, seed=18, extreme=atyp == "INT8"); B = mat("uniform", atyp, seed=19, variant=1, extreme=atyp == "INT8")
    B = MM.Mat(B.nrows, B.ncols, np.union1d(B.keys, A.keys[::2]), values(rng, atyp, len(np.union1d(B.keys, A.keys[::2])), atyp == "INT8"))
    kc = np.union1d(pattern("uniform", 2)[2], A.keys[::3]); C = MM.Mat(A.nrows, A.ncols, kc, rand_values(rng, ctyp, len(kc)))
    M = mask_over(rng, mk[0], A, B, C) if mk else None
    c = dev(C)
    (dev(A).eadd if union else dev(A).emult)(dev(B), getattr(TYPE[otyp], op), out=c, mask=dev(M) if mk else None, accum=getattr(TYPE[acctyp], acc),
                                             desc=desc_of(mk[3], mk[1], mk[2]) if mk else None)
    Tm = MM.ewise(op, otyp, A, B, union)
    exp = MM.write_back(C, Tm, M, mk[1] if mk else False, mk[2] if mk else False, mk[3] if mk else False, (acc, acctyp))
    assert exp.typ == ctyp
    check(c, exp, f"typecast chain {chain}")
