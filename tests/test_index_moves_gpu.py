"""The seams between the index kernels and the value-moving helpers they share (grb_index.hpp; csr_sort_rows, gather_values, fill_iota_u32 in
grb_matops.hip): the same index argument seen from extract (source of position k) and from assign (position of source index i), the closed-form
inverse of a stride from both callers, values moved as words of 1 / 2 / 4 / 8 bytes, the row sort after an unordered fill, the transpose.

One 70 x 4200 operand whose rows sit on both sides of a wave's 64-entry chunk and of the 2048-entry part of k_extract_rows; every expectation is
numpy indexing on a dense (present, value) model of the operands, never the library.  Values are moved, not computed: every comparison is exact.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NROWS, NCOLS = 70, 4200
ROW_LENGTHS = {11: 0, 3: 1, 7: 63, 18: 64, 25: 65, 39: 2048, 32: 2049, 53: 4100}      # every other row: sparse and random
TYPES = ["BOOL", "INT16", "FP32", "FP64"]                                              # value sizes 1, 2, 4, 8
KINDS = ["all", "range", "stride", "backwards", "increasing", "shuffled", "repeats"]
ASSIGN_KINDS = KINDS[:-1]                                                              # a list that names an index twice is the host route's
LIST_KINDS = ("increasing", "shuffled", "repeats")


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


def values(rng, name, shape):
    if name == "BOOL":
        return rng.integers(0, 2, shape).astype(np.bool_)
    if name == "INT16":
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return rng.standard_normal(shape).astype(np.float32 if name == "FP32" else np.float64)


@functools.lru_cache(maxsize=None)
def index_args(d):
    """{kind: (argument for the Python surface, the positions it names)} over a dimension of d (70 or 4200).  A slice includes its stop, as in the
    reference.  stride: the last step stops short of the bound; backwards: so does the last step down, so the largest k with lo - k step >= bound
    is not the bound itself — q * step == d and q < n of the closed-form inverse both decide something."""
    rng = np.random.default_rng(d)
    if d == NROWS:
        rng_, stride, back = slice(2, 40), slice(3, 66, 4), slice(60, 5, -7)          # 3 .. 63;  60 .. 11: both meet rows of ROW_LENGTHS
        must = sorted(ROW_LENGTHS)
    else:
        rng_, stride, back = slice(100, 3999), slice(5, 4191, 3), slice(4150, 17, -5)  # 5 .. 4190;  4150 .. 20
        must = [0, 63, 64, 2047, 2048, d - 1]
    for s in (stride, back):
        assert abs(s.start - s.stop) % abs(s.step) != 0
    chosen = np.union1d(must, rng.choice(d, size=d // 3, replace=False)).astype(np.int64)
    shuffled = rng.permutation(chosen)
    repeats = np.concatenate([shuffled, shuffled[: d // 7], shuffled[:1]])
    return {"all": (None, np.arange(d)), "range": (rng_, np.arange(rng_.start, rng_.stop + 1)),
            "stride": (stride, np.arange(stride.start, stride.stop + 1, stride.step)), "backwards": (back, np.arange(back.start, back.stop - 1, back.step)),
            "increasing": ([int(x) for x in chosen], chosen), "shuffled": ([int(x) for x in shuffled], shuffled), "repeats": ([int(x) for x in repeats], repeats)}


@functools.lru_cache(maxsize=None)
def operands(name):
    """Dense models (present, value), the same pattern for every type: A 70 x 4200 with the rows of ROW_LENGTHS, a non-empty C of the same shape, two
    vectors of 4200 positions."""
    rng = np.random.default_rng(7)                                   # the pattern first, from one seed: it does not depend on the type
    P = np.zeros((NROWS, NCOLS), np.bool_)
    for r in range(NROWS):
        P[r, rng.choice(NCOLS, size=ROW_LENGTHS.get(r, int(rng.integers(0, 40))), replace=False)] = True
    PC = rng.random((NROWS, NCOLS)) < 0.03
    pu, pw = rng.random(NCOLS) < 0.5, rng.random(NCOLS) < 0.4
    assert [int(P[r].sum()) for r in ROW_LENGTHS] == list(ROW_LENGTHS.values())
    vrng = np.random.default_rng(TYPES.index(name))
    return {"A": (P, values(vrng, name, P.shape)), "C": (PC, values(vrng, name, P.shape)), "u": (pu, values(vrng, name, NCOLS)), "w": (pw, values(vrng, name, NCOLS))}


def matrix_of(gb, name, P, V):
    I, J = np.nonzero(P)
    return gb.Matrix.from_arrays(I.astype(np.uint64), J.astype(np.uint64), V[P], P.shape[0], P.shape[1], getattr(gb, name))


def vector_of(gb, name, p, v):
    return gb.Vector.from_arrays(np.nonzero(p)[0].astype(np.uint64), v[p], len(p), getattr(gb, name))


def check(got, P, V, what):
    """Pattern and values of a result against the dense model (row-major order, as to_arrays gives it); floating-point values bit for bit."""
    exp = [x.astype(np.uint64) for x in np.nonzero(P)] + [V[P]]
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g = np.asarray(g)
        assert g.shape == e.shape and g.dtype.itemsize == e.dtype.itemsize and g.tobytes() == e.tobytes(), f"{what}: got {g[:12]} expected {e[:12]} (lengths {g.shape} / {e.shape})"


@pytest.mark.parametrize("bisect", [False, True], ids=["table", "bisect"])
@pytest.mark.parametrize("name", TYPES)
def test_extract_matrix(gb, gpu, name, bisect):
    """A(I, J) for every pair of index kinds; the pairs with a column list again with the list bisected instead of tabled."""
    P, V = operands(name)["A"]
    A = matrix_of(gb, name, P, V)
    for rk in KINDS:
        for ck in (LIST_KINDS if bisect else KINDS):
            (rarg, rows), (carg, cols) = index_args(NROWS)[rk], index_args(NCOLS)[ck]
            with env(GRB_MI355X_EXTRACT=1, GRB_MI355X_EXTRACT_BISECT=1 if bisect else None):
                T = A.extract_matrix(rarg, carg)
                plan = gb.last_kernel_plan()
            assert plan.startswith("extract_matrix") and ("cols=bisect" in plan) == bisect, plan
            check(T.to_arrays(), P[np.ix_(rows, cols)], V[np.ix_(rows, cols)], f"{name} A({rk}, {ck})")


@pytest.mark.parametrize("name", TYPES)
def test_extract_transposed(gb, gpu, name):
    """A'(I, J) under T0: A(J, I) is extracted and the result goes through csr_transpose, with every value size."""
    P, V = operands(name)["A"]
    A = matrix_of(gb, name, P, V)
    for rk, ck in [("all", "all"), ("range", "shuffled"), ("shuffled", "backwards"), ("backwards", "stride"), ("repeats", "increasing")]:
        (rarg, rows), (carg, cols) = index_args(NCOLS)[rk], index_args(NROWS)[ck]
        with env(GRB_MI355X_EXTRACT=1):
            T = A.extract_matrix(rarg, carg, desc=gb.descriptor.T0)
            plan = gb.last_kernel_plan()
        assert plan.startswith("extract_matrix") and "transpose=1" in plan, plan
        check(T.to_arrays(), P.T[np.ix_(rows, cols)], V.T[np.ix_(rows, cols)], f"{name} A'({rk}, {ck})")


@pytest.mark.parametrize("name", TYPES)
def test_assign_matrix(gb, gpu, name):
    """C(I, J) = S into a non-empty C, no mask, no accumulator, for every pair of index kinds; S is the model's A(I, J), so it carries the long rows."""
    (P, V), (PC, VC) = operands(name)["A"], operands(name)["C"]
    for rk in ASSIGN_KINDS:
        for ck in ASSIGN_KINDS:
            (rarg, rows), (carg, cols) = index_args(NROWS)[rk], index_args(NCOLS)[ck]
            at = np.ix_(rows, cols)
            S, C = matrix_of(gb, name, P[at], V[at]), matrix_of(gb, name, PC, VC)
            with env(GRB_MI355X_ASSIGN=1):
                C.assign_matrix(S, rarg, carg)
                plan = gb.last_kernel_plan()
            assert plan.startswith("assign_matrix"), plan
            EP, EV = PC.copy(), VC.copy()
            EP[at], EV[at] = P[at], V[at]                            # inside I x J: S's entry or none; outside: C's own
            check(C.to_arrays(), EP, EV, f"{name} C({rk}, {ck}) = S")


@pytest.mark.parametrize("name", TYPES)
def test_vectors(gb, gpu, name):
    """u(I) and w(I) = s on vectors of 4200 positions."""
    (pu, vu), (pw, vw) = operands(name)["u"], operands(name)["w"]
    u = vector_of(gb, name, pu, vu)
    for kind in KINDS:
        iarg, idx = index_args(NCOLS)[kind]
        with env(GRB_MI355X_EXTRACT=1):
            t = u.extract(iarg)
            plan = gb.last_kernel_plan()
        assert plan.startswith("extract_vector"), plan
        check(t.to_arrays(), pu[idx], vu[idx], f"{name} u({kind})")
        if kind not in ASSIGN_KINDS:
            continue
        s, w = vector_of(gb, name, pu[idx], vu[idx]), vector_of(gb, name, pw, vw)
        with env(GRB_MI355X_ASSIGN=1):
            w.assign(s, iarg)
            plan = gb.last_kernel_plan()
        assert plan.startswith("assign_vector"), plan
        ep, ev = pw.copy(), vw.copy()
        ep[idx], ev[idx] = pu[idx], vu[idx]
        check(w.to_arrays(), ep, ev, f"{name} w({kind}) = s")
