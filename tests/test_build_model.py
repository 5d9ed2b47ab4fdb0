"""The build model (tests/build_model.py) pinned against the library's host route (GRB_MI355X_BUILD=0: build_tuples needs no device), bit for bit, for every
real type x {PLUS, TIMES, MIN, MAX, FIRST, SECOND, ANY} (and LOR on BOOL), on inputs whose result depends on the order in which a run is folded: the
floating-point run [1e16, 1, -1e16, 1] in all 24 input orders (the left fold gives 1 or 0 depending on the order), integer runs that wrap, and runs of
distinct values for the selectors."""
import itertools
import os

import numpy as np
import pytest

import build_model as bm
import operator_model as om

REAL = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
OPS = ["PLUS", "TIMES", "MIN", "MAX", "FIRST", "SECOND", "ANY"]
ORDER_RUN = [1e16, 1.0, -1e16, 1.0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host_build(gb, t, I, J, X, nrows, ncols, op):
    typ = getattr(gb, t)
    os.environ["GRB_MI355X_BUILD"] = "0"
    try:
        if J is None:
            return gb.Vector.from_arrays(I, X, nrows, typ, dup=getattr(typ, op) if op else None).to_arrays()
        return gb.Matrix.from_arrays(I, J, X, nrows, ncols, typ, dup=getattr(typ, op) if op else None).to_arrays()
    finally:
        os.environ.pop("GRB_MI355X_BUILD", None)


def run_values(t, rng, length):
    if t == "BOOL":
        return rng.integers(0, 2, length).astype(np.bool_)
    if om.is_fp(t):
        return (rng.standard_normal(length) * 10.0 ** rng.integers(-3, 17, length)).astype(om.NP[t])
    ev = np.array(om.edge_values(t), dtype=om.NP[t])
    return ev[rng.integers(0, len(ev), length)]


def tuples_with_runs(t, rng, nrows, ncols, runs):
    """`runs`: value arrays, each placed on a position of its own; shuffled together with singletons, so that the members of a run are spread over the input."""
    npos = len(runs) + 20
    flat = rng.choice(nrows * ncols, size=npos, replace=False)
    I, J, X = [], [], []
    for p, vals in zip(flat, list(runs) + [run_values(t, rng, 1) for _ in range(20)]):
        I += [p // ncols] * len(vals); J += [p % ncols] * len(vals); X += list(vals)
    perm = rng.permutation(len(I))
    return np.array(I, np.uint64)[perm], np.array(J, np.uint64)[perm], np.array(X, om.NP[t])[perm]


@pytest.mark.parametrize("t", REAL)
def test_model_is_the_host_route(gb, t):
    rng = np.random.default_rng(REAL.index(t))
    for op in OPS + (["LOR"] if t == "BOOL" else []):
        runs = [run_values(t, rng, length) for length in (2, 2, 3, 5, 17, 64, 65)]
        I, J, X = tuples_with_runs(t, rng, 37, 29, runs)
        want = bm.build(t, I, J, X, 37, 29, op)
        gi, gj, gx = host_build(gb, t, I, J, X, 37, 29, op)
        assert np.array_equal(gi, want[0]) and np.array_equal(gj, want[1]) and same_bits(gx, want[2]), (t, op)
        vi, vx = host_build(gb, t, I * np.uint64(29) + J, None, X, 37 * 29, 1, op)
        wv = bm.build(t, I * np.uint64(29) + J, None, X, 37 * 29, 1, op)
        assert np.array_equal(vi, wv[0]) and wv[1] is None and same_bits(vx, wv[2]), (t, op, "vector")


@pytest.mark.parametrize("t", ["FP32", "FP64"])
def test_input_order_decides_a_floating_point_sum(gb, t):
    seen = set()
    for order in itertools.permutations(range(4)):
        X = np.array([ORDER_RUN[k] for k in order] + [2.5], om.NP[t])
        I = np.array([3, 3, 3, 3, 0], np.uint64); J = np.array([1, 1, 1, 1, 2], np.uint64)
        want = bm.build(t, I, J, X, 4, 4, "PLUS")
        gi, gj, gx = host_build(gb, t, I, J, X, 4, 4, "PLUS")
        assert np.array_equal(gi, [0, 3]) and np.array_equal(gj, [2, 1]) and same_bits(gx, want[2]), order
        assert float(want[2][0]) == 2.5
        seen.add(float(want[2][1]))
    assert seen >= {0.0, 1.0}, "the run was chosen so that the order of the fold shows in the sum"


def test_refusals_in_order(gb):
    I = np.array([1, 1, (1 << 32) + 3], np.uint64); J = np.array([0, 0, 0], np.uint64); X = np.ones(3)
    assert bm.build("FP64", I, J, X, 10, 10, None) == bm.OUT_OF_BOUNDS                      # both faults: the bounds error is reported
    assert bm.build("FP64", I[:2], J[:2], X[:2], 10, 10, None) == bm.DUPLICATE
    with pytest.raises(gb.IndexOutOfBound):
        host_build(gb, "FP64", I, J, X, 10, 10, None)
    with pytest.raises(gb.InvalidValue):
        host_build(gb, "FP64", I[:2], J[:2], X[:2], 10, 10, None)


def test_model_pieces():
    assert [bm.bits(d) for d in (0, 1, 2, 3, 1 << 16, (1 << 16) + 1, 0xFFFFFFF0)] == [0, 0, 1, 2, 16, 17, 32]
    r, c, v = bm.build("INT32", [], [], [], 5, 5, "PLUS")
    assert len(r) == 0 and len(c) == 0 and len(v) == 0
    assert np.array_equal(bm.rowptr(np.array([1, 1, 4], np.uint64), 6), [0, 0, 2, 2, 2, 3, 3])
