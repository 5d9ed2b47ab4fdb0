"""Kronecker product and Kronecker power against recorded examples; needs no GPU (the host route runs where there is no device).

tests/golden/reference_kronecker_vectors.json holds the inputs and the expected entries of the modelled project's three docstring examples of
`Matrix.kronecker` and of its test (`diag(0, 1, 2)` with itself) — data only.  Every case runs with the routing left alone and with
GRB_MI355X_KRON=1: on a machine with an MI355X the second run is the device route (the plan string says so), elsewhere both are the host route.
`kronpow` is checked on its docstring's initiator: exponent 0 and 1, and exponent 3 against the products formed here with Python floats.
"""
import contextlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


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


def _matrix(gb, d):
    t = getattr(gb, d["type"])
    return gb.Matrix.from_arrays(np.array(d["I"], np.uint64), np.array(d["J"], np.uint64), np.array(d["V"], t._np), d["nrows"], d["ncols"], t)


def _cases():
    with open(os.path.join(HERE, "golden", "reference_kronecker_vectors.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("route", [None, 1])
def test_reference_kronecker_examples(gb, route):
    cases = _cases()
    assert len(cases) == 4
    on_device = gb.device_info()["ok"] and route == 1
    for case in cases:
        left, right = _matrix(gb, case["left"]), _matrix(gb, case["right"])
        op = getattr(getattr(gb, case["op"][0]), case["op"][1]) if case["op"] else None
        e = case["expect"]
        out = gb.Matrix.sparse(getattr(gb, case["out_type"]), e["nrows"], e["ncols"]) if case["out_type"] else None
        with env(GRB_MI355X_KRON=route):
            got = left.kronecker(right, op=op, out=out)
            plan = gb.last_kernel_plan()
        if out is not None:
            assert got is out
        if on_device:
            assert plan.startswith("kronecker<"), (plan, case["source"])
        assert (got.nrows, got.ncols) == (e["nrows"], e["ncols"]), case["source"]
        I, J, V = got.to_arrays()
        assert I.tolist() == e["I"] and J.tolist() == e["J"], case["source"]
        assert V.tolist() == e["V"], case["source"]


INITIATOR = ([0, 0, 1], [0, 1, 1], [0.77, 0.88, 0.99])


def _initiator(gb):
    return gb.Matrix.from_lists(*INITIATOR)


def test_kronpow_zero_and_one(gb):
    m = _initiator(gb)
    assert m.type is gb.FP64 and m.shape == (2, 2)
    z = m.kronpow(0)
    assert z.type is gb.FP64 and z.shape == (2, 2)
    assert z.to_lists() == [[0, 1], [0, 1], [1.0, 1.0]]
    assert m.kronpow(1) is m
    assert m.to_lists() == [list(INITIATOR[0]), list(INITIATOR[1]), list(INITIATOR[2])]


def test_kronpow_three(gb):
    """Two squarings of the 2 x 2 initiator: 16 x 16 with 81 entries, each value (a b) (c d) in that association — one product per squaring."""
    m = _initiator(gb)
    p = m.kronpow(3)
    assert p is not m and p.shape == (16, 16) and p.nvals == 81
    d = {(i, j): v for i, j, v in zip(*INITIATOR)}
    n = 2
    for _ in range(2):
        d = {(ia * n + ib, ja * n + jb): va * vb for (ia, ja), va in d.items() for (ib, jb), vb in d.items()}
        n *= n
    assert n == 16 and len(d) == 81
    keys = sorted(d)
    I, J, V = p.to_arrays()
    assert I.tolist() == [k[0] for k in keys] and J.tolist() == [k[1] for k in keys]
    assert V.tolist() == [d[k] for k in keys]
    assert m.to_lists() == [list(INITIATOR[0]), list(INITIATOR[1]), list(INITIATOR[2])]      # the initiator itself is untouched
