"""Which fault wins when a call has two, and what "no mask + complemented mask flag" does, for apply / select / eWise with built-in and user-defined operators.

The drivers of the two operator kinds order their checks differently on purpose:
  user-defined operator:  device, initialised operands, layout refusal (hypersparse / complex), accumulator, dimensions, deferred work, mask
  built-in operator:      device, initialised operands, dimensions, ..., and the accumulator only in the write-back
Containers have 8 positions (8 x 8 matrices), the mismatched operand 9, the hypersparse one the default 2^60.  Every expectation is an error class, an
exact pattern or a counter: there is no tolerance anywhere.  The expectations are what the separate user-defined and built-in drivers did before they were
merged into one function per operation, taken from reading them."""
import numpy as np
import pytest

import test_userop_gpu as U
import test_userselect_gpu as S
from test_userop_gpu import got_dict

pytestmark = pytest.mark.gpu

N = 8
KINDS = ["builtin", "user"]
OPERATIONS = ["apply", "select", "ewise"]


def operands(gb, container, n=N):
    """An operand of n positions (n x n) with entries on every second position, and an output of 8 holding one entry that no operation here produces."""
    idx = np.arange(0, n, 2, dtype=np.uint64)
    x = np.arange(1, len(idx) + 1, dtype=np.float64)
    if container == "vector":
        return gb.Vector.from_arrays(idx, x, n, gb.FP64), gb.Vector.from_lists([1], [6.0], N)
    return gb.Matrix.from_arrays(idx, idx, x, n, n, gb.FP64), gb.Matrix.from_lists([0], [1], [6.0], N, N)


def hyper_operand(gb, container):
    h = gb.Vector.sparse(gb.FP64) if container == "vector" else gb.Matrix.sparse(gb.FP64)
    if container == "vector":
        h[1 << 40] = 2.0
    else:
        h[3, 1 << 40] = 2.0
    return h


def untouched(container):
    return {1: 6.0} if container == "vector" else {(0, 1): 6.0}


def run(gb, operation, kind, a, out, accum=None, desc=None):
    if operation == "apply":
        return a.apply(U.user_op(gb, U.f_unary, "FP64", 1) if kind == "user" else gb.FP64.AINV, out=out, accum=accum, desc=desc)
    if operation == "select":
        return a.select(S.sel(gb, S.mixed, "FP64"), 2.25, out=out, accum=accum, desc=desc) if kind == "user" else a.select(">0", out=out, accum=accum, desc=desc)
    return a.eadd(a, U.user_op(gb, U.f_arith, "FP64", 2) if kind == "user" else gb.FP64.PLUS, out=out, accum=accum, desc=desc)


@pytest.mark.parametrize("operation", OPERATIONS)
@pytest.mark.parametrize("container", ["vector", "matrix"])
def test_built_in_operator_the_dimensions_win_over_the_accumulator(gb, gpu, container, operation):
    a, out = operands(gb, container, N + 1)
    with pytest.raises(gb.DimensionMismatch):
        run(gb, operation, "builtin", a, out, accum=U.user_op(gb, U.f_arith, "FP64", 2))
    assert got_dict(out) == untouched(container)


@pytest.mark.parametrize("operation", OPERATIONS)
@pytest.mark.parametrize("container", ["vector", "matrix"])
def test_user_defined_operator_the_accumulator_wins_over_the_dimensions(gb, gpu, container, operation):
    a, out = operands(gb, container, N + 1)
    with pytest.raises(gb.DomainMismatch, match="f_arith cannot be used as accum"):
        run(gb, operation, "user", a, out, accum=U.user_op(gb, U.f_arith, "FP64", 2))
    assert got_dict(out) == untouched(container)


@pytest.mark.parametrize("operation", ["apply", "select"])
@pytest.mark.parametrize("container", ["vector", "matrix"])
def test_hypersparse_operand_refusal_for_a_user_operator_dimensions_for_a_built_in(gb, gpu, container, operation):
    h = hyper_operand(gb, container)
    _, out = operands(gb, container)
    with pytest.raises(gb.DomainMismatch, match="hypersparse"):
        run(gb, operation, "user", h, out)
    assert got_dict(out) == untouched(container)
    with pytest.raises(gb.DimensionMismatch):
        run(gb, operation, "builtin", h, out)
    assert got_dict(out) == untouched(container)


@pytest.mark.parametrize("replace", [True, False], ids=["replace", "keep"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("operation", OPERATIONS)
@pytest.mark.parametrize("container", ["vector", "matrix"])
def test_no_mask_with_the_complement_flag_writes_nothing(gb, gpu, container, operation, kind, replace):
    a, out = operands(gb, container)
    launched = S.stats(gb)[2]
    run(gb, operation, kind, a, out, desc=gb.descriptor.RC if replace else gb.descriptor.C)
    assert got_dict(out) == ({} if replace else untouched(container))
    if kind == "user":
        assert S.stats(gb)[2] == launched, "a user-defined operator's kernel was launched although nothing may be written"
