"""Which fault wins when a call has two, and what "no mask + complemented mask flag" does, for apply / select / eWise with built-in and user-defined operators.

The drivers of the two operator kinds order their checks differently on purpose:
  user-defined operator:  device, initialised operands, layout refusal (hypersparse / complex), accumulator, dimensions, deferred work, mask
  built-in operator:      device, initialised operands, dimensions, ..., and the accumulator only in the write-back
Containers have 8 positions (8 x 8 matrices), the mismatched operand 9, the hypersparse one the default 2^60.  Every expectation is an error class, an
exact pattern or a counter: there is no tolerance anywhere.  The expectations are what the separate user-defined and built-in drivers did before they were
merged into one function per operation, taken from reading them.

The products (mxm / mxv / vxm) order their checks by the kind of the semiring:
  built-in semiring:      device, initialised operands, dimensions, ..., and the accumulator only in the write-back
  user-defined semiring:  operators the compiled route cannot run, device, initialised operands, layout refusal naming the operator, accumulator, dimensions,
                          deferred work, mask
  positional semiring:    layout refusal naming the semiring, device, initialised operands, accumulator, dimensions, deferred work, mask
Those expectations are what the separate user-defined and positional drivers did before they were folded into one off-table driver per product, taken from reading
them; the plan strings are literals written down from a run of that earlier code."""
import numpy as np
import pytest

import test_userop_gpu as U
import test_userselect_gpu as S
import test_usersemiring_gpu as SR
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


# ---- the products: mxm / mxv / vxm with a built-in, a user-defined and a positional semiring --------------------------------------------------------------------
PRODUCTS = ["mxm", "mxv", "vxm"]
SEMIRINGS = ["builtin", "user", "positional"]
OFF_TABLE = ["user", "positional"]


def semiring(gb, kind):
    if kind == "builtin":
        return gb.FP64.PLUS_TIMES
    if kind == "positional":
        return gb.INT64.MIN_SECONDI
    T = gb.FP64
    return T.new_semiring(T.new_monoid(gb.binary_op(T)(SR.u_add), 0.0), gb.binary_op(T)(SR.u_mul))


def product_operands(gb, product, mismatched=False, hyper=False):
    """(A, u, out): the 8 x 8 matrix, the vector operand (None for mxm) and an output of 8 (8 x 8) holding one entry that no product here makes.  `mismatched`: the
    second operand has 9 positions (mxm: both are 9 x 9, against the 8 x 8 output); `hyper`: both operands have the default 2^60 dimensions."""
    container = "matrix" if product == "mxm" else "vector"
    out = operands(gb, container)[1]
    if hyper:
        return hyper_operand(gb, "matrix"), None if product == "mxm" else hyper_operand(gb, "vector"), out
    if product == "mxm":
        return operands(gb, "matrix", N + 1 if mismatched else N)[0], None, out
    return operands(gb, "matrix")[0], operands(gb, "vector", N + 1 if mismatched else N)[0], out


def multiply(product, sr, A, u, out, accum=None, desc=None):
    if product == "mxm":
        return A.mxm(A, sr, out=out, accum=accum, desc=desc)
    if product == "mxv":
        return A.mxv(u, sr, out=out, accum=accum, desc=desc)
    return u.vxm(A, sr, out=out, accum=accum, desc=desc)


def product_untouched(product):
    return untouched("matrix" if product == "mxm" else "vector")


@pytest.mark.parametrize("product", PRODUCTS)
def test_built_in_semiring_the_dimensions_win_over_the_accumulator(gb, gpu, product):
    A, u, out = product_operands(gb, product, mismatched=True)
    with pytest.raises(gb.DimensionMismatch):
        multiply(product, semiring(gb, "builtin"), A, u, out, accum=U.user_op(gb, U.f_arith, "FP64", 2))
    assert got_dict(out) == product_untouched(product)


@pytest.mark.parametrize("kind", OFF_TABLE)
@pytest.mark.parametrize("product", PRODUCTS)
def test_off_table_semiring_the_accumulator_wins_over_the_dimensions(gb, gpu, product, kind):
    A, u, out = product_operands(gb, product, mismatched=True)
    with pytest.raises(gb.DomainMismatch, match="f_arith cannot be used as accum"):
        multiply(product, semiring(gb, kind), A, u, out, accum=U.user_op(gb, U.f_arith, "FP64", 2))
    assert got_dict(out) == product_untouched(product)


@pytest.mark.parametrize("kind", OFF_TABLE)
@pytest.mark.parametrize("product", PRODUCTS)
def test_hypersparse_operand_refusal_names_the_operator_or_the_semiring(gb, gpu, product, kind):
    A, u, out = product_operands(gb, product, hyper=True)
    extent = "dimension" if product == "mxm" else "dimension or size"
    who = (r"user-defined operator u_add: hypersparse containers \(a " + extent + " beyond the device layout") if kind == "user" else "positional semiring GxB_MIN_SECONDI_INT64: hypersparse"
    with pytest.raises(gb.DomainMismatch, match=who):
        multiply(product, semiring(gb, kind), A, u, out)
    assert got_dict(out) == product_untouched(product)


@pytest.mark.parametrize("replace", [True, False], ids=["replace", "keep"])
@pytest.mark.parametrize("kind", SEMIRINGS)
@pytest.mark.parametrize("product", PRODUCTS)
def test_product_with_no_mask_and_the_complement_flag_writes_nothing(gb, gpu, product, kind, replace):
    A, u, out = product_operands(gb, product)
    sr = semiring(gb, kind)
    launched = S.stats(gb)[2]
    multiply(product, sr, A, u, out, desc=gb.descriptor.RC if replace else gb.descriptor.C)
    plan = gb.last_kernel_plan()
    assert got_dict(out) == ({} if replace else product_untouched(product))
    assert plan == "", "no kernel ran, so the plan string names none"
    if kind == "user":
        assert S.stats(gb)[2] == launched, "a user-defined semiring's kernel was launched although nothing may be written"


# written down from a run of the code before the fold, on the operands of product_operands (an 8 x 8 matrix and an 8-vector with four entries each)
PLANS = {
    ("user", "mxm"): "usersr<add=u_add,mul=u_mul,type=GrB_FP64,kind=mxm> grb_usersr_product pattern: spgemm_hash<static> symbolic bins 4/0/0/0/0 numeric bins 4/0/0/0",
    ("user", "mxv"): "usersr<add=u_add,mul=u_mul,type=GrB_FP64,kind=mxv> grb_usersr_rows",
    ("user", "vxm"): "usersr<add=u_add,mul=u_mul,type=GrB_FP64,kind=vxm> grb_usersr_rows",
    ("positional", "mxm"): "possr<add=MIN,mul=SECONDI,type=INT64,kind=mxm> k_possr_product pattern: spgemm_hash<static> symbolic bins 4/0/0/0/0 numeric bins 4/0/0/0",
    ("positional", "mxv"): "possr<add=MIN,mul=SECONDI,type=INT64,kind=mxv> k_possr_rows",
    ("positional", "vxm"): "possr<add=MIN,mul=SECONDI,type=INT64,kind=vxm> k_possr_rows",
}


@pytest.mark.parametrize("kind", OFF_TABLE)
@pytest.mark.parametrize("product", PRODUCTS)
def test_off_table_plan_string_is_what_it_was(gb, gpu, product, kind):
    A, u, _ = product_operands(gb, product)
    multiply(product, semiring(gb, kind), A, u, None)
    assert gb.last_kernel_plan() == PLANS[kind, product]
