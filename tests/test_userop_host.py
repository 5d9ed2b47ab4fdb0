"""User-defined operators, the part that needs no device: the Python -> C translator of pygraphblas_amd/userop.py checked against Python itself,
what it refuses, and the argument checks and object bookkeeping of GxB_UnaryOp_new / GxB_BinaryOp_new / GrB_*Op_free.

Translator against Python: for every function of CASES the generated definition is compiled as plain C with the host compiler into a shared object and
called through ctypes over a grid of operands per type; the result must equal the Python function's own, converted to the operator's type — bit for bit
for arithmetic-only functions, within 4 ulp of the type for functions that call the math library (libm on both sides).  Integer grids stay where Python's
unbounded integers and C agree: no overflow, shifts below the width, negative operands for // and % included."""
import ctypes as C
import itertools
import math
import os
import shutil
import subprocess
from math import exp, log1p

import numpy as np
import pytest

PRELUDE = "#include <stdint.h>\n#include <stdbool.h>\n#include <math.h>\n"
CT = {"BOOL": C.c_bool, "INT8": C.c_int8, "UINT8": C.c_uint8, "INT32": C.c_int32, "INT64": C.c_int64, "FP32": C.c_float, "FP64": C.c_double}
NP = {"BOOL": np.bool_, "UINT8": np.uint8, "INT32": np.int32, "INT64": np.int64, "FP32": np.float32, "FP64": np.float64}
SHIFT = 5
SCALE = 0.375


# ---- the functions (module level: their source must be readable) ---------------------------------------------------------------------------------
def log_plus(x, y):                                   # Log-Semiring.ipynb: Log32.PLUS
    return x + log1p(exp(y - x))


def one_bit_off(i, j):                                # N-Cube-Graphs.ipynb
    def bit_count(i):
        assert 0 <= i < 0x100000000
        i = i - ((i >> 1) & 0x55555555)
        i = (i & 0x33333333) + ((i >> 2) & 0x33333333)
        return (((i + (i >> 4) & 0xF0F0F0F) * 0x1010101) & 0xffffffff) >> 24

    if bit_count(i ^ j) == 1:
        return 1
    return 0


def relu_plus(x, y):                                  # RadiX-Net: ReLUNeuron.PLUS
    return min(x + y, 32)


def arith(x, y):
    return x * y - (x + y) * 2


def unary_signs(x):
    return -x + (+x) * 3


def invert(x):
    return ~x & 0x7F


def lnot(x):
    return not x


def bits(x, y):
    return ((x & y) | (x ^ 5)) ^ (y << 2) ^ (x >> 1)


def shifts(x, y):
    return (x << SHIFT) + (y >> 2)                    # SHIFT: a module-level constant


def compare(x, y):
    return (x < y) + 2 * (x <= y) + 4 * (x == y) + 8 * (x != y) + 16 * (x > y) + 32 * (x >= y)


def chained(x, y):
    return 1 if 0 <= x < y <= 100 else 0


def bool_ops(x, y):
    return (x and y) + 3 * (x or y) + (7 if x > 1 and y > 1 or x < -1 else 0)


def true_div(x, y):
    return x / (y * y + 1)


def floor_div(x, y):
    return x // (y if y else 3)


def modulo(x, y):
    return x % (y if y else 7)


def floor_div_f(x, y):
    return x // (y if y != 0 else 0.75)


def modulo_f(x, y):
    return x % (y if y != 0 else -0.75)


def power(x, y):
    return x ** 2 + abs(y) ** 3


def power_f(x, y):
    return abs(x) ** 0.5 + y ** 2


def locals_and_aug(x, y):
    t = x
    t += y
    t *= 2
    u = t - 1
    t -= u // 2
    return t + u


def branches(x, y):
    if x > y:
        r = x - y
    elif x == y:
        r = 0
    else:
        if y > 10:
            return -1
        r = y - x
    return r


def cond_expr(x, y):
    return x if x > y else (y if y > 0 else 0)


def minmax_abs(x, y):
    return max(x, y, 3) - min(x, y) + abs(x - y)


def scaled(x):
    return x * SCALE + True                           # float and bool constants, one from the module


def helper_twice(x, y):
    def sq(a):
        return a * a

    def hyp2(a, b):
        return sq(a) + sq(b)

    return hyp2(x, y) + sq(x / 2)                     # sq is specialised for an integer and for a double argument in an integer operator


def math_many(x, y):
    return math.sqrt(abs(x)) + math.sin(x) * math.cos(y) + math.tanh(x) + math.atan2(x, y) + math.log(abs(y) + 1) + math.expm1(x / 8) + math.pow(abs(x), 1.5) + math.copysign(x, y) + math.fmod(x, y + 0.5)


def math_to_int(x):
    return math.floor(x) + 10 * math.ceil(x) + 100 * math.trunc(x) + 1000 * (math.isnan(x) or math.isinf(x))


def math_rest(x):
    return math.log2(abs(x) + 1) + math.log10(abs(x) + 1) + math.exp(x / 4) + math.tan(x / 4) + math.asin(x / 8) + math.acos(x / 8) + math.atan(x) + math.sinh(x / 2) + math.cosh(x / 2) + math.fabs(x)


GRID = {
    "FP64": [-3.5, -1.0, -0.375, 0.0, 0.5, 1.0, 2.25, 7.0],
    "FP32": [-3.5, -1.0, -0.375, 0.0, 0.5, 1.0, 2.25, 7.0],
    "INT64": [-1000003, -17, -3, -1, 0, 1, 2, 5, 12, 100, 65537],
    "INT32": [-17, -3, -1, 0, 1, 2, 5, 12, 100],
    "UINT8": [0, 1, 2, 3, 5, 7, 11],
    "BOOL": [False, True],
}
# (function, number of arguments, types it is checked on, calls the math library[, its own operand grid])
CASES = [
    (log_plus, 2, ["FP32", "FP64"], True),
    (one_bit_off, 2, ["INT64"], False, list(range(0, 18)) + [255, 256, 65535, 65536, 0xFFFFFFFE]),      # (its own assert: 0 <= i ^ j < 2^32)
    (relu_plus, 2, ["FP32", "FP64", "INT64"], False),
    (arith, 2, ["FP32", "FP64", "INT64", "INT32"], False),
    (unary_signs, 1, ["FP64", "INT64", "INT32"], False),
    (invert, 1, ["INT64", "INT32", "UINT8"], False),
    (lnot, 1, ["FP64", "INT64", "UINT8", "BOOL"], False),
    (bits, 2, ["INT64", "UINT8"], False),
    (shifts, 2, ["INT64", "INT32"], False),
    (compare, 2, ["FP32", "FP64", "INT64", "INT32", "UINT8"], False),
    (chained, 2, ["FP64", "INT64", "UINT8"], False),
    (bool_ops, 2, ["FP64", "INT64", "INT32"], False),
    (true_div, 2, ["FP32", "FP64", "INT64"], False),
    (floor_div, 2, ["INT64", "INT32"], False),
    (modulo, 2, ["INT64", "INT32"], False),
    (floor_div_f, 2, ["FP64", "FP32"], False),
    (modulo_f, 2, ["FP64", "FP32"], False),
    (power, 2, ["INT64", "INT32"], False),
    (power_f, 2, ["FP64"], True),
    (locals_and_aug, 2, ["FP64", "INT64", "INT32"], False),
    (branches, 2, ["FP64", "INT64", "INT32"], False),
    (cond_expr, 2, ["FP32", "INT64", "BOOL"], False),
    (minmax_abs, 2, ["FP64", "INT64", "INT32"], False),
    (scaled, 1, ["FP64", "FP32"], False),
    (helper_twice, 2, ["FP64", "INT64"], False),
    (math_many, 2, ["FP64", "FP32"], True),
    (math_to_int, 1, ["FP64", "FP32"], False),
    (math_rest, 1, ["FP64", "FP32"], True),
]


def as_type(typ, r):
    """A Python result as a value of the operator's type: what the C cast of the returned value gives (in range by the grids' construction)."""
    if typ == "BOOL":
        return bool(r)
    if typ.startswith("FP"):
        return NP[typ](r)
    return NP[typ](int(r))                            # a float result of an integer operator truncates toward zero, as a C cast does


@pytest.fixture(scope="module")
def cc():
    exe = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if exe is None:
        pytest.skip("no host C compiler (cc / gcc / clang) on the PATH")
    return exe


@pytest.mark.parametrize("case", CASES, ids=[c[0].__name__ for c in CASES])
def test_translation_matches_python(gb, cc, tmp_path, case):
    from pygraphblas_amd.userop import translate
    func, nargs, typs, uses_math = case[:4]
    for typ in typs:
        T = getattr(gb, typ)
        defn = translate(func, T, nargs)
        src = tmp_path / f"{func.__name__}_{typ}.c"
        so = tmp_path / f"{func.__name__}_{typ}.so"
        src.write_text(PRELUDE + defn)
        # -ffp-contract=off: no fused multiply-add the Python evaluation does not form either (the device build uses the same option)
        subprocess.check_call([cc, "-O1", "-ffp-contract=off", "-fwrapv", "-shared", "-fPIC", "-o", str(so), str(src), "-lm"])
        fn = getattr(C.CDLL(str(so)), func.__name__)
        fn.restype = None
        ct = CT[typ]
        worst = 0.0
        for args in itertools.product(case[4] if len(case) > 4 else GRID[typ], repeat=nargs):
            typed = [as_type(typ, a) for a in args]                     # what the operator receives: values of its type
            py = [bool(a) if typ == "BOOL" else (float(a) if typ.startswith("FP") else int(a)) for a in typed]
            want = as_type(typ, func(*py))
            z = ct()
            fn(C.byref(z), *[C.byref(ct(p)) for p in py])
            got = as_type(typ, z.value)
            if uses_math and typ.startswith("FP"):
                if math.isfinite(float(want)):
                    ulp = float(np.spacing(np.abs(want))) if want != 0 else float(np.finfo(NP[typ]).tiny)
                    err = abs(float(got) - float(want)) / ulp
                    worst = max(worst, err)
                    assert err <= 4.0, f"{func.__name__} {typ}{args}: C gives {got!r}, Python {want!r} ({err:.2f} ulp)\n{defn}"
                else:
                    assert str(got) == str(want), f"{func.__name__} {typ}{args}: C gives {got!r}, Python {want!r}\n{defn}"
            else:
                same = (got == want) or (got != got and want != want)
                if typ.startswith("FP") and same and got == 0:
                    same = math.copysign(1.0, float(got)) == math.copysign(1.0, float(want))      # bit-exact: the zero's sign too
                assert same, f"{func.__name__} {typ}{args}: C gives {got!r}, Python {want!r}\n{defn}"
        if uses_math:
            print(f"{func.__name__} {typ}: largest difference to Python {worst:.2f} ulp")


# ---- what the translator refuses ---------------------------------------------------------------------------------------------------------------------
def uses_random(x):
    import random
    return random.uniform(0, x)


def uses_random_attr(x):
    return math.sqrt(x) + np.random.uniform(0, 1)


def uses_for(x):
    t = 0
    for k in range(3):
        t += x
    return t


def uses_unknown_name(x):
    return x + not_defined_anywhere        # noqa: F821


def uses_while(x):
    while x > 0:
        x -= 1
    return x


def uses_attribute(x):
    return x.real


def uses_closure_object(x):
    return x + len(GRID)


def no_return(x):
    if x > 0:
        return 1


def bitop_on_float(x, y):
    return x & y


@pytest.mark.parametrize("func,nargs,needle", [
    (uses_random, 1, "import"), (uses_random_attr, 1, "named function"), (uses_for, 1, "'for' loop"), (uses_unknown_name, 1, "not_defined_anywhere"),
    (uses_while, 1, "'while' loop"), (uses_attribute, 1, "attribute access"), (uses_closure_object, 1, "GRID"), (no_return, 1, "without returning"),
    (bitop_on_float, 2, "'&' on a floating-point value")], ids=lambda v: getattr(v, "__name__", None))
def test_unsupported_python_is_refused_at_decoration(gb, func, nargs, needle):
    deco = gb.unary_op if nargs == 1 else gb.binary_op
    with pytest.raises(TypeError) as e:
        deco(gb.FP64)(func)
    assert needle in str(e.value) and "line" in str(e.value), str(e.value)


def test_random_uniform_names_the_call(gb):
    """What the Intro-Prez and Sierpinski-Graph notebooks' operators call: there is no device counterpart, and the error says which call it was."""
    with pytest.raises(TypeError, match=r"random\.uniform"):
        gb.unary_op(gb.FP64)(random_uniform)


def random_uniform(x):
    return random.uniform(0, 1)            # noqa: F821


def test_wrong_parameter_count_is_refused(gb):
    with pytest.raises(TypeError, match="parameter"):
        gb.unary_op(gb.FP64)(arith)
    with pytest.raises(TypeError, match="parameter"):
        gb.binary_op(gb.FP64)(scaled)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------------------------
DEFN_U = b"void twice (double *z, const double *x) { (*z) = 2 * (*x) ; }"
DEFN_B = b"void addsq (double *z, const double *x, const double *y) { (*z) = (*x) + (*y) * (*y) ; }"


def handle(gb, name):
    return C.c_void_p(gb._capi.handle(name))


def test_new_checks_its_arguments(gb):
    lib, d = gb.lib, gb._capi.constants
    fp64, fp32, fc64 = handle(gb, "GrB_FP64"), handle(gb, "GrB_FP32"), handle(gb, "GxB_FC64")
    u, b = C.c_void_p(), C.c_void_p()
    assert lib.GxB_UnaryOp_new(C.byref(u), None, fp64, fp64, b"twice", None) == d["GrB_NULL_POINTER"]
    assert lib.GxB_UnaryOp_new(C.byref(u), None, fp64, fp64, None, DEFN_U) == d["GrB_NULL_POINTER"]
    assert lib.GxB_BinaryOp_new(C.byref(b), None, fp64, fp64, fp64, b"addsq", None) == d["GrB_NULL_POINTER"]
    assert lib.GxB_BinaryOp_new(C.byref(b), None, fp64, fp64, fp64, None, DEFN_B) == d["GrB_NULL_POINTER"]
    assert lib.GxB_BinaryOp_new(None, None, fp64, fp64, fp64, b"addsq", DEFN_B) == d["GrB_NULL_POINTER"]
    # all of the operator's types are one real built-in type
    assert lib.GxB_UnaryOp_new(C.byref(u), None, fp64, fp32, b"twice", DEFN_U) == d["GrB_DOMAIN_MISMATCH"]
    assert lib.GxB_BinaryOp_new(C.byref(b), None, fp64, fp64, fp32, b"addsq", DEFN_B) == d["GrB_DOMAIN_MISMATCH"]
    assert lib.GxB_BinaryOp_new(C.byref(b), None, fp32, fp64, fp64, b"addsq", DEFN_B) == d["GrB_DOMAIN_MISMATCH"]
    assert lib.GxB_UnaryOp_new(C.byref(u), None, fc64, fc64, b"twice", DEFN_U) == d["GrB_DOMAIN_MISMATCH"]
    assert lib.GxB_BinaryOp_new(C.byref(b), None, fc64, fc64, fc64, b"addsq", DEFN_B) == d["GrB_DOMAIN_MISMATCH"]
    assert u.value is None and b.value is None
    buf = C.create_string_buffer(512)
    lib.GrBX_last_error(buf, C.c_int(512))
    assert b"addsq" in buf.value
    # fn is never called: NULL and a non-NULL pointer are both accepted
    assert lib.GxB_UnaryOp_new(C.byref(u), None, fp64, fp64, b"twice", DEFN_U) == 0 and u.value
    assert lib.GxB_BinaryOp_new(C.byref(b), C.c_void_p(1), fp64, fp64, fp64, b"addsq", DEFN_B) == 0 and b.value
    t = C.c_void_p()
    assert lib.GxB_UnaryOp_xtype(C.byref(t), u) == 0 and t.value == fp64.value
    assert lib.GxB_BinaryOp_ztype(C.byref(t), b) == 0 and t.value == fp64.value
    assert lib.GrB_UnaryOp_free(C.byref(u)) == 0 and u.value is None
    assert lib.GrB_BinaryOp_free(C.byref(b)) == 0 and b.value is None


def test_free_releases_user_operators_and_leaves_built_ins(gb):
    lib = gb.lib
    fp64 = handle(gb, "GrB_FP64")
    b = C.c_void_p()
    assert lib.GxB_BinaryOp_new(C.byref(b), None, fp64, fp64, fp64, b"addsq", DEFN_B) == 0
    assert lib.GrB_BinaryOp_free(C.byref(b)) == 0 and b.value is None
    assert lib.GrB_BinaryOp_free(C.byref(b)) == 0 and b.value is None              # the nulled handle: a second free is a success
    assert lib.GrB_BinaryOp_free(None) == 0
    u = C.c_void_p()
    assert lib.GxB_UnaryOp_new(C.byref(u), None, fp64, fp64, b"twice", DEFN_U) == 0
    assert lib.GrB_UnaryOp_free(C.byref(u)) == 0 and u.value is None
    assert lib.GrB_UnaryOp_free(C.byref(u)) == 0
    plus, ainv = handle(gb, "GrB_PLUS_FP64"), handle(gb, "GrB_AINV_FP64")
    keep_plus, keep_ainv = plus.value, ainv.value
    assert lib.GrB_BinaryOp_free(C.byref(plus)) == 0 and plus.value == keep_plus     # built-in handles stay untouched
    assert lib.GrB_UnaryOp_free(C.byref(ainv)) == 0 and ainv.value == keep_ainv
    t = C.c_void_p()
    assert lib.GxB_BinaryOp_ztype(C.byref(t), plus) == 0 and t.value == fp64.value


def test_decorated_operator_objects(gb):
    op = gb.binary_op(gb.FP32)(log_plus)
    assert isinstance(op, gb.BinaryOp) and op.kind == "BinaryOp" and op.type is gb.FP32 and op.name == "log_plus" and op.get_op()
    assert "void log_plus(float *z, const float *x, const float *y)" in op.defn and "log1p(exp(" in op.defn
    un = gb.unary_op(gb.INT64)(invert)
    assert isinstance(un, gb.UnaryOp) and un.kind == "UnaryOp" and "void invert(int64_t *z, const int64_t *x)" in un.defn
    with op:                                                                       # the default eWise operator inside the block, like a built-in
        assert gb.types.current_binop.get() is op
    assert gb.types.current_binop.get(None) is None
    nested = gb.binary_op(gb.INT64)(one_bit_off)
    assert nested.defn.index("static int64_t one_bit_off__bit_count_i(") < nested.defn.index("void one_bit_off(")
    # users of the C ABI: refused where a user-defined operator cannot run, naming it, before any device is asked for
    m = C.c_void_p()
    assert gb.lib.GrB_Monoid_new_FP32(C.byref(m), C.c_void_p(op.get_op()), C.c_float(0)) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and m.value is None
    buf = C.create_string_buffer(512)
    gb.lib.GrBX_last_error(buf, C.c_int(512))
    assert b"log_plus" in buf.value
    s = C.c_void_p()
    assert gb.lib.GrB_Semiring_new(C.byref(s), handle(gb, "GrB_PLUS_MONOID_FP32"), C.c_void_p(op.get_op())) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and s.value is None


def test_running_one_without_a_device_fails_loudly(gb):
    if gb.device_info()["ok"]:
        pytest.skip("a HIP device is present")
    plus = gb.binary_op(gb.FP64)(arith)
    un = gb.unary_op(gb.FP64)(unary_signs)
    m = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    for call in (lambda: m.apply(un), lambda: v.apply(un), lambda: m.eadd(m, plus), lambda: m.emult(m, plus), lambda: v.eadd(v, plus), lambda: v.emult(v, plus),
                 lambda: m.apply_first(1.0, plus), lambda: m.apply_second(plus, 1.0), lambda: v.apply_first(1.0, plus), lambda: v.apply_second(plus, 1.0)):
        with pytest.raises(gb.Panic, match="no device"):
            call()
