"""User-defined select operators, the part that needs no device: the Python -> C translation of `@select_op` predicates checked against Python itself, what
is refused at decoration, and the argument checks and object bookkeeping of GxB_SelectOp_new / GxB_SelectOp_free / GxB_SelectOp_fprint.

Translator against Python: the generated definition is compiled as plain C with the host compiler (as tests/test_userop_host.py does) and called through
ctypes over a grid of (i, j, x, thunk) — i and j include 0, 2^31 and 2^32 - 1 — and the `bool` it returns must equal the truth of the Python function's own
result.  Every predicate here is arithmetic only, so the comparison is exact."""
import ctypes as C
import itertools
import shutil
import subprocess

import numpy as np
import pytest

PRELUDE = "#include <stdint.h>\n#include <stdbool.h>\n#include <math.h>\ntypedef uint64_t GrB_Index;\n"
CT = {"BOOL": C.c_bool, "UINT8": C.c_uint8, "INT64": C.c_int64, "FP32": C.c_float, "FP64": C.c_double}
LIMIT = 3
INDICES = [0, 1, 5, 1 << 31, (1 << 32) - 1]
GRID = {
    "FP64": [-3.5, -0.375, 0.0, 0.5, 2.25, 7.0, 100.0, 100.5],
    "FP32": [-3.5, -0.375, 0.0, 0.5, 2.25, 7.0, 100.0, 100.5],
    "INT64": [-1000003, -3, -1, 0, 1, 2, 5, 100, 101],
    "UINT8": [0, 1, 2, 3, 7, 100, 101, 255],
    "BOOL": [False, True],
}


# ---- the predicates (module level: their source must be readable) ------------------------------------------------------------------------------------
def band_above(i, j, x, v):                           # `and`, a captured module constant
    return abs(i - j) <= LIMIT and x > v


def checkerboard(i, j, x, v):                         # `%`, `//`, `or`
    return (i + j) % 3 == 0 or (i // 2) % 2 == 1 and x != v


def chained(i, j, x, v):                              # a chained comparison
    return 0 <= x < v <= 100


def far_and_different(i, j, x, v):                    # a nested helper
    def far(a, b):
        return abs(a - b) > 2

    return far(i, j) and x != v


def upper_half_columns(i, j, x, v):                   # i and j only; the index must arrive unsigned and whole
    return j >= 2147483648 and i < 4294967295


def value_itself(i, j, x, v):                         # the truth of a value (not a comparison's 0 / 1)
    return x


def branches(i, j, x, v):
    if i == j:
        return False
    t = x * 2
    if t > v:
        return True
    return j - i == 1


CASES = [(band_above, ["FP64", "FP32", "INT64", "UINT8"]), (checkerboard, ["FP64", "INT64", "UINT8", "BOOL"]), (chained, ["FP64", "FP32", "INT64", "UINT8"]),
         (far_and_different, ["FP64", "INT64", "BOOL"]), (upper_half_columns, ["FP64", "BOOL"]), (value_itself, ["FP64", "FP32", "INT64", "UINT8", "BOOL"]),
         (branches, ["FP64", "INT64", "UINT8"])]


@pytest.fixture(scope="module")
def cc():
    exe = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if exe is None:
        pytest.skip("no host C compiler (cc / gcc / clang) on the PATH")
    return exe


def py_value(typ, a):
    return bool(a) if typ == "BOOL" else (float(np.float32(a)) if typ == "FP32" else (float(a) if typ == "FP64" else int(a)))


def compiled(cc, tmp_path, func, typ, ttyp, gb):
    from pygraphblas_amd.userop import translate_select
    defn = translate_select(func, getattr(gb, typ), getattr(gb, ttyp) if ttyp else None)
    stem = f"{func.__name__}_{typ}_{ttyp}"
    src, so = tmp_path / (stem + ".c"), tmp_path / (stem + ".so")
    src.write_text(PRELUDE + defn)
    subprocess.check_call([cc, "-O1", "-ffp-contract=off", "-fwrapv", "-shared", "-fPIC", "-o", str(so), str(src), "-lm"])
    fn = getattr(C.CDLL(str(so)), func.__name__)
    fn.restype = C.c_bool
    return fn, defn


@pytest.mark.parametrize("case", CASES, ids=[c[0].__name__ for c in CASES])
def test_translation_matches_python(gb, cc, tmp_path, case):
    func, typs = case
    for typ in typs:
        fn, defn = compiled(cc, tmp_path, func, typ, None, gb)
        assert f"bool {func.__name__}(GrB_Index i, GrB_Index j, const " in defn
        for i, j, x, v in itertools.product(INDICES, INDICES, GRID[typ], GRID[typ]):
            x, v = py_value(typ, x), py_value(typ, v)
            want = bool(func(i, j, x, v))
            got = fn(C.c_uint64(i), C.c_uint64(j), C.byref(CT[typ](x)), C.byref(CT[typ](v)))
            assert got is want, f"{func.__name__} {typ} (i={i}, j={j}, x={x!r}, thunk={v!r}): C gives {got}, Python {want}\n{defn}"


def test_thunk_of_another_type_has_its_own_base(gb, cc, tmp_path):
    """x and the thunk are converted from their own C types: an INT64 thunk of an FP64 operator is an integer in the predicate (`//` is the integer one)."""
    def halves(i, j, x, v):
        return x > v // 2

    fn, defn = compiled(cc, tmp_path, halves, "FP64", "INT64", gb)
    assert "const double *x, const int64_t *thunk" in defn and "grb_floordiv_i" in defn
    for x, v in itertools.product(GRID["FP64"], GRID["INT64"]):
        assert fn(C.c_uint64(0), C.c_uint64(0), C.byref(C.c_double(x)), C.byref(C.c_int64(v))) is bool(halves(0, 0, x, v)), (x, v)
    fn, defn = compiled(cc, tmp_path, halves, "INT64", "FP64", gb)
    assert "const int64_t *x, const double *thunk" in defn and "grb_floordiv_d" in defn
    for x, v in itertools.product(GRID["INT64"], GRID["FP64"]):
        assert fn(C.c_uint64(0), C.c_uint64(0), C.byref(C.c_int64(x)), C.byref(C.c_double(v))) is bool(halves(0, 0, x, v)), (x, v)


# ---- what is refused at decoration -------------------------------------------------------------------------------------------------------------------
def three_parameters(i, j, x):
    return x > 0


def five_parameters(i, j, x, v, w):
    return x > 0


def uses_random(i, j, x, v):
    return random.random() < 0.5           # noqa: F821


def uses_loop(i, j, x, v):
    for k in range(3):
        x += k
    return x > v


def test_wrong_parameter_count_is_refused(gb):
    for f in (three_parameters, five_parameters):
        with pytest.raises(TypeError, match="parameter"):
            gb.select_op(gb.FP64)(f)


def test_a_lambda_is_refused(gb):
    with pytest.raises(TypeError, match="lambda"):
        gb.select_op(gb.FP64)(lambda i, j, x, v: x > v)
    multi = (lambda i, j, x, v:
             x > v)
    with pytest.raises(TypeError, match="lambda"):
        gb.select_op(gb.FP64)(multi)


def test_random_and_loops_are_refused_naming_the_construct(gb):
    with pytest.raises(TypeError, match=r"random\.random") as e:
        gb.select_op(gb.FP64)(uses_random)
    assert "line" in str(e.value)
    with pytest.raises(TypeError, match="'for' loop"):
        gb.select_op(gb.FP64, gb.INT64)(uses_loop)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------------------------
DEFN = b"bool above (GrB_Index i, GrB_Index j, const double *x, const double *thunk) { return j > i && (*x) > (*thunk) ; }"


def handle(gb, name):
    return C.c_void_p(gb._capi.handle(name))


def last_error(gb):
    buf = C.create_string_buffer(1024)
    gb.lib.GrBX_last_error(buf, C.c_int(1024))
    return buf.value.decode()


def test_new_checks_its_arguments(gb):
    lib, d = gb.lib, gb._capi.constants
    fp64, int32, fc64, fc32 = handle(gb, "GrB_FP64"), handle(gb, "GrB_INT32"), handle(gb, "GxB_FC64"), handle(gb, "GxB_FC32")
    s = C.c_void_p()
    assert lib.GxB_SelectOp_new(None, None, fp64, fp64, b"above", DEFN) == d["GrB_NULL_POINTER"]
    assert lib.GxB_SelectOp_new(C.byref(s), None, None, fp64, b"above", DEFN) == d["GrB_NULL_POINTER"]
    assert lib.GxB_SelectOp_new(C.byref(s), None, fp64, fp64, None, DEFN) == d["GrB_NULL_POINTER"]
    assert lib.GxB_SelectOp_new(C.byref(s), None, fp64, fp64, b"above", None) == d["GrB_NULL_POINTER"]
    blank = C.create_string_buffer(128)                                            # memory that is no GraphBLAS object
    not_a_type = C.cast(blank, C.c_void_p)
    assert lib.GxB_SelectOp_new(C.byref(s), None, not_a_type, fp64, b"above", DEFN) == d["GrB_UNINITIALIZED_OBJECT"]
    assert lib.GxB_SelectOp_new(C.byref(s), None, fp64, not_a_type, b"above", DEFN) == d["GrB_UNINITIALIZED_OBJECT"]
    # complex value or thunk types
    for xt, tt in ((fc64, fc64), (fc64, None), (fp64, fc32), (fc32, fp64)):
        assert lib.GxB_SelectOp_new(C.byref(s), None, xt, tt, b"above", DEFN) == d["GrB_DOMAIN_MISMATCH"]
        assert "above" in last_error(gb)
    # the name: a C identifier of at most 39 characters
    for bad in (b"", b"9lives", b"has space", b"semi;colon", b"a" * 40):
        assert lib.GxB_SelectOp_new(C.byref(s), None, fp64, fp64, bad, DEFN) == d["GrB_INVALID_VALUE"], bad
        assert "GxB_SelectOp_new" in last_error(gb)
    assert s.value is None
    # accepted: fn NULL or not, ttype NULL (= xtype) or another real type, a name of 39 characters
    made = []
    for fn, tt, name in ((None, fp64, b"above"), (C.c_void_p(1), None, b"above"), (None, int32, b"above"), (None, None, b"_" + b"b" * 38)):
        h = C.c_void_p()
        assert lib.GxB_SelectOp_new(C.byref(h), fn, fp64, tt, name, DEFN) == 0 and h.value
        made.append(h)
    assert len({h.value for h in made}) == 4
    for h in made:
        assert lib.GxB_SelectOp_free(C.byref(h)) == 0 and h.value is None


def test_free_is_idempotent_and_spares_the_built_ins(gb):
    lib = gb.lib
    fp64 = handle(gb, "GrB_FP64")
    s = C.c_void_p()
    assert lib.GxB_SelectOp_new(C.byref(s), None, fp64, None, b"above", DEFN) == 0
    assert lib.GxB_SelectOp_free(C.byref(s)) == 0 and s.value is None
    assert lib.GxB_SelectOp_free(C.byref(s)) == 0 and s.value is None              # the nulled handle: a second free is a success
    assert lib.GxB_SelectOp_free(None) == 0
    tril = handle(gb, "GxB_TRIL")
    keep = tril.value
    assert lib.GxB_SelectOp_free(C.byref(tril)) == 0 and tril.value == keep         # a built-in handle stays untouched ...
    assert lib.GxB_SelectOp_fprint(tril, b"t", C.c_int(0), None) == 0               # ... and alive
    assert len(gb._capi.names["GxB_SelectOp"]) == 16                               # the header gained functions, no handle


def fprint_text(gb, h, tmp_path):
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    path = tmp_path / "fprint.txt"
    f = libc.fopen(str(path).encode(), b"w")
    assert f
    try:
        assert gb.lib.GxB_SelectOp_fprint(h, b"shown", C.c_int(3), C.c_void_p(f)) == 0
    finally:
        libc.fclose(C.c_void_p(f))
    return path.read_text()


def test_fprint_says_user_defined_and_shows_the_types(gb, tmp_path):
    s = C.c_void_p()
    assert gb.lib.GxB_SelectOp_new(C.byref(s), None, handle(gb, "GrB_FP64"), handle(gb, "GrB_INT32"), b"above", DEFN) == 0
    text = fprint_text(gb, s, tmp_path)
    assert "SelectOp" in text and "shown" in text and "above" in text and "(user-defined)" in text and "GrB_FP64" in text and "GrB_INT32" in text, text
    gb.lib.GxB_SelectOp_free(C.byref(s))
    text = fprint_text(gb, handle(gb, "GxB_TRIL"), tmp_path)
    assert "GxB_TRIL" in text and "user-defined" not in text, text


def test_source_holds_the_definition_and_the_kernel(gb):
    lib, d = gb.lib, gb._capi.constants
    fp64, int32 = handle(gb, "GrB_FP64"), handle(gb, "GrB_INT32")
    buf = C.create_string_buffer(1 << 16)
    texts = {}
    for on_vector in (0, 1):
        assert lib.GrBX_selectop_source(b"above", DEFN, fp64, int32, C.c_int(on_vector), buf, C.c_size_t(len(buf))) == 0
        texts[on_vector] = buf.value.decode()
        t = texts[on_vector]
        assert DEFN.decode() in t and "grb_userselect" in t and "typedef double X; typedef int K;" in t and "GrB_Index" in t
        assert "force_cuda_host_device begin" in t and t.index("force_cuda_host_device begin") < t.index(DEFN.decode()) < t.index("force_cuda_host_device end")
    assert texts[0] != texts[1]                                                    # one text per matrix | vector
    assert lib.GrBX_selectop_source(b"above", DEFN, fp64, None, C.c_int(0), buf, C.c_size_t(len(buf))) == 0
    assert "typedef double X; typedef double K;" in buf.value.decode()
    assert lib.GrBX_selectop_source(b"above", DEFN, fp64, None, C.c_int(0), buf, C.c_size_t(16)) == d["GrB_INSUFFICIENT_SPACE"]
    assert lib.GrBX_selectop_source(b"above", DEFN, handle(gb, "GxB_FC64"), None, C.c_int(0), buf, C.c_size_t(len(buf))) == d["GrB_DOMAIN_MISMATCH"]
    assert lib.GrBX_selectop_source(None, DEFN, fp64, None, C.c_int(0), buf, C.c_size_t(len(buf))) == d["GrB_NULL_POINTER"]
    # the unary / binary text and its kind range are what they were
    assert lib.GrBX_userop_source(b"f", b"void f (double *z, const double *x) { *z = *x; }", fp64, C.c_int(0), buf, C.c_size_t(len(buf))) == 0
    assert "grb_userop" in buf.value.decode() and "grb_userselect" not in buf.value.decode()
    assert lib.GrBX_userop_source(b"f", b"void f (double *z, const double *x) { *z = *x; }", fp64, C.c_int(5), buf, C.c_size_t(len(buf))) == d["GrB_DOMAIN_MISMATCH"]


def test_decorated_operator_object(gb):
    op = gb.select_op(gb.FP64)(band_above)
    assert isinstance(op, gb.SelectOp) and isinstance(op, gb.userop.UserSelectOp) and op.kind == "SelectOp"
    assert op.name == "band_above" and op.type is gb.FP64 and op.thunk_type is gb.FP64 and op.func is band_above and op.get_op()
    assert "bool band_above(GrB_Index i, GrB_Index j, const double *x, const double *thunk)" in op.defn and "(3LL)" in op.defn
    op2 = gb.select_op(gb.INT8, gb.INT64)(far_and_different)
    assert op2.type is gb.INT8 and op2.thunk_type is gb.INT64 and "const int8_t *x, const int64_t *thunk" in op2.defn
    assert op2.defn.index("static int64_t far_and_different__far_ii(") < op2.defn.index("bool far_and_different(")
    assert "select_op" in gb.__all__ and "SelectOp" in gb.__all__
    h = op.get_op()
    del op                                                                         # freed in __del__: nothing to observe but that it does not fail
    assert h


def test_running_one_without_a_device_fails_loudly(gb):
    if gb.device_info()["ok"]:
        pytest.skip("a HIP device is present")
    op = gb.select_op(gb.FP64)(band_above)
    m = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    for call in (lambda: m.select(op), lambda: m.select(op, 1.5), lambda: v.select(op), lambda: v.select(op, 1.5)):
        with pytest.raises(gb.Panic, match="no device"):
            call()
