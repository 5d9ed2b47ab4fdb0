"""User-defined monoids and semirings, the part that needs no device: construction, introspection, printing and release of the objects of
GrBX_Monoid_new_user / GrBX_Semiring_new_user in their three forms (all user-defined, user add with built-in multiply, built-in add with user multiply), every
refusal with the operator's name in GrBX_last_error, the unchanged refusals of GrB_Monoid_new_<T> / GrB_Semiring_new, the Python classmethods, and the generated
kernel text: the expression emitted for every built-in operator of the list, on every type, compiled for the host and compared bit for bit with
tests/operator_model.py on its edge values.  (The wave tree of the row kernel and the lanes of the product kernel are not run serially on the host: the kernels
themselves are checked on the device, tests/test_usersemiring_gpu.py.)"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import operator_model as om

DEFN_ADD = b"void myadd (double *z, const double *x, const double *y) { (*z) = (*x) + (*y) ; }"
DEFN_MUL = b"void mymul (double *z, const double *x, const double *y) { (*z) = (*x) * (*y) ; }"
CT = {"BOOL": C.c_bool, "INT8": C.c_int8, "UINT8": C.c_uint8, "INT16": C.c_int16, "UINT16": C.c_uint16, "INT32": C.c_int32, "UINT32": C.c_uint32,
      "INT64": C.c_int64, "UINT64": C.c_uint64, "FP32": C.c_float, "FP64": C.c_double}
LIST_OPS = ["FIRST", "SECOND", "PAIR", "PLUS", "MINUS", "TIMES", "MIN", "MAX"]
MARK = "// ---- kernel ----"


def handle(gb, name):
    return C.c_void_p(gb._capi.handle(name))


def last_error(gb):
    buf = C.create_string_buffer(1024)
    gb.lib.GrBX_last_error(buf, C.c_int(1024))
    return buf.value.decode()


def new_binop(gb, name, defn, typ="GrB_FP64"):
    h, t = C.c_void_p(), handle(gb, typ)
    assert gb.lib.GxB_BinaryOp_new(C.byref(h), None, t, t, t, name, defn) == 0
    return h


def fprint(gb, fn, obj, tmp_path, name):
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    path = tmp_path / (name + ".txt")
    f = C.c_void_p(libc.fopen(str(path).encode(), b"w"))
    assert f.value
    assert fn(obj, name.encode(), C.c_int(3), f) == 0
    libc.fclose(f)
    return path.read_text()


def test_objects_in_three_forms(gb, tmp_path):
    lib, d = gb.lib, gb._capi.constants
    add, mul = new_binop(gb, b"myadd", DEFN_ADD), new_binop(gb, b"mymul", DEFN_MUL)
    plus_monoid, times = handle(gb, "GrB_PLUS_MONOID_FP64"), handle(gb, "GrB_TIMES_FP64")
    ident = C.c_double(12.5)
    m = C.c_void_p()
    assert lib.GrBX_Monoid_new_user(C.byref(m), add, C.byref(ident)) == 0 and m.value
    forms = {"user_user": (m, mul, b"myadd", b"mymul"), "user_builtin": (m, times, b"myadd", b"TIMES"), "builtin_user": (plus_monoid, mul, b"PLUS", b"mymul")}
    for name, (mon, mult, add_name, mul_name) in forms.items():
        s = C.c_void_p()
        assert lib.GrBX_Semiring_new_user(C.byref(s), mon, mult) == 0 and s.value, name
        got_m, got_b, op = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.GxB_Semiring_add(C.byref(got_m), s) == 0 and got_m.value == mon.value
        assert lib.GxB_Semiring_multiply(C.byref(got_b), s) == 0 and got_b.value == mult.value
        assert lib.GxB_Monoid_operator(C.byref(op), got_m) == 0 and op.value == (add.value if mon is m else handle(gb, "GrB_PLUS_FP64").value)
        t = C.c_void_p()
        assert lib.GxB_BinaryOp_ztype(C.byref(t), got_b) == 0 and t.value == handle(gb, "GrB_FP64").value
        text = fprint(gb, lib.GxB_Semiring_fprint, s, tmp_path, name)
        assert "Semiring" in text and "(user)" in text and add_name.decode() in text and mul_name.decode() in text, text
        keep = s.value
        assert lib.GrB_Semiring_free(C.byref(s)) == 0 and s.value is None and keep
        assert lib.GrB_Semiring_free(C.byref(s)) == 0
    # the monoid: operator, identity, no terminal value, print, release
    x, has, term = C.c_double(0), C.c_bool(True), C.c_double(-1)
    assert lib.GxB_Monoid_identity(C.byref(x), m) == 0 and x.value == 12.5
    assert lib.GxB_Monoid_terminal(C.byref(has), C.byref(term), m) == 0 and has.value is False and term.value == -1
    text = fprint(gb, lib.GxB_Monoid_fprint, m, tmp_path, "monoid")
    assert "Monoid" in text and "(user)" in text and "myadd" in text and "12.5" in text and "terminal" not in text, text
    assert lib.GxB_Monoid_identity(C.byref(x), plus_monoid) == 0 and x.value == 0.0       # built-in monoids answer too
    assert lib.GrB_Monoid_free(C.byref(m)) == 0 and m.value is None
    assert lib.GrB_Monoid_free(C.byref(m)) == 0
    keep = plus_monoid.value                                                             # built-in handles stay untouched
    assert lib.GrB_Monoid_free(C.byref(plus_monoid)) == 0 and plus_monoid.value == keep
    sr = handle(gb, "GrB_PLUS_TIMES_SEMIRING_FP64")
    keep = sr.value
    assert lib.GrB_Semiring_free(C.byref(sr)) == 0 and sr.value == keep
    assert lib.GxB_Monoid_identity(C.byref(x), plus_monoid) == 0
    assert d["GrB_SUCCESS"] == 0
    lib.GrB_BinaryOp_free(C.byref(add)); lib.GrB_BinaryOp_free(C.byref(mul))


def test_every_refusal_names_the_operator(gb):
    lib, d = gb.lib, gb._capi.constants
    DM, NP_ = d["GrB_DOMAIN_MISMATCH"], d["GrB_NULL_POINTER"]
    add = new_binop(gb, b"myadd", DEFN_ADD)
    add32 = new_binop(gb, b"myadd32", b"void myadd32 (float *z, const float *x, const float *y) { (*z) = (*x) + (*y) ; }", "GrB_FP32")
    ident = C.c_double(0)
    m = C.c_void_p()
    # NULL arguments
    assert lib.GrBX_Monoid_new_user(None, add, C.byref(ident)) == NP_
    assert lib.GrBX_Monoid_new_user(C.byref(m), None, C.byref(ident)) == NP_
    assert lib.GrBX_Monoid_new_user(C.byref(m), add, None) == NP_ and m.value is None
    assert lib.GrBX_Monoid_new_user(C.byref(m), add, C.byref(ident)) == 0
    s = C.c_void_p()
    assert lib.GrBX_Semiring_new_user(None, m, add) == NP_
    assert lib.GrBX_Semiring_new_user(C.byref(s), None, add) == NP_
    assert lib.GrBX_Semiring_new_user(C.byref(s), m, None) == NP_ and s.value is None
    # a comparison, a built-in outside the list: the monoid.  (A complex operator cannot be handed over at all: the library exports no built-in binary operator
    # on a complex type, and GxB_BinaryOp_new refuses to make one — tests/test_userop_host.py.)
    m2 = C.c_void_p()
    for cname, word in (("GrB_EQ_FP64", "EQ"), ("GrB_LT_INT32", "LT"), ("GrB_DIV_FP64", "DIV"), ("GxB_ANY_FP64", "ANY"), ("GxB_ISEQ_FP64", "ISEQ"),
                        ("GrB_BOR_UINT8", "BOR"), ("GxB_LOR_FP64", "LOR"), ("GxB_POW_FP64", "POW"), ("GxB_RMINUS_FP64", "RMINUS"), ("GrB_LXNOR", "LXNOR")):
        assert lib.GrBX_Monoid_new_user(C.byref(m2), handle(gb, cname), C.byref(ident)) == DM and m2.value is None, cname
        assert word in last_error(gb), (cname, last_error(gb))
        # ... and the same operators as a multiplier
        assert lib.GrBX_Semiring_new_user(C.byref(s), m, handle(gb, cname)) == DM and s.value is None, cname
        assert word in last_error(gb), (cname, last_error(gb))
    # differing types: a user multiplier of another type, a built-in multiplier of another type, a built-in monoid of another type
    assert lib.GrBX_Semiring_new_user(C.byref(s), m, add32) == DM and s.value is None and "myadd32" in last_error(gb)
    assert lib.GrBX_Semiring_new_user(C.byref(s), m, handle(gb, "GrB_TIMES_INT64")) == DM and s.value is None and "TIMES_INT64" in last_error(gb)
    assert lib.GrBX_Semiring_new_user(C.byref(s), handle(gb, "GrB_PLUS_MONOID_INT32"), add) == DM and s.value is None and "myadd" in last_error(gb)
    # a built-in monoid outside the list
    assert lib.GrBX_Semiring_new_user(C.byref(s), handle(gb, "GxB_ANY_FP64_MONOID"), add) == DM and s.value is None and "ANY" in last_error(gb)
    # GrB_Monoid_new_<T> and GrB_Semiring_new still refuse a user-defined operator
    assert lib.GrB_Monoid_new_FP64(C.byref(m2), add, C.c_double(0)) == DM and m2.value is None and "myadd" in last_error(gb)
    assert lib.GrB_Monoid_new_FP32(C.byref(m2), add32, C.c_float(0)) == DM and m2.value is None and "myadd32" in last_error(gb)
    assert lib.GrB_Semiring_new(C.byref(s), handle(gb, "GrB_PLUS_MONOID_FP64"), add) == DM and s.value is None and "myadd" in last_error(gb)
    lib.GrB_Monoid_free(C.byref(m)); lib.GrB_BinaryOp_free(C.byref(add)); lib.GrB_BinaryOp_free(C.byref(add32))


def test_grb_semiring_new_over_such_a_monoid_is_checked_when_it_runs(gb):
    """GrB_Semiring_new accepts any monoid — one made by GrBX_Monoid_new_user too — and any built-in multiplier of its type.  Such a semiring takes the compiled
    route (the monoid decides), which expresses only the operators of the list: any other multiplier is GrB_DOMAIN_MISMATCH naming it when the semiring is used,
    before a device is asked for, with the output untouched — never another operator's result."""
    lib, d = gb.lib, gb._capi.constants
    DM = d["GrB_DOMAIN_MISMATCH"]
    add = new_binop(gb, b"myadd", DEFN_ADD)
    cases = [("GrB_PLUS_FP64", C.c_double(0), "FP64", ["GrB_DIV_FP64", "GxB_ANY_FP64", "GxB_RMINUS_FP64", "GxB_ISEQ_FP64", "GxB_POW_FP64"]),
             ("GrB_LOR", C.c_bool(False), "BOOL", ["GrB_LT_FP64", "GrB_EQ_INT32", "GrB_LXNOR"]),
             ("GrB_PLUS_UINT8", C.c_uint8(0), "UINT8", ["GrB_BOR_UINT8", "GrB_DIV_UINT8"]),
             (add, C.c_double(0), "FP64", ["GrB_DIV_FP64", "GxB_ANY_FP64"])]
    for op, ident, typ, muls in cases:
        T = getattr(gb, typ)
        m = C.c_void_p()
        assert lib.GrBX_Monoid_new_user(C.byref(m), op if isinstance(op, C.c_void_p) else handle(gb, op), C.byref(ident)) == 0
        A = gb.Matrix.from_lists([0, 1], [1, 0], [1, 1], 2, 2, T)
        v = gb.Vector.from_lists([0, 1], [1, 1], 2, T)
        for mul in muls:
            s = C.c_void_p()
            assert lib.GrB_Semiring_new(C.byref(s), m, handle(gb, mul)) == 0 and s.value, (op, mul)
            out = gb.Matrix.from_lists([0], [0], [1], 2, 2, T)
            w = gb.Vector.from_lists([1], [1], 2, T)
            word = mul.split("_")[1]
            assert lib.GrB_mxm(out._h, None, None, s, A._h, A._h, None) == DM and word in last_error(gb), (mul, last_error(gb))
            assert lib.GrB_mxv(w._h, None, None, s, A._h, v._h, None) == DM and word in last_error(gb), (mul, last_error(gb))
            assert lib.GrB_vxm(w._h, None, None, s, v._h, A._h, None) == DM and word in last_error(gb), (mul, last_error(gb))
            assert out.to_lists() == [[0], [0], [1]] and w.to_lists() == [[1], [1]]
            assert lib.GrB_Semiring_free(C.byref(s)) == 0
        # a multiplier of the list is let through: the call gets as far as the device
        s = C.c_void_p()
        times = {"FP64": "GrB_TIMES_FP64", "BOOL": "GrB_LAND", "UINT8": "GrB_TIMES_UINT8"}[typ]
        assert lib.GrB_Semiring_new(C.byref(s), m, handle(gb, times)) == 0
        out = gb.Matrix.sparse(T, 2, 2)
        info = lib.GrB_mxm(out._h, None, None, s, A._h, A._h, None)
        if gb.device_info()["ok"]:
            assert info == 0 and out.to_lists() == [[0, 1], [0, 1], [1, 1]] and gb.last_kernel_plan().startswith("usersr<")
        else:
            assert info == d["GrB_PANIC"]
        lib.GrB_Semiring_free(C.byref(s)); lib.GrB_Monoid_free(C.byref(m))
    lib.GrB_BinaryOp_free(C.byref(add))


def f_add(x, y):
    return x + y


def f_mul(x, y):
    return x * y


def test_python_classmethods(gb):
    add, mul = gb.binary_op(gb.FP64)(f_add), gb.binary_op(gb.FP64)(f_mul)
    mon = gb.FP64.new_monoid(add, 0.0)
    assert isinstance(mon, gb.userop.UserMonoid) and isinstance(mon, gb.types.Monoid) and mon.op is add and mon.get_op()
    sr = gb.FP64.new_semiring(mon, mul)
    assert isinstance(sr, gb.userop.UserSemiring) and isinstance(sr, gb.types.Semiring) and sr.monoid is mon and sr.op is mul and sr.get_op()
    assert sr.ztype is gb.FP64
    with sr:
        assert gb.types.current_semiring.get() is sr
    assert gb.types.current_semiring.get(None) is None
    with mon:
        assert gb.types.current_monoid.get() is mon
    mixed = gb.FP64.new_semiring(mon, gb.FP64.TIMES), gb.FP64.new_semiring(gb.FP64.PLUS_MONOID, mul), gb.INT8.new_semiring(gb.INT8.new_monoid(gb.INT8.MAX, -128), gb.INT8.PLUS)
    assert all(isinstance(s, gb.types.Semiring) for s in mixed)
    for bad in (gb.FP64.DIV, gb.FP64.ANY, gb.FP64.ISEQ, gb.FP64.EQ, gb.FP64.LOR):
        with pytest.raises(gb.DomainMismatch, match=bad.name):
            gb.FP64.new_monoid(bad, 0.0)
        with pytest.raises(gb.DomainMismatch, match=bad.name):
            gb.FP64.new_semiring(mon, bad)
    with pytest.raises(gb.DomainMismatch, match="f_mul"):
        gb.INT64.new_semiring(gb.INT64.PLUS_MONOID, mul)                    # differing types
    # the operator's type is the class's: the identity is packed as the class's C type
    add32 = gb.binary_op(gb.FP32)(f_add)
    with pytest.raises(gb.DomainMismatch, match="f_add"):
        gb.FP32.new_monoid(add, 0.0)
    with pytest.raises(gb.DomainMismatch, match="f_add"):
        gb.FP64.new_monoid(add32, 0.0)
    with pytest.raises(gb.DomainMismatch, match="PLUS"):
        gb.FP32.new_monoid(gb.FP64.PLUS, 0.0)
    with pytest.raises(gb.DomainMismatch):
        gb.FP32.new_semiring(mon, mul)
    with pytest.raises(TypeError):
        gb.FP64.new_monoid(gb.FP64.AINV, 0.0)
    del sr, mixed, mon                                                      # collection frees the handles (semirings first, then what they point to)


# ---- the generated text --------------------------------------------------------------------------------------------------------------------------------
def source(gb, monoid, mul, kind):
    buf = C.create_string_buffer(1 << 16)
    assert gb.lib.GrBX_usersr_source(monoid, mul, C.c_int(kind), buf, C.c_size_t(1 << 16)) == 0, last_error(gb)
    return buf.value.decode()


def test_text_of_the_kernels(gb):
    add, mul = new_binop(gb, b"myadd", DEFN_ADD), new_binop(gb, b"mymul", DEFN_MUL)
    m, ident = C.c_void_p(), C.c_double(0)
    assert gb.lib.GrBX_Monoid_new_user(C.byref(m), add, C.byref(ident)) == 0
    texts = [source(gb, m, mul, k) for k in range(3)] + [source(gb, m, None, 3)]
    assert len(set(texts)) == 4                                            # the kind — and with it the argument order — is part of the text, so of the cache key
    mxv, vxm, mxm, red = texts
    for t in texts:
        assert MARK in t and "myadd" in t and "typedef double T;" in t
        assert "asm" not in t                                              # plain C++ only
    assert "grb_usersr_rows" in mxv and "grb_usersr_rows" in vxm and "grb_usersr_rows" in red and "grb_usersr_product" in mxm
    assert "#define GRB_KIND 0" in mxv and "#define GRB_KIND 1" in vxm and "#define GRB_KIND 2" in mxm and "#define GRB_KIND 3" in red
    assert "grb_mul_f(u, a)" in vxm and "grb_mul_f(a, u)" in vxm           # both orders are in the text; GRB_KIND picks one at compile time
    assert "mymul" in mxv and "mymul" not in red
    assert "__syncthreads" not in mxm and "__threadfence_block" in mxm     # waves of a workgroup walk rows of different lengths
    # another type or another operator: another text
    assert source(gb, m, handle(gb, "GrB_TIMES_FP64"), 0) != mxv
    assert gb.lib.GrBX_usersr_source(m, None, C.c_int(0), C.create_string_buffer(16), C.c_size_t(16)) == gb._capi.constants["GrB_NULL_POINTER"]
    assert gb.lib.GrBX_usersr_source(m, mul, C.c_int(0), C.create_string_buffer(16), C.c_size_t(16)) == gb._capi.constants["GrB_INSUFFICIENT_SPACE"]
    assert gb.lib.GrBX_usersr_source(m, mul, C.c_int(4), C.create_string_buffer(16), C.c_size_t(16)) == gb._capi.constants["GrB_INVALID_VALUE"]
    gb.lib.GrB_Monoid_free(C.byref(m)); gb.lib.GrB_BinaryOp_free(C.byref(add)); gb.lib.GrB_BinaryOp_free(C.byref(mul))


@pytest.fixture(scope="module")
def cxx():
    # the compiler on the PATH, else the clang++ of the ROCm installation the build itself needs: this check is never skipped
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    exe = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm if os.path.exists(rocm) else None)
    assert exe is not None, "no host C++ compiler: neither c++ / g++ / clang++ on the PATH nor " + rocm
    return exe


def test_emitted_builtin_expressions_match_the_operator_model(gb, cxx, tmp_path):
    """Every built-in operator of the list on every type: the operator section of the reduce_rows text (the monoid's operator alone), each in a namespace of its
    own, compiled once for the host; f(a, b) over all pairs of the model's edge values must be one of the model's accepted results, bit for bit."""
    cases = [(t, op) for t in om.TYPES for op in LIST_OPS + (["LOR", "LAND", "LXOR"] if t == "BOOL" else [])]
    parts = ["#include <cmath>\n#include <cstdint>\n#include <cstring>\n"]
    monoids = []
    for n, (t, op) in enumerate(cases):
        T = getattr(gb, t)
        m, ident = C.c_void_p(), CT[t](0)
        assert gb.lib.GrBX_Monoid_new_user(C.byref(m), C.c_void_p(getattr(T, op).get_op()), C.byref(ident)) == 0, (t, op, last_error(gb))
        monoids.append(m)
        text = source(gb, m, None, 3)
        section = text[:text.index(MARK)]
        assert "grb_add_f" in section
        parts.append(f"namespace case{n} {{\n{section}\n}}\nextern \"C\" void f{n}(void* z, const void* a, const void* b) {{ case{n}::T x, y, r; "
                     f"memcpy(&x, a, sizeof x); memcpy(&y, b, sizeof y); r = case{n}::grb_add_f(x, y); memcpy(z, &r, sizeof r); }}\n")
    src, so = tmp_path / "exprs.cpp", tmp_path / "exprs.so"
    src.write_text("".join(parts))
    subprocess.check_call([cxx, "-O1", "-ffp-contract=off", "-w", "-D__device__=", "-D__forceinline__=inline", "-shared", "-fPIC", "-o", str(so), str(src), "-lm"])
    dll = C.CDLL(str(so))
    checked = 0
    for n, (t, op) in enumerate(cases):
        fn = getattr(dll, f"f{n}")
        fn.restype = None
        ct, npt = CT[t], om.NP[t]
        for a, b in itertools.product(om.edge_values(t), repeat=2):
            x, y, z = ct(a), ct(b), ct()
            fn(C.byref(z), C.byref(x), C.byref(y))
            got = bool(z.value) if t == "BOOL" else (npt(z.value) if om.is_fp(t) else int(z.value))
            want = om.binop(op, t, a, b)
            assert om.accepted(got, want), (t, op, a, b, got, want)
            checked += 1
    assert checked > 10000
    for m in monoids:
        gb.lib.GrB_Monoid_free(C.byref(m))


def test_running_one_without_a_device_fails_loudly(gb):
    if gb.device_info()["ok"]:
        pytest.skip("a HIP device is present")
    add, mul = gb.binary_op(gb.FP64)(f_add), gb.binary_op(gb.FP64)(f_mul)
    mon = gb.FP64.new_monoid(add, 0.0)
    sr = gb.FP64.new_semiring(mon, mul)
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    for call in (lambda: A.mxm(A, sr), lambda: A.mxv(v, sr), lambda: v.vxm(A, sr), lambda: A.reduce_vector(mon)):
        with pytest.raises(gb.Panic, match="no device"):
            call()
