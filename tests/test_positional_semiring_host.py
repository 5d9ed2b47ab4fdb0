"""Positional semirings, the part that needs no device: the 80 handles GxB_{MIN,MAX,ANY,PLUS,TIMES}_{FIRSTI..SECONDJ1}_{INT32,INT64} and what introspection
returns for them (the built-in monoid; an internal multiplier with the right name, type and print-out), the exported binary-operator set left as it was, the
Python attributes, and every refusal that is decided before a device is asked for: GrB_DOMAIN_MISMATCH naming the semiring (or its multiplier), output untouched.
The kernels are checked on the device, tests/test_positional_semiring_gpu.py."""
import ctypes as C
import itertools

ADDS = ["MIN", "MAX", "ANY", "PLUS", "TIMES"]
MULS = ["FIRSTI", "FIRSTI1", "FIRSTJ", "FIRSTJ1", "SECONDI", "SECONDI1", "SECONDJ", "SECONDJ1"]
TYPES = ["INT32", "INT64"]
ALL = list(itertools.product(ADDS, MULS, TYPES))
EXPORTED_BINARY_OPERATORS = 380      # the handles `extern GrB_BinaryOp ...;` of the header before the positional semirings existed


def handle(gb, name):
    return C.c_void_p(gb._capi.handle(name))


def last_error(gb):
    buf = C.create_string_buffer(1024)
    gb.lib.GrBX_last_error(buf, C.c_int(1024))
    return buf.value.decode()


def fprint(gb, fn, obj, tmp_path, name):
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    path = tmp_path / (name + ".txt")
    f = C.c_void_p(libc.fopen(str(path).encode(), b"w"))
    assert f.value
    assert fn(obj, name.encode(), C.c_int(3), f) == 0
    libc.fclose(f)
    return path.read_text()


def multiplier(gb, add, mul, t):
    b = C.c_void_p()
    assert gb.lib.GxB_Semiring_multiply(C.byref(b), handle(gb, f"GxB_{add}_{mul}_{t}")) == 0 and b.value
    return b


def test_all_80_handles_and_their_introspection(gb, tmp_path):
    lib = gb.lib
    assert len(ALL) == 80
    muls_seen = {}
    for add, mul, t in ALL:
        cname = f"GxB_{add}_{mul}_{t}"
        assert cname in gb._capi.names["GrB_Semiring"], cname
        s = handle(gb, cname)
        assert s.value, cname
        m, b, zt, xt, yt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        monoid = f"GxB_ANY_{t}_MONOID" if add == "ANY" else f"GrB_{add}_MONOID_{t}"      # the built-in monoid of that type: the object every other semiring of the type points to
        assert lib.GxB_Semiring_add(C.byref(m), s) == 0 and m.value == handle(gb, monoid).value, cname
        other = C.c_void_p()
        assert lib.GxB_Semiring_add(C.byref(other), handle(gb, f"GxB_{add}_SECOND_{t}")) == 0 and other.value == m.value
        assert lib.GxB_Semiring_multiply(C.byref(b), s) == 0 and b.value, cname
        assert lib.GxB_BinaryOp_ztype(C.byref(zt), b) == 0 and zt.value == handle(gb, "GrB_" + t).value, cname
        assert lib.GxB_BinaryOp_xtype(C.byref(xt), b) == 0 and lib.GxB_BinaryOp_ytype(C.byref(yt), b) == 0 and xt.value == yt.value == zt.value
        muls_seen.setdefault((mul, t), b.value)
        assert muls_seen[(mul, t)] == b.value                     # one internal object per (multiplier, type), shared by the five monoids
    assert len(set(muls_seen.values())) == 16
    for (mul, t), b in muls_seen.items():
        text = fprint(gb, lib.GxB_BinaryOp_fprint, C.c_void_p(b), tmp_path, f"op_{mul}_{t}")
        assert f"GxB_{mul}_{t}" in text and "(built-in)" in text and f"z:GrB_{t}" in text, text
    text = fprint(gb, lib.GxB_Semiring_fprint, handle(gb, "GxB_MIN_SECONDI1_INT64"), tmp_path, "sr")
    assert "Semiring" in text and "(built-in)" in text and "GrB_MIN_INT64" in text and "GxB_SECONDI1_INT64" in text, text
    keep = handle(gb, "GxB_ANY_SECONDI_INT64")
    h = C.c_void_p(keep.value)
    assert lib.GrB_Semiring_free(C.byref(h)) == 0 and h.value == keep.value      # built-in: left alone


def test_no_binary_operator_handle_leaked(gb):
    names = gb._capi.names["GrB_BinaryOp"]
    assert len(names) == EXPORTED_BINARY_OPERATORS
    assert not [n for n in names if any(w in n for w in ("FIRSTI", "FIRSTJ", "SECONDI", "SECONDJ"))]
    for mul, t in itertools.product(MULS, TYPES):
        assert not hasattr(gb.lib, f"GxB_{mul}_{t}"), (mul, t)      # no such symbol in the library either
        assert not hasattr(getattr(gb, t), mul)                     # ... and no Python binary operator


def test_python_attributes(gb):
    for add, mul, t in ALL:
        T = getattr(gb, t)
        sr = getattr(T, f"{add}_{mul}")
        assert isinstance(sr, gb.Semiring) and sr is getattr(T, f"{add}_{mul}".lower()) and sr.ztype is T and sr.cname == f"GxB_{add}_{mul}_{t}"
    assert gb.INT64.MIN_SECONDI1.name == "MIN_SECONDI1"              # the multiplier's digit is part of its name
    assert not hasattr(gb.FP64, "MIN_SECONDI") and not hasattr(gb.UINT64, "ANY_FIRSTJ")


def test_the_multiplier_is_refused_everywhere_else(gb):
    """GrB_Semiring_new, GrBX_Semiring_new_user, GrBX_Monoid_new_user, GrB_Monoid_new_<T>, the dup operator of build and an accumulator: GrB_DOMAIN_MISMATCH
    naming the operator, nothing made, nothing written."""
    lib, DM = gb.lib, gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    for mul, t in (("FIRSTI", "INT64"), ("SECONDJ1", "INT32"), ("SECONDI", "INT64")):
        b, name = multiplier(gb, "MIN", mul, t), f"GxB_{mul}_{t}"
        s, m = C.c_void_p(), C.c_void_p()
        assert lib.GrB_Semiring_new(C.byref(s), handle(gb, f"GrB_PLUS_MONOID_{t}"), b) == DM and s.value is None and name in last_error(gb), last_error(gb)
        assert lib.GrBX_Semiring_new_user(C.byref(s), handle(gb, f"GrB_PLUS_MONOID_{t}"), b) == DM and s.value is None and name in last_error(gb), last_error(gb)
        zero = (C.c_int64 if t == "INT64" else C.c_int32)(0)
        assert lib.GrBX_Monoid_new_user(C.byref(m), b, C.byref(zero)) == DM and m.value is None and name in last_error(gb), last_error(gb)
        assert getattr(lib, "GrB_Monoid_new_" + t)(C.byref(m), b, zero) == DM and m.value is None and name in last_error(gb), last_error(gb)
        # dup of build: the duplicates are never combined
        T = getattr(gb, t)
        A, v = gb.Matrix.sparse(T, 3, 3), gb.Vector.sparse(T, 3)
        I, X = (C.c_uint64 * 2)(1, 1), (zero.__class__ * 2)(5, 6)
        assert getattr(lib, "GrB_Matrix_build_" + t)(A._h, I, I, X, C.c_uint64(2), b) == DM and name in last_error(gb) and A.nvals == 0
        assert getattr(lib, "GrB_Vector_build_" + t)(v._h, I, X, C.c_uint64(2), b) == DM and name in last_error(gb) and v.nvals == 0
        # an accumulator, on a route that runs on the host mirror
        w, u = gb.Vector.from_lists([0, 2], [7, 9], 3, T), gb.Vector.from_lists([0, 1, 2], [1, 2, 3], 3, T)
        assert lib.GrB_Vector_assign(w._h, None, b, u._h, gb._capi.all_indices(), C.c_uint64(3), None) == DM and name in last_error(gb), last_error(gb)
        assert w.to_lists() == [[0, 2], [7, 9]]


def test_hypersparse_and_complex_containers_are_refused_before_a_device(gb):
    lib, DM = gb.lib, gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    for cname in ("GxB_MIN_SECONDI_INT64", "GxB_PLUS_FIRSTJ1_INT32", "GxB_ANY_FIRSTI_INT64"):
        s = handle(gb, cname)
        A = gb.Matrix.from_lists([0, 1], [1, 0], [1, 1], 2, 2, gb.INT64)
        u = gb.Vector.from_lists([0, 1], [1, 1], 2, gb.INT64)
        H = gb.Matrix.sparse(gb.INT64)                                   # 2^60 x 2^60
        H[3, 4] = 1
        hv = gb.Vector.sparse(gb.INT64)
        hv[5] = 1
        Hout = gb.Matrix.sparse(gb.INT64)
        hw = gb.Vector.sparse(gb.INT64)
        for call in (lambda: lib.GrB_mxm(Hout._h, None, None, s, H._h, H._h, None), lambda: lib.GrB_mxv(hw._h, None, None, s, H._h, hv._h, None),
                     lambda: lib.GrB_vxm(hw._h, None, None, s, hv._h, H._h, None)):
            assert call() == DM and cname in last_error(gb) and "hypersparse" in last_error(gb), last_error(gb)
        assert Hout.nvals == 0 and hw.nvals == 0
        # a hypersparse mask on containers with a layout is refused all the same (never reached as a dimension error)
        out, w = gb.Matrix.from_lists([0], [0], [7], 2, 2, gb.INT64), gb.Vector.from_lists([1], [7], 2, gb.INT64)
        assert lib.GrB_mxm(out._h, H._h, None, s, A._h, A._h, None) == DM and cname in last_error(gb)
        assert lib.GrB_mxv(w._h, hv._h, None, s, A._h, u._h, None) == DM and cname in last_error(gb)
        # complex: an operand, the output, the mask
        zh, zv, t = C.c_void_p(), C.c_void_p(), handle(gb, "GxB_FC64")
        assert lib.GrB_Matrix_new(C.byref(zh), t, C.c_uint64(2), C.c_uint64(2)) == 0 and lib.GrB_Vector_new(C.byref(zv), t, C.c_uint64(2)) == 0
        for call in (lambda: lib.GrB_mxm(out._h, None, None, s, zh, A._h, None), lambda: lib.GrB_mxm(out._h, None, None, s, A._h, zh, None),
                     lambda: lib.GrB_mxm(zh, None, None, s, A._h, A._h, None), lambda: lib.GrB_mxm(out._h, zh, None, s, A._h, A._h, None),
                     lambda: lib.GrB_mxv(w._h, None, None, s, zh, u._h, None), lambda: lib.GrB_vxm(w._h, None, None, s, u._h, zh, None),
                     lambda: lib.GrB_mxv(w._h, None, None, s, A._h, zv, None), lambda: lib.GrB_mxv(zv, None, None, s, A._h, u._h, None),
                     lambda: lib.GrB_vxm(w._h, zv, None, s, u._h, A._h, None)):
            assert call() == DM and cname in last_error(gb) and "complex" in last_error(gb), last_error(gb)
        assert out.to_lists() == [[0], [0], [7]] and w.to_lists() == [[1], [7]]
        lib.GrB_Matrix_free(C.byref(zh)); lib.GrB_Vector_free(C.byref(zv))


def test_elementwise_and_kronecker_refuse_the_semiring(gb):
    lib, DM = gb.lib, gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    for cname in ("GxB_MIN_SECONDI_INT64", "GxB_TIMES_FIRSTI1_INT32", "GxB_ANY_SECONDJ_INT64"):
        s = handle(gb, cname)
        A = gb.Matrix.from_lists([0, 1], [1, 0], [1, 1], 2, 2, gb.INT64)
        u = gb.Vector.from_lists([0, 1], [1, 1], 2, gb.INT64)
        out, w, K = gb.Matrix.from_lists([0], [0], [7], 2, 2, gb.INT64), gb.Vector.from_lists([1], [7], 2, gb.INT64), gb.Matrix.from_lists([0], [0], [7], 4, 4, gb.INT64)
        for fn, args, word in ((lib.GrB_Matrix_eWiseAdd_Semiring, (out._h, None, None, s, A._h, A._h, None), "eWiseAdd"),
                               (lib.GrB_Matrix_eWiseMult_Semiring, (out._h, None, None, s, A._h, A._h, None), "eWiseMult"),
                               (lib.GrB_Vector_eWiseAdd_Semiring, (w._h, None, None, s, u._h, u._h, None), "eWiseAdd"),
                               (lib.GrB_Vector_eWiseMult_Semiring, (w._h, None, None, s, u._h, u._h, None), "eWiseMult"),
                               (lib.GrB_Matrix_kronecker_Semiring, (K._h, None, None, s, A._h, A._h, None), "kronecker")):
            assert fn(*args) == DM and cname in last_error(gb) and word in last_error(gb), (cname, word, last_error(gb))
        assert out.to_lists() == [[0], [0], [7]] and w.to_lists() == [[1], [7]] and K.to_lists() == [[0], [0], [7]]
