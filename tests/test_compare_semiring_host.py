"""Comparison semirings, the part that needs no device: the 300 handles GxB_{LOR,LAND,LXOR,EQ,ANY}_{EQ,NE,GT,LT,GE,LE}_{INT8..UINT64,FP32,FP64}, what introspection
returns for them (the BOOL monoid, the exported comparison GrB_<cmp>_<T>), the Python attributes with a BOOL result type, the refusals that are decided before a
device is asked for — GrB_DOMAIN_MISMATCH naming the semiring, output untouched — and the composition of the same two objects with GrB_Semiring_new, which is still
made.  The kernels are checked on the device, tests/test_compare_semiring_gpu.py."""
import ctypes as C
import itertools
import os

ADDS = ["LOR", "LAND", "LXOR", "EQ", "ANY"]
CMPS = ["EQ", "NE", "GT", "LT", "GE", "LE"]
TYPES = ["INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
ALL = list(itertools.product(ADDS, CMPS, TYPES))
MONOID = {"LOR": "GrB_LOR_MONOID_BOOL", "LAND": "GrB_LAND_MONOID_BOOL", "LXOR": "GrB_LXOR_MONOID_BOOL", "EQ": "GxB_EQ_BOOL_MONOID", "ANY": "GxB_ANY_BOOL_MONOID"}
MONOID_OP = {"LOR": "GxB_LOR_BOOL", "LAND": "GxB_LAND_BOOL", "LXOR": "GxB_LXOR_BOOL", "EQ": "GrB_LXNOR", "ANY": "GxB_ANY_BOOL"}      # the operators of those monoids
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_all_300_handles_are_declared_and_registered(gb):
    assert len(ALL) == 300
    with open(os.path.join(ROOT, "include", "grb_mi355x.h")) as f:
        header = f.read()
    names = set(gb._capi.names["GrB_Semiring"])
    for add, cmp_, t in ALL:
        cname = f"GxB_{add}_{cmp_}_{t}"
        assert cname in names, cname
        assert f"extern GrB_Semiring {cname};\n" in header, cname
        assert handle(gb, cname).value, cname
    assert len(names) == 1559 and not gb._capi.missing


def test_introspection_returns_the_bool_monoid_and_the_exported_comparison(gb, tmp_path):
    lib = gb.lib
    for add, cmp_, t in ALL:
        cname = f"GxB_{add}_{cmp_}_{t}"
        s = handle(gb, cname)
        m, b, op, zt, xt, yt = (C.c_void_p() for _ in range(6))
        assert lib.GxB_Semiring_add(C.byref(m), s) == 0 and m.value == handle(gb, MONOID[add]).value, cname
        assert lib.GxB_Semiring_multiply(C.byref(b), s) == 0 and b.value == handle(gb, f"GrB_{cmp_}_{t}").value, cname
        assert lib.GxB_Monoid_operator(C.byref(op), m) == 0 and op.value == handle(gb, MONOID_OP[add]).value, cname
        assert lib.GxB_BinaryOp_ztype(C.byref(zt), b) == 0 and zt.value == handle(gb, "GrB_BOOL").value, cname
        assert lib.GxB_BinaryOp_xtype(C.byref(xt), b) == 0 and lib.GxB_BinaryOp_ytype(C.byref(yt), b) == 0
        assert xt.value == yt.value == handle(gb, "GrB_" + t).value, cname
    for cname, addname, mulname in (("GxB_LOR_EQ_INT64", "GxB_LOR_BOOL", "GrB_EQ_INT64"), ("GxB_EQ_LE_FP32", "GrB_LXNOR", "GrB_LE_FP32"),
                                    ("GxB_ANY_NE_UINT8", "GxB_ANY_BOOL", "GrB_NE_UINT8")):
        text = fprint(gb, lib.GxB_Semiring_fprint, handle(gb, cname), tmp_path, cname)
        assert "Semiring" in text and "(built-in)" in text and addname in text and mulname in text, text
    keep = handle(gb, "GxB_LXOR_GT_FP64")
    h = C.c_void_p(keep.value)
    assert lib.GrB_Semiring_free(C.byref(h)) == 0 and h.value == keep.value      # built-in: left alone


def test_python_attributes_have_a_bool_result_type(gb):
    for add, cmp_, t in ALL:
        T = getattr(gb, t)
        sr = getattr(T, f"{add}_{cmp_}")
        assert isinstance(sr, gb.Semiring) and sr is getattr(T, f"{add}_{cmp_}".lower()), (add, cmp_, t)
        assert sr.cname == f"GxB_{add}_{cmp_}_{t}" and sr.name == f"{add}_{cmp_}"
        assert sr.ztype is gb.BOOL, (add, cmp_, t)
    assert gb.INT64.LOR_EQ is gb.INT64.lor_eq and gb.FP32.LAND_GT.ztype is gb.BOOL
    assert gb.BOOL.LOR_EQ.cname == "GxB_LOR_EQ_BOOL"                   # the _BOOL column is what it was
    assert not hasattr(gb.FP64, "LOR_ISEQ") and not hasattr(gb.INT8, "PLUS_EQ")


def test_hypersparse_and_complex_containers_are_refused_before_a_device(gb):
    lib, DM = gb.lib, gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    for cname in ("GxB_LOR_EQ_INT64", "GxB_LXOR_GT_FP32", "GxB_ANY_LE_UINT8"):
        s = handle(gb, cname)
        A = gb.Matrix.from_lists([0, 1], [1, 0], [1, 1], 2, 2, gb.INT64)
        u = gb.Vector.from_lists([0, 1], [1, 1], 2, gb.INT64)
        H = gb.Matrix.sparse(gb.INT64)                                   # 2^60 x 2^60
        H[3, 4] = 1
        hv = gb.Vector.sparse(gb.INT64)
        hv[5] = 1
        Hout = gb.Matrix.sparse(gb.BOOL)
        hw = gb.Vector.sparse(gb.BOOL)
        for call in (lambda: lib.GrB_mxm(Hout._h, None, None, s, H._h, H._h, None), lambda: lib.GrB_mxv(hw._h, None, None, s, H._h, hv._h, None),
                     lambda: lib.GrB_vxm(hw._h, None, None, s, hv._h, H._h, None)):
            assert call() == DM and cname in last_error(gb) and "hypersparse" in last_error(gb), last_error(gb)
        assert Hout.nvals == 0 and hw.nvals == 0
        # a hypersparse mask on containers with a layout is refused all the same (never reached as a dimension error)
        out, w = gb.Matrix.from_lists([0], [0], [True], 2, 2, gb.BOOL), gb.Vector.from_lists([1], [True], 2, gb.BOOL)
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
        assert out.to_lists() == [[0], [0], [True]] and w.to_lists() == [[1], [True]]
        lib.GrB_Matrix_free(C.byref(zh)); lib.GrB_Vector_free(C.byref(zv))


def test_the_same_two_objects_still_compose_with_semiring_new(gb):
    """GrB_Semiring_new(BOOL monoid, GrB_<cmp>_<T>) is made as before (info 0, a user object, not the built-in handle); what it answers at use is pinned by
    tests/test_operator_table_gpu.py::test_semiring_multipliers and not touched here."""
    lib = gb.lib
    for add, cmp_, t in (("LOR", "EQ", "INT32"), ("LXOR", "GT", "FP64"), ("ANY", "LE", "UINT64")):
        sr = C.c_void_p()
        assert lib.GrB_Semiring_new(C.byref(sr), handle(gb, MONOID[add]), handle(gb, f"GrB_{cmp_}_{t}")) == 0 and sr.value
        assert sr.value != handle(gb, f"GxB_{add}_{cmp_}_{t}").value
        m, b = C.c_void_p(), C.c_void_p()
        assert lib.GxB_Semiring_add(C.byref(m), sr) == 0 and m.value == handle(gb, MONOID[add]).value
        assert lib.GxB_Semiring_multiply(C.byref(b), sr) == 0 and b.value == handle(gb, f"GrB_{cmp_}_{t}").value
        assert lib.GrB_Semiring_free(C.byref(sr)) == 0 and sr.value is None
