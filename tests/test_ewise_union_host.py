"""GxB_Matrix_eWiseUnion / GxB_Vector_eWiseUnion without a device: the two symbols are exported, the argument checks that come before a device is asked for
(NULL, uninitialised, a scalar without an entry) answer in that order, and the Python surface exists and reaches the library."""
import ctypes as C

import pytest

NULL_POINTER, UNINITIALIZED, INVALID_VALUE = 4, 2, 5


def scalar(gb, typ, value=None):
    s = C.c_void_p()
    assert gb.lib.GxB_Scalar_new(C.byref(s), C.c_void_p(typ._h)) == 0
    if value is not None:
        assert getattr(gb.lib, "GxB_Scalar_setElement_" + typ.__name__)(s, typ._c(value)) == 0
    return s


def test_the_two_symbols_are_exported(gb):
    for f in ("GxB_Matrix_eWiseUnion", "GxB_Vector_eWiseUnion"):
        assert f in gb._capi.functions and hasattr(gb.lib, f)
    assert gb._capi.missing == []


def test_argument_checks_come_before_the_device(gb):
    A = gb.Matrix.from_lists([0, 1], [0, 1], [1.0, 2.0], 2, 2, gb.FP64); Cm = gb.Matrix.sparse(gb.FP64, 2, 2)
    u = gb.Vector.from_lists([0], [1.0], 2, gb.FP64); w = gb.Vector.sparse(gb.FP64, 2)
    op = C.c_void_p(gb.FP64.MINUS.get_op())
    one, empty = scalar(gb, gb.FP64, 1.0), scalar(gb, gb.FP64)
    for fn, out, x in ((gb.lib.GxB_Matrix_eWiseUnion, Cm, A), (gb.lib.GxB_Vector_eWiseUnion, w, u)):
        call = lambda c=out._h, o=op, a=x._h, al=one, b=x._h, be=one: fn(c, None, None, o, a, al, b, be, None)
        assert call(al=None) == NULL_POINTER and call(be=None) == NULL_POINTER, "a NULL alpha or beta"
        assert call(c=None) == NULL_POINTER and call(o=None) == NULL_POINTER and call(a=None) == NULL_POINTER and call(b=None) == NULL_POINTER
        assert call(al=None, be=empty) == NULL_POINTER, "NULL is looked for before the scalars' entries"
        assert call(al=empty) == INVALID_VALUE and call(be=empty) == INVALID_VALUE, "a scalar without an entry, without a device"
    for s in (one, empty):
        gb.lib.GxB_Scalar_free(C.byref(s))


def test_python_surface(gb):
    """Matrix.eunion / Vector.eunion exist, refuse what is not a binary operator, and reach the library: without a device they raise Panic like every compute call."""
    A = gb.Matrix.from_lists([0, 1], [0, 1], [1.0, 2.0], 2, 2, gb.FP64); B = gb.Matrix.from_lists([1], [1], [5.0], 2, 2, gb.FP64)
    u = gb.Vector.from_lists([0], [1.0], 2, gb.FP64); v = gb.Vector.from_lists([1], [3.0], 2, gb.FP64)
    for x, y in ((A, B), (u, v)):
        with pytest.raises(TypeError):
            x.eunion(y, gb.FP64.PLUS_MONOID, 0, 0)
        if gb.device_info()["ok"]:
            got = x.eunion(y, gb.FP64.MINUS, 0.5, -2.0)
            assert got.nvals == 2 and sorted(got.to_arrays()[-1].tolist()) == sorted([1.0 + 2.0, (2.0 - 5.0) if x is A else (0.5 - 3.0)])
            assert x.eunion(y, None, 0, 0).nvals == 2
        else:
            with pytest.raises(gb.base.Panic, match="no device"):
                x.eunion(y, gb.FP64.MINUS, 0.5, -2.0)
            with pytest.raises(gb.base.Panic, match="no device"):
                x.eunion(y, None, 0, 0)
