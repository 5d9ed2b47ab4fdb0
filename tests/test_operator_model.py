"""tests/operator_model.py pinned without a GPU: against the C oracle (itself pinned to the reference's golden vectors), against tests/companion_model.py
on the operators both know, against hand-written facts for the rules that are not plain C, and against the monoid laws."""
import math

import numpy as np
import pytest

from oracle import oracle as O
import companion_model as CM
import operator_model as M

INF, NAN = math.inf, math.nan
# The oracle evaluates all 29 operators of oracle.OPS on BOOL; on the other types it has no POW and no LXNOR (its switch falls through to zero), so
# those two are pinned by the hand-written facts instead.
ORACLE_MULS = {t: [op for op in O.OPS if t == "BOOL" or op not in ("POW", "LXNOR")] for t in M.TYPES}
ORACLE_ADDS = {t: [op for op in M.monoids_of(t) if op in O.OPS] for t in M.TYPES}


def to_np(t, v):
    return np.array([v], M.NP[t])


def from_np(t, x):
    x = x[0]
    return bool(x) if t == "BOOL" else (int(x) if M.is_int(t) else x)


@pytest.mark.parametrize("t", M.TYPES)
def test_binops_against_the_oracle_on_1x1_products(t):
    """oracle.mxm on 1 x 1 operands is one product and no reduction: every multiplier the oracle knows, all ordered pairs of the edge values."""
    E = M.edge_values(t); add = ORACLE_ADDS[t][0]; z = np.zeros(1, np.uint64); n = 0
    for mul in ORACLE_MULS[t]:
        for a in E:
            A = O.Tuples(t, 1, 1, z, z, to_np(t, a))
            for b in E:
                got = O.mxm(O.Tuples(t, 1, 1), A, O.Tuples(t, 1, 1, z, z, to_np(t, b)), add, mul, t)
                assert got.nvals == 1
                exp = M.binop(mul, t, a, b)
                if mul in M.CMP and t != "BOOL":                       # (the oracle keeps a comparison's 0 / 1 in the semiring's type)
                    exp = tuple(M.cast("BOOL", t, r) for r in exp)
                assert M.accepted(from_np(t, got.X), exp), (mul, t, a, b, got.X[0], exp)
                n += 1
    assert n == len(ORACLE_MULS[t]) * len(E) ** 2


@pytest.mark.parametrize("t", M.TYPES)
def test_monoid_folds_against_the_oracle_on_1xk_products(t):
    """A 1 x k by k x 1 product with FIRST as the multiplier reduces the row's k values with the monoid: k = 2 over all ordered pairs, and the whole edge set."""
    E = M.edge_values(t)
    rows = [[a, b] for a in E for b in E] + [E, E[::-1]]
    for add in ORACLE_ADDS[t]:
        for vals in rows:
            k = len(vals); idx = np.arange(k, dtype=np.uint64); z = np.zeros(k, np.uint64)
            A = O.Tuples(t, 1, k, z, idx, np.array(vals, M.NP[t])); B = O.Tuples(t, k, 1, idx, z, np.array(vals, M.NP[t]))
            got = O.mxm(O.Tuples(t, 1, 1), A, B, add, "FIRST", t)
            assert got.nvals == 1 and M.accepted(from_np(t, got.X), M.fold(add, t, vals)), (add, t, vals, got.X[0])


@pytest.mark.parametrize("ft", M.TYPES)
def test_casts_against_the_oracle(ft):
    """The oracle casts the operands into the semiring's type and the product into the output's: FIRST on 1 x 1 operands is cast(ft -> st -> ot)."""
    z = np.zeros(1, np.uint64)
    for st in M.TYPES:
        for a in M.edge_values(ft):
            got = O.mxm(O.Tuples(st, 1, 1), O.Tuples(ft, 1, 1, z, z, to_np(ft, a)), O.Tuples(st, 1, 1, z, z, to_np(st, M.edge_values(st)[0])),
                        ORACLE_ADDS[st][0], "FIRST", st)
            assert M.same(from_np(st, got.X), M.cast(ft, st, a)), (ft, st, a, got.X[0])


def test_against_the_companion_model():
    for t in M.TYPES:
        E = M.edge_values(t)
        if t == "BOOL":
            continue                                                    # (the companion model has no BOOL renaming: it wraps Python arithmetic)
        for op in ("PLUS", "MINUS", "TIMES", "DIV", "FIRST", "SECOND"):
            for a in E:
                for b in E:
                    if op == "DIV" and (b == 0 or M.is_int(t) and (abs(a) >= 2 ** 53 or abs(b) >= 2 ** 53)):
                        continue                                        # (it says of itself: no zero divisors; and it divides through a double)
                    if M.is_fp(t) and (op in ("PLUS", "MINUS", "TIMES", "DIV")) and t == "FP32":
                        continue                                        # (it computes FP32 in double without rounding)
                    try:
                        with np.errstate(all="ignore"):
                            exp = CM.binop(op, t, float(a) if M.is_fp(t) else a, float(b) if M.is_fp(t) else b)
                    except (OverflowError, ValueError, ZeroDivisionError):
                        continue
                    assert M.accepted(exp, M.binop(op, t, a, b)), (op, t, a, b, exp)
        for op in ("AINV", "ABS", "IDENTITY", "ONE"):
            for a in E:
                assert M.accepted(CM.unop(op, t, float(a) if M.is_fp(t) else a), M.unop(op, t, a)), (op, t, a)
        for a in E:                                                     # MINV where the companion model's own division is defined and exact
            if M.is_int(t) and a != 0 and abs(a) < 2 ** 53:
                assert M.accepted(CM.unop("MINV", t, a), M.unop("MINV", t, a)), (t, a)
        for tt in M.INT_TYPES:                                          # integer -> integer casts: both wrap
            if M.is_int(t):
                for a in E:
                    assert CM.wrap(tt, a) == M.cast(t, tt, a)


def test_hand_written_facts_for_the_rules_that_are_not_plain_c():
    one = lambda r: r[0] if len(r) == 1 else pytest.fail(f"not unique: {r}")
    # integer division: x / 0 saturates by the sign of x, 0 / 0 = 0, INT_MIN / -1 wraps
    assert one(M.binop("DIV", "INT8", 5, 0)) == 127 and one(M.binop("DIV", "INT8", -5, 0)) == -128 and one(M.binop("DIV", "INT8", 0, 0)) == 0
    assert one(M.binop("DIV", "UINT16", 9, 0)) == 65535 and one(M.binop("DIV", "UINT16", 0, 0)) == 0
    assert one(M.binop("RDIV", "UINT16", 0, 9)) == 65535 and one(M.binop("RDIV", "INT32", 0, -9)) == -2 ** 31
    assert one(M.binop("DIV", "INT64", -2 ** 63, -1)) == -2 ** 63 and one(M.binop("DIV", "INT32", -2 ** 31, -1)) == -2 ** 31
    assert one(M.binop("DIV", "INT32", -7, 2)) == -3 and one(M.binop("DIV", "INT32", 7, -2)) == -3          # C truncates toward zero
    assert one(M.binop("DIV", "UINT64", 2 ** 64 - 1, 2)) == 2 ** 63 - 1
    # MINV is 1 / x by the same rule; on BOOL DIV is FIRST, so MINV is true
    assert [one(M.unop("MINV", "INT8", x)) for x in (0, 1, -1, 2, -128)] == [127, 1, -1, 0, 0]
    assert [one(M.unop("MINV", "UINT8", x)) for x in (0, 1, 2, 255)] == [255, 1, 0, 0]
    assert one(M.unop("MINV", "BOOL", False)) is True and one(M.unop("MINV", "BOOL", True)) is True
    # integer POW: double pow and a saturating cast
    assert one(M.binop("POW", "INT8", 2, 7)) == 127 and one(M.binop("POW", "INT8", -2, 7)) == -128 and one(M.binop("POW", "UINT8", 2, 8)) == 255
    assert one(M.binop("POW", "INT32", 3, 4)) == 81 and one(M.binop("POW", "INT32", 0, 0)) == 1 and one(M.binop("POW", "INT32", 2, -1)) == 0
    assert one(M.binop("POW", "INT32", 0, -1)) == 2 ** 31 - 1 and one(M.binop("POW", "UINT32", 7, 0)) == 1
    assert one(M.binop("POW", "INT64", 2, 63)) == 2 ** 63 - 1 and one(M.binop("POW", "INT64", -2, 63)) == -2 ** 63
    assert one(M.binop("POW", "INT8", 3, 1)) == 3 and one(M.binop("POW", "UINT64", 3, 34)) == 16677181699666568      # 3^34 = ...569 is a tie: to even
    assert one(M.binop("POW", "INT64", -1, -3)) == -1 and one(M.binop("POW", "INT64", -1, -2)) == 1 and one(M.binop("POW", "INT64", 2 ** 63 - 2, 1)) == 2 ** 63 - 1
    assert one(M.binop("POW", "UINT64", 2, 2 ** 64 - 1)) == 2 ** 64 - 1 and one(M.binop("POW", "INT16", -3, 32767)) == -32768
    assert one(M.binop("POW", "UINT32", 2 ** 32 - 1, 33)) == 2 ** 32 - 1 and one(M.binop("POW", "INT32", -(2 ** 31), 33)) == -(2 ** 31) and one(M.binop("POW", "INT32", -(2 ** 31), 32)) == 2 ** 31 - 1
    assert one(M.binop("POW", "BOOL", False, True)) is False and one(M.binop("POW", "BOOL", False, False)) is True
    assert one(M.binop("POW", "FP64", np.float64(1.0), np.float64(NAN))) == 1.0 and math.isnan(one(M.binop("POW", "FP64", np.float64(-1.0), np.float64(0.5))))
    # casts: float -> integer saturates, NaN -> 0; anything -> BOOL is x != 0; integer -> integer wraps; integer -> float rounds once
    assert M.cast("FP64", "INT64", 2.0 ** 63) == 2 ** 63 - 1 and M.cast("FP64", "INT64", -2.0 ** 63 - 2.0 ** 11) == -2 ** 63
    assert M.cast("FP64", "UINT64", 2.0 ** 64) == 2 ** 64 - 1 and M.cast("FP64", "UINT64", 2.0 ** 63) == 2 ** 63
    assert M.cast("FP32", "UINT8", np.float32(-0.5)) == 0 and M.cast("FP32", "UINT8", np.float32(255.5)) == 255 and M.cast("FP32", "INT8", np.float32(-2.5)) == -2
    assert M.cast("FP64", "INT32", NAN) == 0 and M.cast("FP32", "UINT64", np.float32(NAN)) == 0
    assert M.cast("FP64", "INT16", INF) == 32767 and M.cast("FP64", "INT16", -INF) == -32768 and M.cast("FP64", "UINT32", -INF) == 0
    assert M.cast("INT8", "UINT64", -1) == 2 ** 64 - 1 and M.cast("UINT64", "INT8", 2 ** 64 - 1) == -1 and M.cast("INT32", "UINT8", 257) == 1
    assert M.cast("FP64", "BOOL", NAN) is True and M.cast("FP64", "BOOL", -0.0) is False and M.cast("FP32", "BOOL", np.float32(1e-45)) is True
    assert M.cast("BOOL", "FP32", True) == 1.0 and M.cast("BOOL", "INT8", True) == 1
    assert M.cast("UINT64", "FP32", 2 ** 64 - 1) == np.float32(2.0 ** 64) and M.cast("INT64", "FP64", 2 ** 63 - 1) == 2.0 ** 63
    assert M.cast("UINT64", "FP32", 2 ** 24 + 1) == np.float32(2.0 ** 24) and M.cast("UINT64", "FP32", 2 ** 24 + 3) == np.float32(2.0 ** 24 + 4)
    assert M.cast("INT64", "FP32", (1 << 53) + (1 << 29) + 1) == np.float32(2.0 ** 53 + 2.0 ** 30)      # one rounding: through a double it would be 2^53
    assert M.cast("FP64", "FP32", 1e300) == np.float32(INF) and M.cast("FP64", "FP32", 2.0 ** 24 + 1) == np.float32(2.0 ** 24)
    # ABS / AINV of INT_MIN wrap; unsigned AINV is modulo 2^bits
    for t in ("INT8", "INT16", "INT32", "INT64"):
        assert one(M.unop("ABS", t, M.tmin(t))) == M.tmin(t) and one(M.unop("AINV", t, M.tmin(t))) == M.tmin(t)
    assert one(M.unop("AINV", "UINT8", 1)) == 255 and one(M.unop("ABS", "UINT8", 255)) == 255 and one(M.unop("BNOT", "INT8", 0)) == -1
    assert one(M.unop("LNOT", "FP32", np.float32(NAN))) == 0.0 and one(M.unop("LNOT", "INT8", 0)) == 1
    # the BOOL renamings
    for a in (False, True):
        for b in (False, True):
            assert one(M.binop("MINUS", "BOOL", a, b)) == (a ^ b) == one(M.binop("RMINUS", "BOOL", a, b)) == one(M.binop("LXOR", "BOOL", a, b))
            assert one(M.binop("PLUS", "BOOL", a, b)) == (a or b) and one(M.binop("TIMES", "BOOL", a, b)) == (a and b)
            assert one(M.binop("DIV", "BOOL", a, b)) == a and one(M.binop("RDIV", "BOOL", a, b)) == b and one(M.binop("LXNOR", "BOOL", a, b)) == (a == b)
    # comparisons: unsigned above 2^63, NaN
    assert one(M.binop("ISGE", "UINT64", 2 ** 63 + 5, 3)) == 1 and one(M.binop("GT", "UINT64", 2 ** 64 - 1, 2 ** 63)) is True
    assert one(M.binop("EQ", "FP64", np.float64(NAN), np.float64(NAN))) is False and one(M.binop("NE", "FP32", np.float32(NAN), np.float32(NAN))) is True
    assert one(M.binop("ISLE", "FP32", np.float32(NAN), np.float32(1))) == 0.0 and one(M.binop("LXOR", "FP32", np.float32(NAN), np.float32(0))) == 1.0
    # floating-point MIN / MAX omit a NaN; the zeros are not ordered
    assert one(M.binop("MIN", "FP64", np.float64(NAN), np.float64(3))) == 3.0 and one(M.binop("MAX", "FP32", np.float32(-INF), np.float32(NAN))) == -INF
    assert math.isnan(one(M.binop("MIN", "FP64", np.float64(NAN), np.float64(NAN)))) and len(M.binop("MAX", "FP64", np.float64(0.0), np.float64(-0.0))) == 2
    assert M.binop("ANY", "INT8", 1, 2) == (2, 1)
    # bit operators count from 1
    assert one(M.binop("BGET", "UINT8", 0x80, 8)) == 1 and one(M.binop("BGET", "UINT8", 0x80, 9)) == 0 and one(M.binop("BGET", "UINT8", 0xFF, 0)) == 0
    assert one(M.binop("BSET", "INT8", 0, 8)) == -128 and one(M.binop("BCLR", "INT8", -1, 8)) == 127 and one(M.binop("BSET", "INT8", 5, 9)) == 5
    assert one(M.binop("BSET", "INT64", 0, 64)) == -2 ** 63 and one(M.binop("BCLR", "INT64", 7, -1)) == 7 and one(M.binop("BXNOR", "UINT8", 0xF0, 0x0F)) == 0
    # sign, rounding, frexp, ldexp, the special values of the math library
    assert M.same(one(M.unop("SIGNUM", "FP64", np.float64(-0.0))), 0.0) and math.isnan(one(M.unop("SIGNUM", "FP32", np.float32(NAN))))
    assert one(M.unop("ROUND", "FP64", np.float64(2.5))) == 3.0 and one(M.unop("ROUND", "FP64", np.float64(-2.5))) == -3.0
    assert M.same(one(M.unop("ROUND", "FP64", np.float64(-0.4))), -0.0) and M.same(one(M.unop("CEIL", "FP32", np.float32(-0.5))), -0.0)
    assert one(M.unop("FREXPX", "FP64", np.float64(8.0))) == 0.5 and one(M.unop("FREXPE", "FP64", np.float64(8.0))) == 4.0
    assert one(M.unop("FREXPE", "FP64", np.float64(INF))) is M.UNSPECIFIED
    assert one(M.binop("LDEXP", "FP64", np.float64(3.0), np.float64(2.5))) == 12.0 and one(M.binop("LDEXP", "FP64", np.float64(3.0), np.float64(NAN))) == 3.0
    assert one(M.binop("LDEXP", "FP32", np.float32(1.0), np.float32(1e30))) == INF and one(M.binop("LDEXP", "FP32", np.float32(1.0), np.float32(-INF))) == 0.0
    assert M.same(one(M.binop("COPYSIGN", "FP64", np.float64(NAN), np.float64(-1))), NAN) and M.same(one(M.binop("COPYSIGN", "FP64", np.float64(2), np.float64(-0.0))), -2.0)
    assert one(M.unop("TGAMMA", "FP64", np.float64(-0.0))) == -INF and math.isnan(one(M.unop("TGAMMA", "FP64", np.float64(-1.0)))) and one(M.unop("TGAMMA", "FP64", np.float64(3.0))) == 2.0
    assert one(M.unop("LGAMMA", "FP64", np.float64(-1.0))) == INF and one(M.unop("LGAMMA", "FP64", np.float64(1.0))) == 0.0
    assert M.same(one(M.unop("EXPM1", "FP64", np.float64(-0.0))), -0.0) and M.same(one(M.unop("LOG1P", "FP32", np.float32(-0.0))), -0.0)      # C99 F.9.3: +-0 -> +-0
    assert one(M.unop("LOG", "FP64", np.float64(0.0))) == -INF and math.isnan(one(M.unop("LOG", "FP64", np.float64(-1.0)))) and one(M.unop("ERFC", "FP64", np.float64(INF))) == 0.0
    assert one(M.binop("REMAINDER", "FP64", np.float64(2.5), np.float64(1.0))) == 0.5 and one(M.binop("FMOD", "FP64", np.float64(-2.5), np.float64(1.0))) == -0.5
    assert math.isnan(one(M.binop("REMAINDER", "FP64", np.float64(1.0), np.float64(0.0)))) and one(M.binop("HYPOT", "FP64", np.float64(INF), np.float64(NAN))) == INF


def test_the_edge_values_hold_what_the_issue_lists():
    for t in M.INT_TYPES:
        E = M.edge_values(t); b = M.bits(t)
        need = [0, 1, 2, 3, 7, M.tmin(t), M.tmin(t) + 1, M.tmax(t), M.tmax(t) - 1, M.tmax(t) // 2] + [w for w in (8, 16, 32, 64) if w <= M.tmax(t)] + ([b + 1] if b + 1 <= M.tmax(t) else [])
        assert all(v in E for v in need) and (not M.is_signed(t) or -1 in E) and all(M.tmin(t) <= v <= M.tmax(t) for v in E) and len(set(E)) == len(E)
    for t in M.FP_TYPES:
        E = M.edge_values(t); fi = np.finfo(M.NP[t])
        for v in (0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.5, -2.5, 3.0, INF, -INF, NAN, fi.max, fi.tiny, fi.smallest_subnormal, 2.0 ** 24 + 1, 2.0 ** 53 + 1, 2.0 ** 31, 2.0 ** 63,
                  2.0 ** 64, -2.0 ** 63 - 2.0 ** 11, 255.5, 1e30):
            assert any(M.same(M.NP[t](v), e) for e in E), (t, v)
        assert all(type(e) is M.NP[t] for e in E)
    assert M.edge_values("BOOL") == [False, True]


@pytest.mark.parametrize("t", M.TYPES)
def test_the_monoid_laws(t):
    for op in M.monoids_of(t):
        ident, term = M.monoid_identity(op, t), M.monoid_terminal(op, t)
        for x in M.edge_values(t):
            if op == "ANY":
                continue                                                # (ANY keeps either argument: its identity is never combined with a value)
            if M.is_fp(t) and op in ("MIN", "MAX") and x != x:
                continue                                                # (a NaN argument is omitted: MIN(inf, NaN) = inf, the rule of DESIGN.md section 8)
            for r in (M.binop(op, t, ident, x), M.binop(op, t, x, ident)):
                if M.is_fp(t) and op == "PLUS" and M.same(x, -0.0):
                    assert len(r) == 1 and M.same(r[0], 0.0)            # (0 + -0 = +0: equal as numbers, the one value IEEE addition has no bit-exact identity for)
                else:
                    assert len(r) == 1 and M.same(r[0], x), (op, t, x, r)
            if term is not None:
                for r in (M.binop(op, t, term, x), M.binop(op, t, x, term)):
                    assert len(r) == 1 and M.same(r[0], term), (op, t, x, r)
        # the identity has the type's own width
        if M.is_int(t):
            assert M.tmin(t) <= ident <= M.tmax(t)
    if M.is_int(t) and not M.is_signed(t):
        assert M.monoid_identity("BAND", t) == M.monoid_identity("BXNOR", t) == 2 ** M.bits(t) - 1 and M.monoid_terminal("BOR", t) == 2 ** M.bits(t) - 1
    if t == "INT8":
        assert (M.monoid_identity("MIN", t), M.monoid_identity("MAX", t), M.monoid_terminal("MIN", t), M.monoid_terminal("TIMES", t)) == (127, -128, -128, 0)
    if t == "FP32":
        assert M.monoid_identity("MIN", t) == INF and M.monoid_terminal("MAX", t) == INF and M.monoid_terminal("TIMES", t) is None and M.monoid_terminal("PLUS", t) is None
