"""An independent model of the built-in operator tables and typecasts (test infrastructure), written from the rules and not from the HIP sources:
SURVEY.md App. A items 5 and 7, the `[upstream semantics]` notes of grb_ops.hpp and C99 Annex F.  tests/test_operator_model.py pins it to the C oracle, to
tests/companion_model.py and to hand-written facts; tests/test_operator_table_gpu.py compares every exported operator handle of the library with it.

Values: BOOL is a Python bool, the integer types are Python ints wrapped explicitly to the type's width, FP32 / FP64 are numpy.float32 / numpy.float64
scalars.  `binop` / `unop` / `fold` return the TUPLE of accepted results: usually one value; both arguments for ANY; both zeros for MIN / MAX of +0.0
and -0.0; a NaN stands for any NaN; `UNSPECIFIED` where C leaves the value open (the exponent frexp reports for inf / NaN).

The rules that are not plain C:
  * integer x / 0 saturates by the sign of x, 0 / 0 = 0, INT_MIN / -1 wraps; MINV(x) = 1 / x by the same rule;
  * integer POW is double pow(), correctly rounded, and a saturating cast back;
  * float -> integer saturates and NaN -> 0; anything -> BOOL is x != 0; every other cast is the C conversion (one rounding);
  * the BOOL column renames arithmetic to logic: PLUS = MAX = LOR, TIMES = MIN = LAND, MINUS = RMINUS = NE = ISNE = LXOR, EQ = ISEQ = LXNOR,
    DIV = FIRST, RDIV = SECOND, POW = GE, and MINV(x) = DIV(true, x) = true;
  * floating-point MIN / MAX omit a NaN argument (fmin / fmax);
  * BGET / BSET / BCLR count bits from 1; a position outside 1 .. bits gives 0 (BGET) or leaves x alone;
  * LDEXP(x, y) scales by 2^k with k = y cast to INT32 by the float -> integer rule above (C leaves an out-of-range conversion undefined; the
    library's own cast is the one definition every route can share).
"""
import math

import numpy as np

TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
NP = {"BOOL": np.bool_, "INT8": np.int8, "UINT8": np.uint8, "INT16": np.int16, "UINT16": np.uint16, "INT32": np.int32, "UINT32": np.uint32,
      "INT64": np.int64, "UINT64": np.uint64, "FP32": np.float32, "FP64": np.float64}
INT_TYPES = [t for t in TYPES if "INT" in t]
FP_TYPES = ["FP32", "FP64"]
UNSPECIFIED = "unspecified"

ARITH = ["FIRST", "SECOND", "PAIR", "ANY", "MIN", "MAX", "PLUS", "MINUS", "RMINUS", "TIMES", "DIV", "RDIV", "POW"]
IS_CMP = ["ISEQ", "ISNE", "ISGT", "ISLT", "ISGE", "ISLE"]
CMP = ["EQ", "NE", "GT", "LT", "GE", "LE"]
LOGIC = ["LOR", "LAND", "LXOR"]
BITWISE = ["BOR", "BAND", "BXOR", "BXNOR", "BGET", "BSET", "BCLR"]
FP_ONLY = ["ATAN2", "HYPOT", "FMOD", "REMAINDER", "COPYSIGN", "LDEXP"]
# operators whose result comes out of the math library (a bound applies); every other operator is exact
MATH_BINOPS = {"POW", "ATAN2", "HYPOT", "FMOD", "REMAINDER"}
MATH_UNOPS = {"LOG", "EXP", "LOG2", "SIN", "COS", "TAN", "ACOS", "ASIN", "ATAN", "SINH", "COSH", "TANH", "ACOSH", "ASINH", "ATANH", "EXP2", "EXPM1",
              "LOG10", "LOG1P", "LGAMMA", "TGAMMA", "ERF", "ERFC"}
EXACT_FP_UNOPS = ["SQRT", "SIGNUM", "CEIL", "FLOOR", "ROUND", "TRUNC", "FREXPX", "FREXPE", "ISINF", "ISNAN", "ISFINITE"]
COMMON_UNOPS = ["IDENTITY", "AINV", "MINV", "LNOT", "ONE", "ABS"]


def is_int(t): return "INT" in t
def is_fp(t): return t.startswith("FP")
def is_signed(t): return t.startswith("INT")
def bits(t): return int(t.lstrip("UINT"))
def tmin(t): return -(1 << (bits(t) - 1)) if is_signed(t) else 0
def tmax(t): return (1 << (bits(t) - 1)) - 1 if is_signed(t) else (1 << bits(t)) - 1


def binops_of(t):
    """The binary operators the library exports for type `t`."""
    ops = ARITH + IS_CMP + CMP + LOGIC
    if t == "BOOL": return ops + ["LXNOR"]
    return ops + (BITWISE if is_int(t) else FP_ONLY)


def unops_of(t):
    if t == "BOOL": return list(COMMON_UNOPS)
    return COMMON_UNOPS + (["BNOT"] if is_int(t) else EXACT_FP_UNOPS + sorted(MATH_UNOPS))


def monoids_of(t):
    if t == "BOOL": return ["LOR", "LAND", "LXOR", "LXNOR", "EQ", "ANY"]
    return ["MIN", "MAX", "PLUS", "TIMES", "ANY"] + (["BOR", "BAND", "BXOR", "BXNOR"] if is_int(t) and not is_signed(t) else [])


def wrap(t, x):
    """The integer x modulo 2^bits, read as a value of the integer type t."""
    b = bits(t); x = int(x) & ((1 << b) - 1)
    return x - (1 << b) if is_signed(t) and x >> (b - 1) else x


def edge_values(t):
    """The fixed edge values of a type (ISSUE: 0, +-1, 2, 3, 7, the extremes and their neighbours, the bit widths and one above, two mid-range values;
    the IEEE specials, the format's limits, the integer-range boundaries a cast meets)."""
    if t == "BOOL":
        return [False, True]
    if is_int(t):
        lo, hi = tmin(t), tmax(t)
        c = [0, 1, -1, 2, 3, 7, lo, lo + 1, hi, hi - 1, hi // 2, 8, 9, 16, 17, 32, 33, 64, 65, hi // 3, (hi // 5) * 3 + 1, -(hi // 7) * 3]
        out = []
        for v in c:
            if lo <= v <= hi and v not in out: out.append(v)
        return out
    f = NP[t]; fi = np.finfo(f)
    c = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.5, -2.5, 3.0, math.inf, -math.inf, math.nan, float(fi.max), float(fi.tiny), float(fi.smallest_subnormal),
         2.0 ** 24 + 1, 2.0 ** 53 + 1, 2.0 ** 31, 2.0 ** 63, 2.0 ** 64, -2.0 ** 63 - 2.0 ** 11, 255.5, 1e30]
    out = []
    for v in c:
        v = f(v)                                                   # (each rounded to the type: 2^24 + 1 is 2^24 in FP32, 2^53 + 1 is 2^53 in both)
        if not any(same(v, w) for w in out): out.append(v)
    return out


def same(a, b):
    """Bit-level equality of two model values: NaN equals NaN, +0.0 differs from -0.0."""
    if isinstance(a, (float, np.floating)) or isinstance(b, (float, np.floating)):
        a, b = float(a), float(b)
        if a != a or b != b: return a != a and b != b
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
    return a == b


def accepted(got, results):
    return any(r is UNSPECIFIED or same(got, r) for r in results)


# ---- casts -----------------------------------------------------------------------------------------------------------------------------------------
def _int_to_fp(t, n):
    """The integer n rounded ONCE to the nearest value of the float type (ties to even), as the C conversion does."""
    p = 24 if t == "FP32" else 53
    m = abs(n); bl = m.bit_length()
    if bl > p:
        sh = bl - p; q, rem = m >> sh, m & ((1 << sh) - 1); half = 1 << (sh - 1)
        if rem > half or (rem == half and q & 1): q += 1
        m = q << sh
    return NP[t](float(m) if n >= 0 else -float(m))


def cast(ft, tt, x):
    if tt == "BOOL":
        return bool(x != 0)                                          # (a NaN differs from 0: true)
    if ft == "BOOL":
        x = 1 if x else 0; ft = "UINT8"
    if is_fp(tt):
        with np.errstate(over="ignore"):
            return NP[tt](x) if is_fp(ft) else _int_to_fp(tt, int(x))
    if is_fp(ft):
        x = float(x)
        if x != x: return 0
        if math.isinf(x): return tmax(tt) if x > 0 else tmin(tt)
        return min(max(int(x), tmin(tt)), tmax(tt))                  # int() truncates toward zero, exactly
    return wrap(tt, x)


# ---- binary operators ------------------------------------------------------------------------------------------------------------------------------
def _idiv(t, x, y):
    if y == 0:
        return 0 if x == 0 else (tmax(t) if x > 0 else tmin(t))
    q = abs(x) // abs(y)
    return wrap(t, -q if (x < 0) != (y < 0) else q)


def _ipow(t, x, y):
    """Integer POW: the correctly rounded double of x^y, cast back with saturation.  (The power is formed exactly: math libraries differ in the
    last place beyond 2^53 — pow(3, 34) is a tie that one libm rounds up and another to even — and on integers the cast would turn a result
    just below a whole number into the number below.)"""
    if y == 0: return 1
    if y < 0:
        return tmax(t) if x == 0 else (0 if abs(x) > 1 else (x if y % 2 else 1))        # +inf; a fraction truncates to 0; (+-1)^y
    if abs(x) > 1 and (y >= 64 or (abs(x) ** y).bit_length() > 64):   # beyond every integer type (and, further out, beyond double): saturates by sign
        return tmin(t) if x < 0 and y % 2 else tmax(t)
    return cast("FP64", t, _int_to_fp("FP64", x ** y))


def _fp_math2(op, x, y):
    """The double-precision result of a math-library operator on doubles."""
    with np.errstate(all="ignore"):
        if op == "POW": return np.power(x, y)
        if op == "ATAN2": return np.arctan2(x, y)
        if op == "HYPOT": return np.hypot(x, y)
        if op == "FMOD": return np.fmod(x, y)
        if op == "REMAINDER":
            try: return np.float64(math.remainder(x, y))
            except ValueError: return np.float64(math.nan)
    raise ValueError(op)


def binop(op, t, a, b):
    """The accepted results of z = op(a, b) with a, b of type t; z has type t, or BOOL for EQ .. LE."""
    if op == "ANY":
        return (b, a)
    if t == "BOOL":
        r = {"FIRST": a, "DIV": a, "SECOND": b, "RDIV": b, "PAIR": True,
             "MIN": a and b, "TIMES": a and b, "LAND": a and b, "MAX": a or b, "PLUS": a or b, "LOR": a or b,
             "MINUS": a != b, "RMINUS": a != b, "ISNE": a != b, "NE": a != b, "LXOR": a != b, "ISEQ": a == b, "EQ": a == b, "LXNOR": a == b,
             "ISGT": a > b, "GT": a > b, "ISLT": a < b, "LT": a < b, "ISGE": a >= b, "GE": a >= b, "POW": a >= b, "ISLE": a <= b, "LE": a <= b}[op]
        return (bool(r),)
    fp = is_fp(t); T = NP[t] if fp else (lambda v: wrap(t, v))
    if op == "FIRST": return (a,)
    if op == "SECOND": return (b,)
    if op == "PAIR": return (T(1),)
    if op in ("MIN", "MAX"):
        if fp:
            if a != a: return (b,)
            if b != b: return (a,)
            if a == b: return (a,) if same(a, b) else (a, b)
        return (min(a, b),) if op == "MIN" else (max(a, b),)
    if op in IS_CMP or op in CMP:
        r = {"EQ": a == b, "NE": a != b, "GT": a > b, "LT": a < b, "GE": a >= b, "LE": a <= b}[op[-2:]]
        return (bool(r),) if op in CMP else (T(1 if r else 0),)
    if op in LOGIC:
        p, q = bool(a != 0), bool(b != 0)
        return (T(1 if {"LOR": p or q, "LAND": p and q, "LXOR": p != q}[op] else 0),)
    if fp:
        with np.errstate(all="ignore"):
            if op == "PLUS": return (a + b,)
            if op == "MINUS": return (a - b,)
            if op == "RMINUS": return (b - a,)
            if op == "TIMES": return (a * b,)
            if op == "DIV": return (a / b,)
            if op == "RDIV": return (b / a,)
            if op == "COPYSIGN": return (np.copysign(a, b),)
            if op == "LDEXP": return (T(np.ldexp(np.float64(a), np.int32(cast(t, "INT32", b)))),)
            return (T(_fp_math2(op, np.float64(a), np.float64(b))),)
    if op == "PLUS": return (wrap(t, a + b),)
    if op == "MINUS": return (wrap(t, a - b),)
    if op == "RMINUS": return (wrap(t, b - a),)
    if op == "TIMES": return (wrap(t, a * b),)
    if op == "DIV": return (_idiv(t, a, b),)
    if op == "RDIV": return (_idiv(t, b, a),)
    if op == "POW": return (_ipow(t, a, b),)
    m = (1 << bits(t)) - 1; ua, ub = a & m, b & m
    if op == "BOR": return (wrap(t, ua | ub),)
    if op == "BAND": return (wrap(t, ua & ub),)
    if op == "BXOR": return (wrap(t, ua ^ ub),)
    if op == "BXNOR": return (wrap(t, ~(ua ^ ub)),)
    inside = 1 <= b <= bits(t)
    if op == "BGET": return ((ua >> (b - 1)) & 1 if inside else 0,)
    if op == "BSET": return (wrap(t, ua | (1 << (b - 1))) if inside else a,)
    if op == "BCLR": return (wrap(t, ua & ~(1 << (b - 1))) if inside else a,)
    raise ValueError((op, t))


def binop_math64(op, t, a, b):
    """For a floating-point math-library operator: the double-precision result the bound is taken against."""
    return _fp_math2(op, np.float64(a), np.float64(b))


def binop_ztype(op, t):
    return "BOOL" if op in CMP else t


# ---- unary operators -------------------------------------------------------------------------------------------------------------------------------
def _c_round(x):
    if x != x or math.isinf(x) or abs(x) >= 2.0 ** 52: return x
    r = math.floor(abs(x))
    if abs(x) - r >= 0.5: r += 1
    return math.copysign(float(r), x)


def _lib1(f, x, pole=math.nan):
    try: return f(x)
    except ValueError: return pole
    except OverflowError: return math.inf


def _tgamma(x):
    if x != x: return math.nan
    if x == 0: return math.copysign(math.inf, x)                     # C99 F.9.5.4: tgamma(+-0) = +-inf
    if x == -math.inf or (x < 0 and x == math.floor(x)): return math.nan
    return _lib1(math.gamma, x)


def _lgamma(x):
    if x != x: return math.nan
    if math.isinf(x) or (x <= 0 and x == math.floor(x)): return math.inf
    return _lib1(math.lgamma, x)


def fp_math1(op, x):
    """The double-precision result of a math-library unary operator on a double (C99 Annex F at the special values)."""
    x = np.float64(x)
    with np.errstate(all="ignore"):
        f = {"LOG": np.log, "EXP": np.exp, "LOG2": np.log2, "SIN": np.sin, "COS": np.cos, "TAN": np.tan, "ACOS": np.arccos, "ASIN": np.arcsin,
             "ATAN": np.arctan, "SINH": np.sinh, "COSH": np.cosh, "TANH": np.tanh, "ACOSH": np.arccosh, "ASINH": np.arcsinh, "ATANH": np.arctanh,
             "EXP2": np.exp2, "EXPM1": np.expm1, "LOG10": np.log10, "LOG1P": np.log1p}.get(op)
        if f is not None: return np.float64(f(x))
    x = float(x)
    if op == "LGAMMA": return np.float64(_lgamma(x))
    if op == "TGAMMA": return np.float64(_tgamma(x))
    if op == "ERF": return np.float64(math.erf(x))
    if op == "ERFC": return np.float64(math.erfc(x))
    raise ValueError(op)


def unop(op, t, x):
    """The accepted results of z = op(x), x and z of type t."""
    if t == "BOOL":
        return ({"IDENTITY": x, "AINV": x, "ABS": x, "MINV": True, "LNOT": not x, "ONE": True}[op],)
    fp = is_fp(t); T = NP[t] if fp else (lambda v: wrap(t, v))
    if op == "IDENTITY": return (x,)
    if op == "ONE": return (T(1),)
    if op == "LNOT": return (T(0 if x != 0 else 1),)
    if op == "AINV": return (-x,) if fp else (wrap(t, -x),)
    if op == "ABS": return (abs(x),) if fp else (wrap(t, abs(x)),)
    if op == "MINV":
        with np.errstate(all="ignore"):
            return (T(1) / x,) if fp else (_idiv(t, 1, x),)
    if op == "BNOT": return (wrap(t, ~x),)
    d = float(x)
    if op == "SQRT":
        with np.errstate(all="ignore"): return (T(np.sqrt(np.float64(d))),)      # (correctly rounded; through double it still rounds once for FP32)
    if op == "SIGNUM": return (x,) if d != d else (T((d > 0) - (d < 0)),)
    if op == "CEIL": return (T(np.ceil(np.float64(d))),)
    if op == "FLOOR": return (T(np.floor(np.float64(d))),)
    if op == "TRUNC": return (T(np.trunc(np.float64(d))),)
    if op == "ROUND": return (T(_c_round(d)),)
    if op == "FREXPX": return (x,) if (d != d or math.isinf(d)) else (T(math.frexp(d)[0]),)
    if op == "FREXPE": return (UNSPECIFIED,) if (d != d or math.isinf(d)) else (T(math.frexp(d)[1]),)
    if op == "ISINF": return (T(1 if math.isinf(d) else 0),)
    if op == "ISNAN": return (T(1 if d != d else 0),)
    if op == "ISFINITE": return (T(1 if math.isfinite(d) else 0),)
    with np.errstate(over="ignore"):
        return (T(fp_math1(op, d)),)


# ---- monoids ---------------------------------------------------------------------------------------------------------------------------------------
def monoid_identity(op, t):
    if t == "BOOL":
        return {"LOR": False, "LXOR": False, "ANY": False, "LAND": True, "LXNOR": True, "EQ": True}[op]
    T = NP[t] if is_fp(t) else int
    if op == "MIN": return T(math.inf) if is_fp(t) else tmax(t)
    if op == "MAX": return T(-math.inf) if is_fp(t) else tmin(t)
    if op == "TIMES": return T(1)
    if op in ("BAND", "BXNOR"): return tmax(t)                      # all bits set (the unsigned types only)
    if op in ("PLUS", "ANY", "BOR", "BXOR"): return T(0)
    raise ValueError((op, t))


def monoid_terminal(op, t):
    """The value that ends a reduction early, or None.  (ANY stops at its first value whatever it is: it has no terminal VALUE.)"""
    if t == "BOOL":
        return {"LOR": True, "LAND": False}.get(op)
    T = NP[t] if is_fp(t) else int
    if op == "MIN": return T(-math.inf) if is_fp(t) else tmin(t)
    if op == "MAX": return T(math.inf) if is_fp(t) else tmax(t)
    if op == "TIMES" and is_int(t): return 0
    if op == "BOR": return tmax(t)
    if op == "BAND": return 0
    return None


def fold(op, t, values):
    """The accepted results of reducing `values` (at least one) with the monoid from left to right."""
    if op == "ANY":
        out = []
        for v in values:
            if not any(same(v, w) for w in out): out.append(v)
        return tuple(out)
    accs = [values[0]]
    for v in values[1:]:
        nxt = []
        for a in accs:
            for r in binop(op, t, a, v):
                if not any(same(r, w) for w in nxt): nxt.append(r)
        accs = nxt
    return tuple(accs)
