"""User-defined unary, binary and select operators: `@unary_op(T)` / `@binary_op(T)` / `@select_op(T, thunk_type=None)`.

Same names and call shape as the reference's decorators (pygraphblas/binaryop.py:137, unaryop.py:101).  The reference compiles the
Python function with numba into a host function pointer; a HIP kernel cannot call one.  Here the function's AST is translated into
the C definition SuiteSparse 7's `GxB_UnaryOp_new` / `GxB_BinaryOp_new` take as text, and the library compiles that text for the
device at first use (grb_userop.cpp).  The result is used like a built-in operator: `A.apply(op)`, `A.apply_first(s, op)`,
`A.apply_second(op, s)`, `A.eadd(B, op)`, `A.emult(B, op)` on `Matrix` and `Vector`, and (binary) as a `with op:` context.

    @binary_op(FP32)
    def PLUS(x, y):
        return x + log1p(exp(y - x))

`@select_op(T, thunk_type=None)` (reference: pygraphblas/selectop.py:103) makes a predicate over an entry's row, column, value and the thunk, for
`A.select(op, thunk)` on `Matrix` and `Vector` (`GxB_SelectOp_new`): i and j are integers, x has the kind of T, v that of `thunk_type` (T when not given),
and the returned value's truth decides whether the entry stays.

    @select_op(FP64)
    def band_above(i, j, x, v):
        return abs(i - j) <= 2 and x > v

The supported subset of Python (anything else raises `TypeError` at decoration time, naming the construct and its line):

* parameters; int / float / bool constants, also captured from the enclosing scopes;
* local assignment and augmented assignment, `return`, `if` / `elif` / `else`, conditional expressions, `pass`; `assert` is dropped;
* `+ - *`, unary `- + ~ not`, `& | ^ << >>` (integers only), comparisons (chained ones too), `and` / `or`;
* `/` is evaluated in double; `//` and `%` have Python's floor semantics (for floats CPython's own algorithm); `**` maps to `pow`
  (two integers: the exact integer power; a negative exponent gives `pow`'s double truncated to an integer, where Python gives a float);
* `abs`, `min`, `max`, and from `math` (as `math.f` or bare `f`): log log1p log2 log10 exp expm1 sqrt sin cos tan asin acos atan
  atan2 sinh cosh tanh fabs floor ceil trunc pow copysign fmod isnan isinf;
* nested helper functions made of the same subset: they become static C functions ahead of the operator.

Evaluation model: an integer-typed expression is an `int64_t`, a float-typed one a `double` — also inside an FP32 operator, as
Python itself computes — and the returned value is converted to the operator's type with a C cast.  What Python raises an exception
for (division by zero, `math.log(0)`, integers beyond 64 bits) follows C instead: IEEE infinities / NaN, 0 for an integer division
or remainder by zero, two's-complement wrap-around.
"""
import ast
import ctypes as C
import inspect
import math
import textwrap

from . import types
from ._capi import lib
from .base import check, _error_codes, GraphBLASException, DomainMismatch

__all__ = ["unary_op", "binary_op", "select_op", "UserUnaryOp", "UserBinaryOp", "UserSelectOp", "translate", "translate_select"]

_CTYPE = {"BOOL": "bool", "INT8": "int8_t", "UINT8": "uint8_t", "INT16": "int16_t", "UINT16": "uint16_t", "INT32": "int32_t",
          "UINT32": "uint32_t", "INT64": "int64_t", "UINT64": "uint64_t", "FP32": "float", "FP64": "double"}
_C = {"i": "int64_t", "d": "double"}

_MATH1 = ("log1p", "log2", "log10", "exp", "expm1", "sqrt", "sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "fabs")
_MATH2 = ("atan2", "pow", "copysign", "fmod")
_MATHI = ("floor", "ceil", "trunc")
_MATHB = ("isnan", "isinf")
_MATH = _MATH1 + _MATH2 + _MATHI + _MATHB + ("log",)

# C helpers of the generated text (plain C, valid as C++ too); only the ones a definition uses are emitted, in this order
_HELPERS = (
    ("grb_floordiv_i", "static int64_t grb_floordiv_i(int64_t a, int64_t b) { int64_t q; if (b == 0) return 0; q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) q--; return q; }"),
    ("grb_mod_i", "static int64_t grb_mod_i(int64_t a, int64_t b) { int64_t r; if (b == 0) return 0; r = a % b; if (r != 0 && ((r < 0) != (b < 0))) r += b; return r; }"),
    ("grb_floordiv_d", "static double grb_floordiv_d(double a, double b) { double mod = fmod(a, b), div = (a - mod) / b, f; if (mod != 0) { if ((b < 0) != (mod < 0)) div -= 1.0; } "
                       "if (div != 0) { f = floor(div); if (div - f > 0.5) f += 1.0; } else f = copysign(0.0, a / b); return f; }"),
    ("grb_mod_d", "static double grb_mod_d(double a, double b) { double mod = fmod(a, b); if (mod != 0) { if ((b < 0) != (mod < 0)) mod += b; } else mod = copysign(0.0, b); return mod; }"),
    ("grb_pow_i", "static int64_t grb_pow_i(int64_t a, int64_t b) { int64_t r = 1; if (b < 0) return (int64_t)pow((double)a, (double)b); while (b) { if (b & 1) r *= a; b >>= 1; if (b) a *= a; } return r; }"),
    ("grb_abs_i", "static int64_t grb_abs_i(int64_t a) { return a < 0 ? -a : a; }"),
    ("grb_min_i", "static int64_t grb_min_i(int64_t a, int64_t b) { return b < a ? b : a; }"),
    ("grb_max_i", "static int64_t grb_max_i(int64_t a, int64_t b) { return b > a ? b : a; }"),
    ("grb_min_d", "static double grb_min_d(double a, double b) { return b < a ? b : a; }"),
    ("grb_max_d", "static double grb_max_d(double a, double b) { return b > a ? b : a; }"),
    ("grb_isinf", "static int64_t grb_isinf(double a) { return (a == a) && (a - a != 0); }"),
)

_CONSTRUCT = {"For": "'for' loop", "AsyncFor": "'for' loop", "While": "'while' loop", "With": "'with' block", "Try": "'try' block", "Raise": "'raise'",
              "Lambda": "lambda", "ListComp": "comprehension", "GeneratorExp": "comprehension", "Attribute": "attribute access", "Subscript": "subscript",
              "Tuple": "tuple", "List": "list", "Dict": "dict", "Global": "'global'", "Nonlocal": "'nonlocal'", "Import": "'import'", "ImportFrom": "'import'",
              "Delete": "'del'", "ClassDef": "class definition", "JoinedStr": "f-string", "Yield": "'yield'", "Await": "'await'", "Starred": "starred expression",
              "NamedExpr": "assignment expression", "MatMult": "'@' operator"}


def _join(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return "d" if "d" in (a, b) else "i"


def _cast(text, have, want):
    return text if have == want else f"(({_C[want]})({text}))"


class _Translator:
    """One decorated function -> C text."""

    def __init__(self, func, base, line0, consts):
        self.func, self.base, self.line0, self.consts = func, base, line0, consts
        self.used = set()          # C helpers of _HELPERS
        self.specs = {}            # (helper name, argument types) -> (C name, return type, text)
        self.order = []            # C texts of specialised helper functions, in dependency order
        self.active = []           # helpers being specialised (recursion check)
        self.select = None         # a select operator: the C types (X, K) of its value and thunk

    def err(self, node, what):
        line = self.line0 + getattr(node, "lineno", 1) - 1
        raise TypeError(f"{self.func.__name__}: {what} is not supported in a user-defined operator (line {line})")

    def unsupported(self, node):
        name = type(node).__name__
        self.err(node, _CONSTRUCT.get(name, name))

    # ---- one function (the operator itself or a specialised helper) -----------------------------------------------------------
    def function(self, fdef, argtypes, helpers):
        """Returns (locals' types, return type, body lines) of `fdef` called with `argtypes`."""
        a = fdef.args
        if a.vararg or a.kwarg or a.kwonlyargs or a.defaults or getattr(a, "posonlyargs", None):
            self.err(fdef, "a parameter list with defaults, * or **")
        params = [p.arg for p in a.args]
        if len(params) != len(argtypes):
            self.err(fdef, f"calling {fdef.name} with {len(argtypes)} arguments")
        helpers = dict(helpers)
        assigned = set()
        for st in fdef.body:
            self._scan(st, assigned, helpers)
        env = dict(zip(params, argtypes))
        state = {"ret": None}
        for _ in range(2 * (len(assigned) + len(params)) + 4):          # types only ever widen (i -> d): a fixed point within that many passes
            before = (dict(env), state["ret"])
            ctx = {"env": env, "assigned": assigned | set(params), "helpers": helpers, "state": state, "is_op": fdef is self.top}
            lines = self.block(fdef.body, ctx, 1)
            if (env, state["ret"]) == before:
                break
        if not self._always_returns(fdef.body):
            self.err(fdef, f"a function that may end without returning a value ({fdef.name})")
        return env, state["ret"] or "i", lines, params

    def _scan(self, st, assigned, helpers):
        """Names assigned in this function's own body, and its nested helper definitions."""
        if isinstance(st, ast.FunctionDef):
            helpers[st.name] = (st, dict(helpers))
            return
        if isinstance(st, ast.Assign):
            for t in st.targets:
                if isinstance(t, ast.Name):
                    assigned.add(t.id)
        elif isinstance(st, (ast.AugAssign, ast.AnnAssign)) and isinstance(st.target, ast.Name):
            assigned.add(st.target.id)
        elif isinstance(st, ast.If):
            for s in st.body + st.orelse:
                self._scan(s, assigned, helpers)

    def _always_returns(self, body):
        if not body:
            return False
        last = body[-1]
        if isinstance(last, ast.Return):
            return True
        if isinstance(last, ast.If):
            return self._always_returns(last.body) and self._always_returns(last.orelse)
        return False

    # ---- statements -------------------------------------------------------------------------------------------------------------
    def block(self, body, ctx, depth):
        out = []
        pad = "  " * depth
        for st in body:
            if isinstance(st, ast.FunctionDef):
                continue                                                  # a helper: emitted where it is called, per argument types
            if isinstance(st, (ast.Assert, ast.Pass)):
                continue                                                  # assert is dropped
            if isinstance(st, ast.Expr) and isinstance(st.value, ast.Constant) and isinstance(st.value.value, str):
                continue                                                  # docstring
            if isinstance(st, ast.Return):
                if st.value is None:
                    self.err(st, "'return' without a value")
                text, t = self.expr(st.value, ctx)
                ctx["state"]["ret"] = _join(ctx["state"]["ret"], t)
                if ctx["is_op"] and self.select:
                    out.append(f"{pad}return ({text}) != 0;")
                elif ctx["is_op"]:
                    out.append(f"{pad}{{ *z = ({self.ctype})({text}); return; }}")
                else:
                    out.append(f"{pad}return {_cast(text, t, ctx['state']['ret'])};")
            elif isinstance(st, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
                if isinstance(st, ast.Assign):
                    if len(st.targets) != 1 or not isinstance(st.targets[0], ast.Name):
                        self.err(st, "assignment to anything but one local name")
                    name, value = st.targets[0].id, st.value
                elif isinstance(st, ast.AnnAssign):
                    if not isinstance(st.target, ast.Name) or st.value is None:
                        self.err(st, "assignment to anything but one local name")
                    name, value = st.target.id, st.value
                else:
                    if not isinstance(st.target, ast.Name):
                        self.err(st, "assignment to anything but one local name")
                    name = st.target.id
                    value = ast.copy_location(ast.BinOp(left=ast.copy_location(ast.Name(id=name, ctx=ast.Load()), st), op=st.op, right=st.value), st)
                text, t = self.expr(value, ctx)
                env = ctx["env"]
                env[name] = _join(env.get(name), t)
                out.append(f"{pad}v_{name} = {_cast(text, t, env[name])};")
            elif isinstance(st, ast.If):
                text, _t = self.expr(st.test, ctx)
                out.append(f"{pad}if ({text}) {{")
                out += self.block(st.body, ctx, depth + 1)
                if st.orelse:
                    out.append(f"{pad}}} else {{")
                    out += self.block(st.orelse, ctx, depth + 1)
                out.append(f"{pad}}}")
            else:
                self.unsupported(st)
        return out

    # ---- expressions: (C text, 'i' | 'd') -----------------------------------------------------------------------------------------
    def constant(self, node, v):
        if isinstance(v, bool):
            return ("1" if v else "0"), "i"
        if isinstance(v, int):
            if not -(1 << 63) <= v < (1 << 63):
                self.err(node, f"the integer constant {v} (beyond 64 bits)")
            return (f"{v}LL" if v > -(1 << 63) else "(-9223372036854775807LL - 1)"), "i"
        if isinstance(v, float):
            if math.isnan(v):
                return "NAN", "d"
            if math.isinf(v):
                return ("INFINITY" if v > 0 else "(-INFINITY)"), "d"
            r = repr(v)
            return (r if any(c in r for c in ".en") else r + ".0"), "d"
        self.err(node, f"a constant of type {type(v).__name__}")

    def expr(self, node, ctx):
        if isinstance(node, ast.Constant):
            return self.constant(node, node.value)
        if isinstance(node, ast.Name):
            if node.id in ctx["assigned"]:
                return f"v_{node.id}", ctx["env"].get(node.id, "i")
            if node.id in self.consts:
                text, t = self.constant(node, self.consts[node.id])
                return f"({text})", t
            self.err(node, f"the name '{node.id}' (not a parameter, a local, or an int / float / bool constant of an enclosing scope)")
        if isinstance(node, ast.BinOp):
            return self.binop(node, ctx)
        if isinstance(node, ast.UnaryOp):
            text, t = self.expr(node.operand, ctx)
            if isinstance(node.op, ast.USub):
                return f"(-{text})", t
            if isinstance(node.op, ast.UAdd):
                return text, t
            if isinstance(node.op, ast.Not):
                return f"((int64_t)!({text}))", "i"
            if t != "i":
                self.err(node, "'~' on a floating-point value")
            return f"(~{text})", "i"
        if isinstance(node, ast.Compare):
            ops = {ast.Eq: "==", ast.NotEq: "!=", ast.Lt: "<", ast.LtE: "<=", ast.Gt: ">", ast.GtE: ">="}
            left, parts = self.expr(node.left, ctx)[0], []
            for op, right in zip(node.ops, node.comparators):
                if type(op) not in ops:
                    self.err(node, f"the comparison '{type(op).__name__}'")
                r = self.expr(right, ctx)[0]
                parts.append(f"({left} {ops[type(op)]} {r})")
                left = r
            return "((int64_t)(" + " && ".join(parts) + "))", "i"
        if isinstance(node, ast.BoolOp):
            vals = [self.expr(v, ctx) for v in node.values]
            t = None
            for _x, tt in vals:
                t = _join(t, tt)
            text = _cast(vals[-1][0], vals[-1][1], t)
            for x, tt in reversed(vals[:-1]):                              # `a and b` is b if a else a; `a or b` is a if a else b
                a = _cast(x, tt, t)
                text = f"({x} ? {text} : {a})" if isinstance(node.op, ast.And) else f"({x} ? {a} : {text})"
            return text, t
        if isinstance(node, ast.IfExp):
            c = self.expr(node.test, ctx)[0]
            a, ta = self.expr(node.body, ctx)
            b, tb = self.expr(node.orelse, ctx)
            t = _join(ta, tb)
            return f"({c} ? {_cast(a, ta, t)} : {_cast(b, tb, t)})", t
        if isinstance(node, ast.Call):
            return self.call(node, ctx)
        self.unsupported(node)

    def binop(self, node, ctx):
        a, ta = self.expr(node.left, ctx)
        b, tb = self.expr(node.right, ctx)
        t = _join(ta, tb)
        op = type(node.op)
        if op in (ast.Add, ast.Sub, ast.Mult):
            return f"({_cast(a, ta, t)} {'+' if op is ast.Add else '-' if op is ast.Sub else '*'} {_cast(b, tb, t)})", t
        if op is ast.Div:
            return f"({_cast(a, ta, 'd')} / {_cast(b, tb, 'd')})", "d"
        if op in (ast.FloorDiv, ast.Mod, ast.Pow):
            stem = {ast.FloorDiv: "grb_floordiv_", ast.Mod: "grb_mod_", ast.Pow: "grb_pow_"}[op]
            if op is ast.Pow and t == "d":
                return f"pow({_cast(a, ta, 'd')}, {_cast(b, tb, 'd')})", "d"
            self.used.add(stem + t)
            return f"{stem}{t}({_cast(a, ta, t)}, {_cast(b, tb, t)})", t
        sym = {ast.BitAnd: "&", ast.BitOr: "|", ast.BitXor: "^", ast.LShift: "<<", ast.RShift: ">>"}.get(op)
        if sym is None:
            self.err(node, f"the operator '{op.__name__}'")
        if t != "i":
            self.err(node, f"'{sym}' on a floating-point value")
        return f"({a} {sym} {b})", "i"

    def call(self, node, ctx):
        if node.keywords:
            self.err(node, "a call with keyword arguments")
        f = node.func
        if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name):
            dotted, fname = f"{f.value.id}.{f.attr}", (f.attr if f.value.id == "math" and f.value.id not in ctx["assigned"] else None)
        elif isinstance(f, ast.Name):
            dotted, fname = f.id, f.id
        else:
            self.err(node, "a call of anything but a named function")
        args = [self.expr(x, ctx) for x in node.args]
        n = len(args)

        def need(k):
            if n != k:
                self.err(node, f"{dotted} with {n} argument(s)")
        if isinstance(f, ast.Name) and fname in ctx["helpers"] and fname not in ctx["assigned"]:
            return self.helper(node, fname, ctx["helpers"][fname], args)
        if fname in ("abs", "min", "max") and isinstance(f, ast.Name) and fname not in ctx["assigned"] and fname not in self.consts:
            if fname == "abs":
                need(1)
                if args[0][1] == "d":
                    return f"fabs({args[0][0]})", "d"
                self.used.add("grb_abs_i")
                return f"grb_abs_i({args[0][0]})", "i"
            if n < 2:
                self.err(node, f"{fname} of an iterable")
            t = None
            for _x, tt in args:
                t = _join(t, tt)
            self.used.add(f"grb_{fname}_{t}")
            text = _cast(args[0][0], args[0][1], t)
            for x, tt in args[1:]:
                text = f"grb_{fname}_{t}({text}, {_cast(x, tt, t)})"
            return text, t
        if fname in _MATH and not (isinstance(f, ast.Name) and fname in ctx["assigned"]):
            if isinstance(f, ast.Name):                                     # a bare name must be math's function (or unbound: taken as it)
                bound = self.scope.get(fname, getattr(math, fname))
                if bound is not getattr(math, fname):
                    self.err(node, f"a call to {dotted} (not math.{fname})")
            d = [_cast(x, tt, "d") for x, tt in args]
            if fname == "log":
                if n == 2:
                    return f"(log({d[0]}) / log({d[1]}))", "d"
                need(1)
                return f"log({d[0]})", "d"
            if fname in _MATH1:
                need(1)
                return f"{fname}({d[0]})", "d"
            if fname in _MATH2:
                need(2)
                return f"{fname}({d[0]}, {d[1]})", "d"
            if fname in _MATHI:
                need(1)
                return f"((int64_t){fname}({d[0]}))", "i"
            need(1)
            if fname == "isnan":
                return f"((int64_t)({d[0]} != {d[0]}))", "i"
            self.used.add("grb_isinf")
            return f"grb_isinf({d[0]})", "i"
        self.err(node, f"a call to {dotted}")

    def helper(self, node, name, entry, args):
        fdef, helpers = entry
        key = (id(fdef), tuple(t for _x, t in args))
        if key in self.active:
            self.err(node, f"recursion ({name})")
        if key not in self.specs:
            self.active.append(key)
            env, ret, lines, params = self.function(fdef, [t for _x, t in args], helpers)
            self.active.pop()
            cname = f"{self.func.__name__}__{name}_{''.join(key[1]) or 'v'}"
            text = self.emit(cname, fdef, env, ret, lines, params, None)
            if key not in self.specs:
                self.order.append(text)
            self.specs[key] = (cname, ret)
        cname, ret = self.specs[key]
        return f"{cname}({', '.join(x for x, _t in args)})", ret

    def emit(self, cname, fdef, env, ret, lines, params, ctype):
        out = []
        if ctype is None:
            out.append(f"static {_C[ret]} {cname}({', '.join(f'{_C[env[p]]} v_{p}' for p in params) or 'void'}) {{")
            skip = set(params)
        elif self.select:
            out.append(f"bool {cname}(GrB_Index i, GrB_Index j, const {self.select[0]} *x, const {self.select[1]} *thunk) {{")
            skip = set()
            for p, q in zip(params, ("i", "j", "*x", "*thunk")):
                out.append(f"  {_C[env[p]]} v_{p} = ({_C[env[p]]})({q});")
                skip.add(p)
        else:
            ptrs = ["x", "y"][:len(params)]
            out.append(f"void {cname}({ctype} *z, " + ", ".join(f"const {ctype} *{p}" for p in ptrs) + ") {")
            skip = set()
            for p, q in zip(params, ptrs):
                out.append(f"  {_C[env[p]]} v_{p} = ({_C[env[p]]})(*{q});")
                skip.add(p)
        for name in sorted(env):
            if name not in skip:
                out.append(f"  {_C[env[name]]} v_{name} = 0;")
        out += lines
        out.append("}")
        return "\n".join(out)


def _parse(func):
    """(the function's `def` node, its first line, the names it can see, the int / float / bool constants among them)"""
    if not inspect.isfunction(func):
        raise TypeError("a user-defined operator is made from a plain Python function")
    try:
        lines, line0 = inspect.getsourcelines(func)
    except (OSError, TypeError) as e:
        raise TypeError(f"{getattr(func, '__name__', func)}: the function's source is not available ({e})")
    try:
        tree = ast.parse(textwrap.dedent("".join(lines)))
    except SyntaxError:                                                    # (a lambda inside a longer expression: its lines alone do not parse)
        tree = None
    if tree is None or not tree.body or not isinstance(tree.body[0], ast.FunctionDef):
        raise TypeError(f"{func.__name__}: a user-defined operator is made from a 'def' (not a lambda)")
    cv = inspect.getclosurevars(func)
    scope = dict(cv.builtins)
    scope.update(cv.globals)
    scope.update(cv.nonlocals)
    consts = {k: v for k, v in scope.items() if isinstance(v, (bool, int, float))}
    return tree.body[0], line0, scope, consts


def _base(typ):
    return "d" if typ.__name__ in ("FP32", "FP64") else "i"


def translate(func, typ, nargs):
    """The C definition (`defn` of GxB_UnaryOp_new / GxB_BinaryOp_new) of the Python function `func` as an operator on `typ`."""
    fdef, line0, scope, consts = _parse(func)
    base = _base(typ)
    tr = _Translator(func, base, line0, consts)
    tr.scope, tr.top, tr.ctype = scope, fdef, _CTYPE[typ.__name__]
    if len(fdef.args.args) != nargs:
        tr.err(fdef, f"a function of {len(fdef.args.args)} parameter(s) as {'a unary' if nargs == 1 else 'a binary'} operator")
    env, _ret, body, params = tr.function(fdef, [base] * nargs, {})
    text = tr.emit(func.__name__, fdef, env, "i", body, params, _CTYPE[typ.__name__])
    helpers = [h for name, h in _HELPERS if name in tr.used]
    return "\n".join(helpers + tr.order + [text]) + "\n"


def translate_select(func, typ, thunk_type=None):
    """The C definition (`defn` of GxB_SelectOp_new) of the Python predicate `func(i, j, x, v)`: i and j integers, x a value of `typ`, v one of `thunk_type`
    (`typ` when None); the truth of what it returns is the `bool` result."""
    fdef, line0, scope, consts = _parse(func)
    thunk_type = thunk_type or typ
    tr = _Translator(func, _base(typ), line0, consts)
    tr.scope, tr.top, tr.ctype = scope, fdef, "bool"
    tr.select = (_CTYPE[typ.__name__], _CTYPE[thunk_type.__name__])
    if len(fdef.args.args) != 4:
        tr.err(fdef, f"a function of {len(fdef.args.args)} parameter(s) as a select operator (it takes four: i, j, x, thunk)")
    env, _ret, body, params = tr.function(fdef, ["i", "i", _base(typ), _base(thunk_type)], {})
    text = tr.emit(func.__name__, fdef, env, "i", body, params, "bool")
    helpers = [h for name, h in _HELPERS if name in tr.used]
    return "\n".join(helpers + tr.order + [text]) + "\n"


def _raise(info, what):
    buf = C.create_string_buffer(1024)
    lib.GrBX_last_error(buf, C.c_int(1024))
    raise _error_codes.get(info, GraphBLASException)(buf.value.decode() or f"{what}: GrB_Info {info}")


class _UserOp:
    def _setup(self, kind, func, typ, h, defn):
        self.kind, self.cname, self.name, self.type = kind, func.__name__, func.__name__, typ
        self._h, self._token = h.value, None
        self.func, self.defn = func, defn

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            self._h = None
            self._free(C.byref(C.c_void_p(h)))

    def __repr__(self):
        return f"<User{self.kind} {self.type.__name__}.{self.name}>"


class UserUnaryOp(_UserOp, types.UnaryOp):
    """A unary operator compiled from a Python function (`@unary_op(T)`)."""
    _free = staticmethod(lambda ref: lib.GrB_UnaryOp_free(ref))

    def __init__(self, func, typ, defn=None):
        defn = defn if defn is not None else translate(func, typ, 1)
        h, t = C.c_void_p(), C.c_void_p(typ._h)
        info = lib.GxB_UnaryOp_new(C.byref(h), None, t, t, func.__name__.encode(), defn.encode())
        if info:
            _raise(info, "GxB_UnaryOp_new")
        self._setup("UnaryOp", func, typ, h, defn)


class UserBinaryOp(_UserOp, types.BinaryOp):
    """A binary operator compiled from a Python function (`@binary_op(T)`); as a context manager it is the default eWise operator."""
    _free = staticmethod(lambda ref: lib.GrB_BinaryOp_free(ref))

    def __init__(self, func, typ, defn=None):
        defn = defn if defn is not None else translate(func, typ, 2)
        h, t = C.c_void_p(), C.c_void_p(typ._h)
        info = lib.GxB_BinaryOp_new(C.byref(h), None, t, t, t, func.__name__.encode(), defn.encode())
        if info:
            _raise(info, "GxB_BinaryOp_new")
        self._setup("BinaryOp", func, typ, h, defn)


class UserSelectOp(_UserOp, types.SelectOp):
    """A select operator compiled from a Python predicate (`@select_op(T, thunk_type)`): `A.select(op, thunk)`."""
    _free = staticmethod(lambda ref: lib.GxB_SelectOp_free(ref))

    def __init__(self, func, typ, thunk_type=None, defn=None):
        defn = defn if defn is not None else translate_select(func, typ, thunk_type)
        h = C.c_void_p()
        info = lib.GxB_SelectOp_new(C.byref(h), None, C.c_void_p(typ._h), C.c_void_p(thunk_type._h) if thunk_type is not None else None,
                                    func.__name__.encode(), defn.encode())
        if info:
            _raise(info, "GxB_SelectOp_new")
        self._setup("SelectOp", func, typ, h, defn)
        self.thunk_type = thunk_type or typ


class UserMonoid(types.Monoid):
    """`T.new_monoid(op, identity)`: a monoid over a user-defined or (expressible) built-in binary operator (GrBX_Monoid_new_user).  Holds a reference to its
    operator — the C object keeps a pointer to it — and frees its handle on collection."""

    def __init__(self, typ, op, identity):
        if not isinstance(op, types.BinaryOp):
            raise TypeError(f"new_monoid takes a binary operator, not {type(op).__name__}")
        if op.type._h != typ._h:      # (the identity is packed as this class's C type: the operator's type must be the class's)
            raise DomainMismatch(f"{typ.__name__}.new_monoid: operator {op.name} is of type {op.type.__name__}")
        h = C.c_void_p()
        info = lib.GrBX_Monoid_new_user(C.byref(h), C.c_void_p(op.get_op()), C.byref(typ._c(identity)))
        if info:
            _raise(info, "GrBX_Monoid_new_user")
        self.kind, self.cname, self.name, self.type = "Monoid", f"user_{op.name}", f"{op.name}_MONOID", typ
        self._h, self._token = h.value, None
        self.op, self.identity = op, identity

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            self._h = None
            lib.GrB_Monoid_free(C.byref(C.c_void_p(h)))

    def __repr__(self):
        return f"<UserMonoid {self.type.__name__}.{self.name}>"


class UserSemiring(types.Semiring):
    """`T.new_semiring(monoid, op)`: a semiring at least one of whose operators is user-defined (GrBX_Semiring_new_user); a `semiring=` argument, a context
    manager (`with sr: A @ B`) and a callable (`sr(A, B)`) like the built-in ones.  Holds references to its monoid and multiplier."""

    def __init__(self, typ, monoid, op):
        if not isinstance(monoid, types.Monoid) or not isinstance(op, types.BinaryOp):
            raise TypeError("new_semiring takes a monoid and a binary operator")
        for what in (monoid, op):
            if what.type._h != typ._h:
                raise DomainMismatch(f"{typ.__name__}.new_semiring: {what.kind} {what.name} is of type {what.type.__name__}")
        h = C.c_void_p()
        info = lib.GrBX_Semiring_new_user(C.byref(h), C.c_void_p(monoid.get_op()), C.c_void_p(op.get_op()))
        if info:
            _raise(info, "GrBX_Semiring_new_user")
        self.kind, self.cname, self.type = "Semiring", f"user_{monoid.name}_{op.name}", typ
        self.name = f"{monoid.name[:-7] if monoid.name.endswith('_MONOID') else monoid.name}_{op.name}"
        self._h, self._token = h.value, None
        self.monoid, self.op = monoid, op

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            self._h = None
            lib.GrB_Semiring_free(C.byref(C.c_void_p(h)))

    def __repr__(self):
        return f"<UserSemiring {self.type.__name__}.{self.name}>"


def unary_op(arg_type):
    """Decorator: a Python function of one argument -> a `GrB_UnaryOp` on `arg_type` (reference: pygraphblas/unaryop.py:101)."""
    def inner(func):
        return UserUnaryOp(func, arg_type)
    return inner


def binary_op(arg_type, nopython=True):
    """Decorator: a Python function of two arguments -> a `GrB_BinaryOp` on `arg_type` (reference: pygraphblas/binaryop.py:137;
    `nopython` is accepted for the reference's call shape and has no meaning here)."""
    def inner(func):
        return UserBinaryOp(func, arg_type)
    return inner


def select_op(arg_type, thunk_type=None):
    """Decorator: a Python predicate `f(i, j, x, v)` -> a `GxB_SelectOp` on values of `arg_type` with a thunk of `thunk_type`
    (`arg_type` when None) (reference: pygraphblas/selectop.py:103)."""
    def inner(func):
        return UserSelectOp(func, arg_type, thunk_type)
    return inner
