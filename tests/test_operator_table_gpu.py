"""Every exported unary / binary / monoid handle of the 11 real types, and all 121 typecasts, on the device against tests/operator_model.py over the
fixed edge values (operator_model.edge_values), through every route that writes the arithmetic out again: vector and matrix eWise, bound apply, the
accumulator, the chain interpreter and the hipRTC chain compiler, apply, the three SpMV routes, vxm, mxm, and the reductions.

Comparison: everything is exact (the value lies in the model's accepted set, NaN matches NaN, the sign of zero counts) except the math-library operators
(operator_model.MATH_BINOPS / MATH_UNOPS): FP64 within relative 1e-12 of the model's double (one subnormal spacing where the result is subnormal: the
format holds no more), FP32 within one float32 ulp of the model's double rounded to float32 — only where that double is finite and the argument is not
within 1e-3 of a zero of the function; non-finite results and exact zeros match exactly there too.

LOOSENED holds the math-library operators that miss 1e-12 on the MI355X because of the device math library's own accuracy:
    (operator, type): (largest relative error measured over the edge set, bound = twice that, reason)
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import operator_model as M

pytestmark = pytest.mark.gpu

LOOSENED = {}

# handles that are not checked here: only positional operators, complex-type stubs and user-defined placeholders may be listed
EXCLUDED = {name: "positional operator: covered by test_positional_unary_operators"
            for name in [f"GxB_POSITION{p}_{t}" for p in ("I", "I1", "J", "J1") for t in ("INT32", "INT64")]}

CHECKED = set()
MAX_ERR = {}
_T = "BOOL|UINT8|UINT16|UINT32|UINT64|INT8|INT16|INT32|INT64|FP32|FP64"
_name_re = re.compile(rf"^(?:GxB|GrB)_([A-Z0-9]+?)(?:_MONOID)?_({_T})(?:_MONOID)?$")
CHAIN_TYPES = ["INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]       # the chains hold the 4- and 8-byte types (grb_lazy.hpp)
JIT_TYPES = ["INT32", "UINT64", "FP32", "FP64"]                            # hipRTC: one integer and one floating-point type per width


def parse(cname):
    """(operator, type) of an exported handle name, the way pygraphblas_amd/types.py::_build reads them; None when it is not of the 11 real types."""
    if cname in ("GrB_LNOT", "GrB_LOR", "GrB_LAND", "GrB_LXOR", "GrB_LXNOR"):
        return cname[4:], "BOOL"
    m = _name_re.match(cname)
    return m.groups() if m else None


def handles(gb, kind):
    return [(c,) + parse(c) for c in gb._capi.names[kind] if parse(c) and c not in EXCLUDED]


# ---- model tables --------------------------------------------------------------------------------------------------------------------------------
class Table:
    """Accepted results of one operator over an operand list as arrays: exp0 / exp1 (the two accepted values; equal when unique), `free` where the
    value is unspecified, and for a math-library operator m64 (the model's double) and `near` (argument near a zero of the function)."""

    def __init__(self, zt, results, m64=None, near=None):
        self.zt = zt
        self.exp0 = np.array([r[0] if r[0] is not M.UNSPECIFIED else 0 for r in results], M.NP[zt])
        self.exp1 = np.array([r[-1] if r[-1] is not M.UNSPECIFIED else 0 for r in results], M.NP[zt])
        self.free = np.array([r[0] is M.UNSPECIFIED for r in results], bool)
        self.m64 = None if m64 is None else np.array(m64, np.float64)
        self.near = None if near is None else np.array(near, bool)

    def take(self, idx):
        t = object.__new__(Table); t.zt = self.zt
        for k in ("exp0", "exp1", "free", "m64", "near"):
            v = getattr(self, k); setattr(t, k, None if v is None else v[idx])
        return t

    def either_zero(self):
        """Where the result is a zero, accept both: under a floating-point PLUS monoid the identity +0 may take part, and (+0) + (-0) = +0."""
        t = self.take(np.arange(len(self.exp0))); t.any_zero = (t.exp0 == 0) | (t.exp1 == 0)
        return t

    def cast(self, tt):
        """The results cast into another type (an accumulator's BOOL result stored into its vector)."""
        t = object.__new__(Table); t.zt = tt; t.free = self.free; t.m64 = self.m64 if tt == self.zt else None; t.near = self.near if tt == self.zt else None
        conv = lambda a: np.array([M.cast(self.zt, tt, v.item() if self.zt != "FP32" else v) for v in a], M.NP[tt])
        t.exp0, t.exp1 = (self.exp0, self.exp1) if tt == self.zt else (conv(self.exp0), conv(self.exp1))
        return t


def py(t, v):
    """A numpy element as a model value."""
    return bool(v) if t == "BOOL" else (int(v) if M.is_int(t) else v)


def arr(t, values):
    return np.array(values, M.NP[t])


def _zero_near1(f, x):
    if not math.isfinite(x): return False
    with np.errstate(all="ignore"):
        v = [float(f(p)) for p in (x, x - 1e-3, x + 1e-3, x * (1 - 1e-3), x * (1 + 1e-3))]
    v = [w for w in v if w == w]
    return any(w == 0 for w in v) or (min(v) < 0 < max(v) if v else False)


_tables = {}


def binop_table(op, t):
    """Over all ordered pairs of the type's edge values: index i * len(E) + j is op(E[i], E[j])."""
    key = ("b", op, t)
    if key not in _tables:
        E = M.edge_values(t); pairs = [(a, b) for a in E for b in E]
        res = [M.binop(op, t, a, b) for a, b in pairs]
        m64 = near = None
        if op in M.MATH_BINOPS and M.is_fp(t):
            m64 = [M.binop_math64(op, t, a, b) for a, b in pairs]
            near = [_zero_near1(lambda p: M.binop_math64(op, t, p, b), float(a)) or _zero_near1(lambda p: M.binop_math64(op, t, a, p), float(b)) for a, b in pairs]
        _tables[key] = Table(M.binop_ztype(op, t), res, m64, near)
    return _tables[key]


def unop_table(op, t):
    key = ("u", op, t)
    if key not in _tables:
        E = M.edge_values(t); m64 = near = None
        if op in M.MATH_UNOPS:
            m64 = [M.fp_math1(op, x) for x in E]; near = [_zero_near1(lambda p: M.fp_math1(op, p), float(x)) for x in E]
        _tables[key] = Table(t, [M.unop(op, t, x) for x in E], m64, near)
    return _tables[key]


def pair_operands(t):
    E = M.edge_values(t)
    return arr(t, [a for a in E for b in E]), arr(t, [b for a in E for b in E])


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
    return a == b


def check(what, got, tab, name=None):
    """`got` against a Table by the rules in the module docstring."""
    got = np.ascontiguousarray(got, M.NP[tab.zt]); assert got.shape == tab.exp0.shape, (what, got.shape, tab.exp0.shape)
    ok = _same(got, tab.exp0) | _same(got, tab.exp1) | tab.free
    if getattr(tab, "any_zero", None) is not None:
        ok = ok | (tab.any_zero & (got == 0))
    if tab.m64 is not None:
        f32 = tab.zt == "FP32"
        with np.errstate(all="ignore"):
            ref = tab.m64.astype(np.float32).astype(np.float64) if f32 else tab.m64
            g = got.astype(np.float64); err = np.abs(g - ref)
            bounded = np.isfinite(ref) & (ref != 0) & ~tab.near                                    # where the bound is evaluated
            if f32:
                tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
            else:
                rel = LOOSENED[(name, tab.zt)][1] if (name, tab.zt) in LOOSENED else 1e-12
                tol = np.maximum(rel * np.abs(ref), 5e-324)
            rel_err = np.where(bounded & np.isfinite(g), err / np.abs(ref), 0.0)
            if name is not None and rel_err.size:
                MAX_ERR[(name, tab.zt)] = max(MAX_ERR.get((name, tab.zt), 0.0), float(rel_err.max()))
            ok = ok | (bounded & np.isfinite(g) & (err <= tol))
            ok = ok | (tab.near & np.isfinite(ref) & np.isfinite(g) & ((g != 0) | (ref != 0) | (np.signbit(g) == np.signbit(ref))) & (np.abs(g - ref) <= 1e-2))
    if not ok.all():
        bad = np.flatnonzero(~ok)[:6]
        pytest.fail(f"{what}: {int((~ok).sum())} of {ok.size} differ; first at {bad.tolist()}: device {got[bad]!r}, model {tab.exp0[bad]!r} / {tab.exp1[bad]!r}")


class Collect:
    """Runs one handle's checks and keeps going after a mismatch, so that one run reports every operator that differs."""

    def __init__(self): self.errors = []

    def __call__(self, cname, fn, *args, **kw):
        try:
            r = fn(*args, **kw)
        except (AssertionError, pytest.fail.Exception) as e:
            self.errors.append(f"{cname}: {str(e)[:600]}"); return None
        return r

    def done(self):
        assert not self.errors, f"{len(self.errors)} handle(s) differ from the model:\n" + "\n".join(self.errors)


# ---- device plumbing -----------------------------------------------------------------------------------------------------------------------------
def TY(gb, t): return getattr(gb, t)
def full_vec(gb, t, values): return gb.Vector.from_dense_array(np.ascontiguousarray(values, M.NP[t]), TY(gb, t))
def dense(v):
    x, p = v.to_dense_arrays(); return x, p != 0


def full_mat(gb, t, values, nrows, ncols):
    I, J = np.divmod(np.arange(nrows * ncols, dtype=np.uint64), np.uint64(ncols))
    return gb.Matrix.from_arrays(I, J, np.ascontiguousarray(values, M.NP[t]), nrows, ncols, TY(gb, t))


def mat_values(m):
    """Row-major values of a matrix and its flat positions."""
    I, J, X = m.to_arrays(); o = np.lexsort((J, I))
    return (I[o] * np.uint64(m.ncols) + J[o]).astype(np.int64), X[o]


def op_obj(gb, kind, cname, op, t):
    return getattr(gb.types, kind)(cname, op, TY(gb, t))


def mat_apply_bound(gb, which, op, A, scalar, out):
    t = A.type.__name__
    fn = getattr(gb.lib, f"GxB_Matrix_apply_BinaryOp{which}_{t}")
    s = A.type._c(scalar)
    args = (out._h, None, None, C.c_void_p(op.get_op())) + ((s, A._h) if which == "1st" else (A._h, s)) + (None,)
    gb.base.check(fn(*args), out)
    return out


def scalar_of(t, v):
    return v.item() if hasattr(v, "item") else v


# ---- (a)-(e): every binary handle ---------------------------------------------------------------------------------------------------------------
def binary_routes(gb, cname, op, t, chain=False):
    """Routes (a) vector emult, (b) vector eadd with pass-through, (c) matrix emult / eadd, (d) bound apply, (e) the accumulator; with `chain` the
    vector routes (a), (b), (d) followed by a second step, so that they run as one chain.  Returns the results for bit-for-bit comparison between modes."""
    T = TY(gb, t); tab = binop_table(op, t); zt = tab.zt; Z = TY(gb, zt)
    B = op_obj(gb, "BinaryOp", cname, op, t); E = M.edge_values(t); ne = len(E); X, Y = pair_operands(t); n = len(X)
    Ev = arr(t, E); out = []
    fin = (lambda r: r.emult(r, Z.FIRST, out=gb.Vector.sparse(Z, r.size))) if chain else (lambda r: r)
    x, y = full_vec(gb, t, X), full_vec(gb, t, Y)
    # (a)
    g, p = dense(fin(x.emult(y, B, out=gb.Vector.sparse(Z, n))))
    assert p.all(); check(f"{cname} vector emult chain={chain}", g, tab, op); out.append(g)
    # (b) positions 0 .. n-1 hold both operands, n .. 2n-1 only x at even and only y at odd offsets, 2n .. 2n+3 neither
    idx = np.arange(n, dtype=np.uint64); ex, ey = idx[::2], idx[1::2]
    xs = gb.Vector.from_arrays(np.concatenate([idx, n + ex]), np.concatenate([X, X[::2]]), 2 * n + 4, T)
    ys = gb.Vector.from_arrays(np.concatenate([idx, n + ey]), np.concatenate([Y, Y[1::2]]), 2 * n + 4, T)
    g, p = dense(fin(xs.eadd(ys, B, out=gb.Vector.sparse(Z, 2 * n + 4))))
    assert p[:2 * n].all() and not p[2 * n:].any(), f"{cname} vector eadd pattern"
    check(f"{cname} vector eadd chain={chain}", g[:n], tab, op); out.append(g[:2 * n])
    thru = np.empty(n, M.NP[t]); thru[::2] = X[::2]; thru[1::2] = Y[1::2]
    want = thru if zt == t else arr(zt, [M.cast(t, zt, py(t, v)) for v in thru])
    check(f"{cname} vector eadd pass-through chain={chain}", g[n:2 * n], Table(zt, [(v,) for v in want]))
    # (d) vector
    ev = full_vec(gb, t, Ev)
    for k, s in enumerate(E):
        g, p = dense(fin(ev.apply_first(scalar_of(t, s), B, out=gb.Vector.sparse(Z, ne))))
        assert p.all(); check(f"{cname} vector apply_first({s!r}) chain={chain}", g, tab.take(np.arange(ne) + k * ne), op); out.append(g)
        g, p = dense(fin(ev.apply_second(B, scalar_of(t, s), out=gb.Vector.sparse(Z, ne))))
        assert p.all(); check(f"{cname} vector apply_second({s!r}) chain={chain}", g, tab.take(np.arange(ne) * ne + k), op); out.append(g)
    if chain:
        return out
    # (c) the same pairs as an ne x ne matrix; eadd gets ne more columns that hold A only (even rows) or B only (odd rows)
    A, Bm = full_mat(gb, t, X, ne, ne), full_mat(gb, t, Y, ne, ne)
    pos, g = mat_values(A.emult(Bm, B, out=gb.Matrix.sparse(Z, ne, ne)))
    assert np.array_equal(pos, np.arange(n)); check(f"{cname} matrix emult", g, tab, op)
    I, J = np.divmod(np.arange(n, dtype=np.uint64), np.uint64(ne)); ev_rows, od_rows = (I % 2 == 0), (I % 2 == 1)
    A2 = gb.Matrix.from_arrays(np.concatenate([I, I[ev_rows]]), np.concatenate([J, J[ev_rows] + ne]), np.concatenate([X, X[ev_rows]]), ne, 2 * ne, T)
    B2 = gb.Matrix.from_arrays(np.concatenate([I, I[od_rows]]), np.concatenate([J, J[od_rows] + ne]), np.concatenate([Y, Y[od_rows]]), ne, 2 * ne, T)
    Cm = A2.eadd(B2, B, out=gb.Matrix.sparse(Z, ne, 2 * ne)); ci, cj, cx = Cm.to_arrays()
    d = np.zeros((ne, 2 * ne), M.NP[zt]); pm = np.zeros((ne, 2 * ne), bool); d[ci.astype(int), cj.astype(int)] = cx; pm[ci.astype(int), cj.astype(int)] = True
    assert pm.all(), f"{cname} matrix eadd pattern"
    check(f"{cname} matrix eadd", d[:, :ne].reshape(-1), tab, op)
    thru = np.where(ev_rows, X, Y); want = thru if zt == t else arr(zt, [M.cast(t, zt, py(t, v)) for v in thru])
    check(f"{cname} matrix eadd pass-through", d[:, ne:].reshape(-1), Table(zt, [(v,) for v in want]))
    # (d) matrix: the edge values as a 1 x ne and an ne x 1 matrix
    Er, Ec = full_mat(gb, t, Ev, 1, ne), full_mat(gb, t, Ev, ne, 1)
    for k, s in enumerate(E):
        _, g = mat_values(mat_apply_bound(gb, "1st", B, Er, scalar_of(t, s), gb.Matrix.sparse(Z, 1, ne)))
        check(f"{cname} matrix apply_first({s!r})", g, tab.take(np.arange(ne) + k * ne), op)
        _, g = mat_values(mat_apply_bound(gb, "2nd", B, Ec, scalar_of(t, s), gb.Matrix.sparse(Z, ne, 1)))
        check(f"{cname} matrix apply_second({s!r})", g, tab.take(np.arange(ne) * ne + k), op)
    # (e) w = accum(w, scalar), w = accum(w, IDENTITY(y)), and w = accum(w, FIRST(y, y)) with and without the one-pass eWise; the operator's result is
    # cast into w's type
    tabw = tab.cast(t)
    for k, s in enumerate(E):
        w = full_vec(gb, t, Ev); w.assign_scalar(scalar_of(t, s), accum=B)
        g, p = dense(w); assert p.all(); check(f"{cname} assign_scalar({s!r}, accum)", g, tabw.take(np.arange(ne) * ne + k), op)
    w = full_vec(gb, t, X); y.apply(T.IDENTITY, out=w, accum=B)
    g, p = dense(w); assert p.all(); check(f"{cname} apply(IDENTITY, accum)", g, tabw, op)
    for fused in ("1", "0"):
        os.environ["GRB_MI355X_EWISE_FUSED"] = fused
        try:
            w = full_vec(gb, t, X); y.emult(y, T.FIRST, out=w, accum=B)
            g, p = dense(w)
        finally:
            os.environ.pop("GRB_MI355X_EWISE_FUSED", None)
        assert p.all(); check(f"{cname} emult(FIRST, accum) fused={fused}", g, tabw, op)
    return out


@pytest.mark.parametrize("t", M.TYPES)
def test_binary_operators(gb, gpu, t):
    hs = [h for h in handles(gb, "GrB_BinaryOp") if h[2] == t]
    assert sorted({h[1] for h in hs}) == sorted(M.binops_of(t)), "the model and the registry disagree about the binary operators of " + t
    col = Collect()
    for cname, op, _ in hs:
        if col(cname, binary_routes, gb, cname, op, t) is not None:
            CHECKED.add(cname)
    col.done()


@pytest.mark.parametrize("t", CHAIN_TYPES)
def test_binary_operators_as_chains(gb, gpu, t, monkeypatch, tmp_path):
    """Route (f): the vector routes as two-step chains through the interpreter (GRB_MI355X_CHAIN_JIT=0) and, for one integer and one floating-point type
    per width, through hipRTC (=2, every kernel really compiled: an empty cache) — each against the model, and the two bit for bit."""
    monkeypatch.setenv("GRB_MI355X_CACHE_DIR", str(tmp_path))
    col = Collect()

    def one(cname, op):
        res = {}
        for mode in ("0", "2") if t in JIT_TYPES else ("0",):
            monkeypatch.setenv("GRB_MI355X_CHAIN_JIT", mode)
            res[mode] = binary_routes(gb, cname, op, t, chain=True)
        if "2" in res:
            for k, (a0, a2) in enumerate(zip(res["0"], res["2"])):
                assert a0.tobytes() == a2.tobytes() or np.array_equal(a0, a2, equal_nan=(a0.dtype.kind == "f")), (cname, "interpreter and hipRTC differ", k)
    for cname, op, _ in [h for h in handles(gb, "GrB_BinaryOp") if h[2] == t]:
        col(cname, one, cname, op)
    col.done()


# ---- (g): every unary handle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", M.TYPES)
def test_unary_operators(gb, gpu, t):
    hs = [h for h in handles(gb, "GrB_UnaryOp") if h[2] == t]
    assert sorted({h[1] for h in hs}) == sorted(M.unops_of(t)), "the model and the registry disagree about the unary operators of " + t
    T = TY(gb, t); E = arr(t, M.edge_values(t)); ne = len(E)
    col = Collect()

    def one(cname, op):
        U = op_obj(gb, "UnaryOp", cname, op, t); tab = unop_table(op, t)
        v = full_vec(gb, t, E)
        g, p = dense(v.apply(U)); assert p.all(); check(f"{cname} vector apply", g, tab, op)
        v.apply(U, out=v); g, p = dense(v); assert p.all(); check(f"{cname} vector apply in place", g, tab, op)
        for shape in ((1, ne), (ne, 1)):
            A = full_mat(gb, t, E, *shape)
            _, g = mat_values(A.apply(U)); check(f"{cname} matrix apply {shape}", g, tab, op)
            A.apply(U, out=A); _, g = mat_values(A); check(f"{cname} matrix apply in place {shape}", g, tab, op)
        return True
    for cname, op, _ in hs:
        if col(cname, one, cname, op):
            CHECKED.add(cname)
    col.done()


# ---- (h): the 121 typecasts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", M.TYPES)
def test_typecasts_on_edge_values(gb, gpu, ft):
    E = M.edge_values(ft); Ev = arr(ft, E); ne = len(E); F = TY(gb, ft)
    perm = np.arange(ne - 1, -1, -1, dtype=np.uint64)
    for tt in M.TYPES:
        Tt = TY(gb, tt)
        want = Table(tt, [(M.cast(ft, tt, v),) for v in E])
        g, p = dense(full_vec(gb, ft, Ev).apply(Tt.IDENTITY, out=gb.Vector.sparse(Tt, ne)))
        assert p.all(); check(f"cast {ft} -> {tt} by apply(IDENTITY)", g, want)
        _, g = mat_values(full_mat(gb, ft, Ev, 1, ne).apply(Tt.IDENTITY, out=gb.Matrix.sparse(Tt, 1, ne)))
        check(f"cast {ft} -> {tt} by matrix apply(IDENTITY)", g, want)
        for mt in M.TYPES:                                              # operands ft, operator mt, output tt
            Mt = TY(gb, mt)
            want2 = Table(tt, [(M.cast(mt, tt, M.cast(ft, mt, v)),) for v in E])
            x = full_vec(gb, ft, Ev)
            g, p = dense(x.emult(x, Mt.FIRST, out=gb.Vector.sparse(Tt, ne)))
            assert p.all(); check(f"cast {ft} -> {mt} -> {tt} by emult(FIRST)", g, want2)
            # mxv: one entry per row (row i holds E[i] in column ne-1-i), semiring of type mt, output of type tt
            A = gb.Matrix.from_arrays(np.arange(ne, dtype=np.uint64), perm, Ev, ne, ne, F)
            u = full_vec(gb, ft, Ev[::-1].copy())
            sr = getattr(Mt, "LOR_FIRST" if mt == "BOOL" else "PLUS_FIRST")
            g, p = dense(A.mxv(u, semiring=sr, out=gb.Vector.sparse(Tt, ne)))
            assert p.all(); check(f"cast {ft} -> {mt} -> {tt} by mxv(FIRST)", g, want2)
            sr = getattr(Mt, "LOR_SECOND" if mt == "BOOL" else "PLUS_SECOND")
            g, p = dense(A.mxv(u, semiring=sr, out=gb.Vector.sparse(Tt, ne)))
            assert p.all(); check(f"cast {ft} -> {mt} -> {tt} by mxv(SECOND)", g, want2)


# ---- (i): semiring multipliers -------------------------------------------------------------------------------------------------------------------
def admitted(op, t):
    """The multipliers the semiring kernels take (grb_ops.hpp::semiring_op_supported, restated): FIRST .. LXOR without the math-library POW, the integer
    bitwise operators, and on BOOL everything up to LXNOR (a comparison's result is a BOOL like its arguments there)."""
    if t == "BOOL": return True
    return (op in M.ARITH and op != "POW") or op in M.IS_CMP or op in M.LOGIC or (M.is_int(t) and op in ("BOR", "BAND", "BXOR", "BXNOR"))


def new_semiring(gb, monoid_cname, binop_cname):
    sr = C.c_void_p()
    info = gb.lib.GrB_Semiring_new(C.byref(sr), C.c_void_p(gb._capi.handle(monoid_cname)), C.c_void_p(gb._capi.handle(binop_cname)))
    return info, sr


@pytest.mark.parametrize("t", M.TYPES)
def test_semiring_multipliers(gb, gpu, t, monkeypatch):
    """One entry per row, so no reduction takes part: row i of A holds X[i] in column n-1-i and u[n-1-i] = Y[i].  Each multiplier under two monoids
    (so that the compile-time specialised semirings and the dynamic switch both run), through mxv on the three SpMV routes, vxm and mxm."""
    T = TY(gb, t); X, Y = pair_operands(t); n = len(X); rows = np.arange(n, dtype=np.uint64); perm = rows[::-1].copy()
    A = gb.Matrix.from_arrays(rows, perm, X, n, n, T); u = full_vec(gb, t, Y[::-1].copy())              # mxv: op(A(i,k), u(k))
    ux = full_vec(gb, t, X); Ay = gb.Matrix.from_arrays(rows, perm, Y, n, n, T)                          # vxm: op(u(i), A(i,j)) lands in column n-1-i
    By = gb.Matrix.from_arrays(perm, rows, Y, n, n, T)                                                   # mxm: A(i,n-1-i) * B(n-1-i,i) lands on the diagonal
    monoids = ("GrB_LOR_MONOID_BOOL", "GrB_LAND_MONOID_BOOL") if t == "BOOL" else (f"GrB_PLUS_MONOID_{t}", f"GrB_MIN_MONOID_{t}")
    col = Collect()

    def one(cname, op):
        tab = binop_table(op, t)
        if not admitted(op, t):
            info, sr = new_semiring(gb, monoids[0] if tab.zt == t else "GrB_LOR_MONOID_BOOL", cname); assert info == 0, (cname, info)
            w = gb.Vector.sparse(TY(gb, tab.zt), n)
            assert gb.lib.GrB_mxv(w._h, None, None, sr, A._h, u._h, None) == 5, cname                   # GrB_INVALID_VALUE
            msg = C.c_char_p(); gb.lib.GrB_Vector_error(C.byref(msg), w._h)
            assert b"not implemented" in msg.value and w.nvals == 0, cname
            gb.lib.GrB_Semiring_free(C.byref(sr))
            return
        for mon in monoids:
            info, sr = new_semiring(gb, mon, cname); assert info == 0, (cname, mon, info)
            tabt = tab.cast(t).either_zero() if M.is_fp(t) and "PLUS" in mon else tab.cast(t)      # (the MIN monoid keeps the sign check: fmin(inf, -0) = -0)
            for method in ("adaptive", "rowgroup", "push"):
                monkeypatch.setenv("GRB_MI355X_SPMV", method)
                w = gb.Vector.sparse(T, n); gb.base.check(gb.lib.GrB_mxv(w._h, None, None, sr, A._h, u._h, None), w)
                g, p = dense(w); assert p.all(); check(f"{cname} under {mon}: mxv {method}", g, tabt, op)
                w = gb.Vector.sparse(T, n); gb.base.check(gb.lib.GrB_vxm(w._h, None, None, sr, ux._h, Ay._h, None), w)
                g, p = dense(w); assert p.all(); check(f"{cname} under {mon}: vxm {method}", g[::-1], tabt, op)
            monkeypatch.delenv("GRB_MI355X_SPMV")
            Cm = gb.Matrix.sparse(T, n, n); gb.base.check(gb.lib.GrB_mxm(Cm._h, None, None, sr, A._h, By._h, None), Cm)
            ci, cj, cx = Cm.to_arrays(); o = np.argsort(ci)
            assert np.array_equal(ci[o], rows) and np.array_equal(cj[o], rows), f"{cname} under {mon}: mxm pattern"
            check(f"{cname} under {mon}: mxm", cx[o], tabt, op)
            gb.lib.GrB_Semiring_free(C.byref(sr))
    for cname, op, _ in [h for h in handles(gb, "GrB_BinaryOp") if h[2] == t]:
        col(cname, one, cname, op)
        monkeypatch.delenv("GRB_MI355X_SPMV", raising=False)
    col.done()


# ---- (j): every monoid handle --------------------------------------------------------------------------------------------------------------------
def monoid_rows(op, t, rng):
    """Rows of 1, 2, 9, 65 and 300 values (the lane-per-row prefix, a row group and beyond) and the results the model accepts for each."""
    E = M.edge_values(t); rows = []
    if M.is_fp(t) and op in ("PLUS", "TIMES"):
        # finite values whose partial results are exact in every order (sums of multiples of 1/2; products of +-1 and a few +-1/2), then rows with inf / NaN
        f = M.NP[t]; pool = [f(v) for v in ((0.5, -0.5, 1.0, -1.0, 2.5, -2.5, 3.0, 0.0, -0.0) if op == "PLUS" else (1.0, -1.0))]
        for k in (1, 2, 9, 65, 300):
            vals = [pool[i] for i in rng.integers(0, len(pool), k)]
            if op == "TIMES":
                for i in rng.integers(0, k, min(k, 6)): vals[i] = f(0.5) if i % 2 else f(-0.5)
            rows.append(vals)
        inf, nan = f(math.inf), f(math.nan)
        rows += [[f(1), inf, f(0.5)], [inf, -inf], [nan, f(1)], [f(-1), inf, f(3)], [inf, f(0.0)], [f(2.5), nan, inf]]
        out = []
        for vals in rows:
            r = M.fold(op, t, vals)
            if len(r) == 1 and r[0] == 0 and op == "PLUS": r = (f(0.0), f(-0.0))          # (the identity +0 may take part in the sum: -0 + 0 = +0)
            out.append((vals, r))
        return out
    for k in (1, 2, 9, 65, 300):
        rows.append([E[i] for i in rng.integers(0, len(E), k)])
    rows.append(list(E))
    if M.is_fp(t):
        f = M.NP[t]; rows += [[f(math.nan)] * 3, [f(0.0), f(-0.0)], [f(math.nan), f(-0.0), f(0.0), f(math.nan)]]
        out = []
        for vals in rows:                                                # MIN / MAX: a NaN is omitted, all NaN gives NaN, the two zeros are not ordered
            if op == "ANY": out.append((vals, M.fold(op, t, vals))); continue
            real = [v for v in vals if v == v]
            if not real: out.append((vals, (f(math.nan),))); continue
            m = min(real) if op == "MIN" else max(real)
            out.append((vals, tuple({math.copysign(1.0, v): v for v in real if v == m}.values())))
        return out
    return [(vals, M.fold(op, t, vals)) for vals in rows]


def reduce_scalar(gb, kind, t, mon, obj):
    out = TY(gb, t)._c(0)
    gb.base.check(getattr(gb.lib, f"GrB_{kind}_reduce_{t}")(C.byref(out), None, C.c_void_p(mon.get_op()), obj._h, None), obj)
    return out.value


@pytest.mark.parametrize("t", M.TYPES)
def test_monoids(gb, gpu, t, monkeypatch):
    hs = [h for h in handles(gb, "GrB_Monoid") if h[2] == t]
    assert sorted({h[1] for h in hs}) == sorted(M.monoids_of(t)), "the model and the registry disagree about the monoids of " + t
    T = TY(gb, t); f = (lambda v: py(t, M.NP[t](v)))
    col = Collect()

    def one(cname, op):
        mon = op_obj(gb, "Monoid", cname, op, t); rng = np.random.default_rng(7)
        rows = monoid_rows(op, t, rng); width = max(len(v) for v, _ in rows)
        # the identity: what the reduction of nothing returns
        got = reduce_scalar(gb, "Vector", t, mon, gb.Vector.sparse(T, 10))
        assert M.same(f(got), M.monoid_identity(op, t)), (cname, "identity", got)
        # reduce to a scalar: a vector, and a one-row matrix
        for vals, want in rows:
            got = reduce_scalar(gb, "Vector", t, mon, full_vec(gb, t, arr(t, vals)))
            assert M.accepted(f(got), want), (cname, "vector reduce", len(vals), got, want)
            got = reduce_scalar(gb, "Matrix", t, mon, full_mat(gb, t, arr(t, vals), 1, len(vals)))
            assert M.accepted(f(got), want), (cname, "matrix reduce", len(vals), got, want)
        # the rows as one matrix (row 1 stays empty): row-reduce to a vector, and the monoid as the add of a semiring with FIRST as multiplier
        ri = [0] + list(range(2, len(rows) + 1)); nr = len(rows) + 1
        I = np.concatenate([np.full(len(v), r, np.uint64) for r, (v, _) in zip(ri, rows)])
        J = np.concatenate([np.arange(len(v), dtype=np.uint64) for v, _ in rows]); Xv = np.concatenate([arr(t, v) for v, _ in rows])
        A = gb.Matrix.from_arrays(I, J, Xv, nr, width, T)

        def rows_ok(w, what):
            g, p = dense(w)
            assert np.array_equal(np.flatnonzero(p), ri), (cname, what, "pattern (an empty row produces no entry)")
            for r, (vals, want) in zip(ri, rows):
                assert M.accepted(f(g[r]), want), (cname, what, len(vals), g[r], want)
        rows_ok(A.reduce_vector(mon, out=gb.Vector.sparse(T, nr)), "row reduce")
        info, sr = new_semiring(gb, cname, f"GrB_FIRST_{t}"); assert info == 0, (cname, info)
        u = full_vec(gb, t, arr(t, [M.edge_values(t)[-1]] * width))
        for method in (None, "adaptive", "rowgroup", "push"):
            if method: monkeypatch.setenv("GRB_MI355X_SPMV", method)
            else: monkeypatch.delenv("GRB_MI355X_SPMV", raising=False)
            w = gb.Vector.sparse(T, nr); gb.base.check(gb.lib.GrB_mxv(w._h, None, None, sr, A._h, u._h, None), w)
            rows_ok(w, f"mxv {method} with FIRST")
        monkeypatch.delenv("GRB_MI355X_SPMV", raising=False)
        gb.lib.GrB_Semiring_free(C.byref(sr))
        return True
    for cname, op, _ in hs:
        if col(cname, one, cname, op):
            CHECKED.add(cname)
        monkeypatch.delenv("GRB_MI355X_SPMV", raising=False)
    col.done()


def test_every_exported_handle_is_checked_or_excluded(gb, gpu):
    """Runs last in the file: every unary / binary / monoid handle the header exports is in CHECKED (filled by the tests above) or in EXCLUDED."""
    exported = [c for kind in ("GrB_UnaryOp", "GrB_BinaryOp", "GrB_Monoid") for c in gb._capi.names[kind]]
    missing = [c for c in exported if c not in CHECKED and c not in EXCLUDED]
    stale = [c for c in EXCLUDED if c not in exported]
    print(f"\noperator table: {len(CHECKED)} handles checked, {len(EXCLUDED)} excluded, of {len(exported)} exported")
    for k in sorted(MAX_ERR):
        if MAX_ERR[k] > 0: print(f"  largest relative error of {k[0]} {k[1]} over the edge set: {MAX_ERR[k]:.3e}")
    assert not missing, f"handles neither checked nor excluded: {missing}"
    assert not stale, f"EXCLUDED names that are not exported: {stale}"
    assert all(r.startswith(("positional", "complex", "user-defined")) for r in EXCLUDED.values())
