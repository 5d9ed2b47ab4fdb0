"""A numpy model of the bitmap-vector operations (test infrastructure), independent of the library: a vector is `(val, pres)`, one value and one presence
flag per position, and every operation is an element-wise numpy expression over all n positions, so ten million positions cost a few array passes.  The value
of a position without an entry means nothing: comparisons look at `val[pres]` only.

Operators, typecasts and the truth of a mask value are those of tests/matrix_model.py (`binop`, `unop`, `cast`, `mask_truth`, and `select` for the value
selects); this file adds only what is about positions:
  * eWiseAdd / eWiseMult, apply (unary, bound first or second scalar), value select, typecast;
  * scalar assign over all positions, over an index list, under a mask;
  * the write-back `w<M, replace> = accum(w, T)` (C API 1.3 section 3.5.4): a valued, structural or complemented mask; no mask with complement allows nothing;
  * reduction to a scalar: the monoid folded over the present values in its own type; floating-point MIN / MAX start from the first value (a NaN is omitted
    unless every value is NaN), an empty vector gives the monoid's identity;
  * `iseq`: the same pattern and == values (NaN differs from NaN, -0.0 equals 0.0).

tests/test_vector_model.py pins it to a per-position dictionary transcription of the same rules; tests/test_vector_kernels_at_size_gpu.py compares the HIP
kernels with it at sizes past one round of their grids."""
import numpy as np

import matrix_model as MM

NP = MM.NP


class Vec:
    def __init__(self, val, pres):
        self.val = np.asarray(val); self.pres = np.asarray(pres, bool)
        assert self.val.ndim == 1 and self.val.shape == self.pres.shape and self.val.dtype in MM.NAME

    @property
    def typ(self): return MM.NAME[self.val.dtype]
    @property
    def n(self): return len(self.val)
    @property
    def nvals(self): return int(self.pres.sum())

    def copy(self): return Vec(self.val.copy(), self.pres.copy())


def empty(n, typ):
    return Vec(np.zeros(n, NP[typ]), np.zeros(n, bool))


def cast(u, typ):
    return Vec(MM.cast(u.val, typ), u.pres)


# ---- operations: each returns T, the result before the write-back -----------------------------------------------------------------------------------------
def ewise(op, typ, u, v, union):
    """Where both have an entry op(u, v), in that order, in the operator's type; in a union an entry of one operand alone passes through, cast to that type."""
    assert u.n == v.n
    both = u.pres & v.pres
    second = np.where(both, v.val, np.ones(1, v.val.dtype)) if op == "DIV" else v.val      # (no divisor is looked at where it does not count)
    z = MM.binop(op, typ, u.val, second)
    val = np.where(both, z, np.where(u.pres, MM.cast(u.val, typ), MM.cast(v.val, typ)))
    return Vec(val, (u.pres | v.pres) if union else both)


def apply(op, typ, u):
    return Vec(MM.unop(op, typ, u.val), u.pres)


def bind1st(op, typ, scalar, u):
    """op(scalar, u(i))."""
    return Vec(MM.binop(op, typ, np.full(u.n, scalar, NP[typ]), u.val), u.pres)


def bind2nd(op, typ, u, scalar):
    """op(u(i), scalar)."""
    return Vec(MM.binop(op, typ, u.val, np.full(u.n, scalar, NP[typ])), u.pres)


def select(sel, thunk, u):
    """The entries a value select keeps (matrix_model.select on the n x 1 column)."""
    at = np.flatnonzero(u.pres)
    kept = MM.select(sel, thunk, MM.Mat(u.n, 1, at, u.val[at]))
    pres = np.zeros(u.n, bool); pres[kept.keys] = True
    return Vec(u.val, pres)


# ---- the write-back ------------------------------------------------------------------------------------------------------------------------------------------
def mask_allows(mask, struct, comp, n):
    """For each position: does the mask (None: no mask) let it be written?"""
    if mask is None:
        return np.full(n, not comp)
    assert mask.n == n
    truth = mask.pres if struct else mask.pres & MM.mask_truth(mask.val)
    return truth != comp


def write_back(w, T, mask=None, struct=False, comp=False, replace=False, accum=None):
    """w<M, replace> = accum(w, T): Z = T, or accum(w, T) on the union of the two patterns in the accumulator's type (`accum` = (operator, type) or None);
    Z is cast to w's type; where the mask allows, w takes Z's entry or loses its own; where it does not, w keeps its entry unless `replace` deletes it."""
    assert w.n == T.n
    Z = T if accum is None else ewise(accum[0], accum[1], w, T, True)
    Z = cast(Z, w.typ)
    allow = mask_allows(mask, struct, comp, w.n)
    pres = np.where(allow, Z.pres, w.pres & (not replace))
    return Vec(np.where(allow & Z.pres, Z.val, w.val), pres)


def assign_scalar(w, scalar, index=None, mask=None, struct=False, comp=False, replace=False, accum=None):
    """w<M, replace>(I) = accum(w(I), scalar), I every position (None) or an index list: inside I, Z holds accum(w, scalar) where w has an entry and the scalar
    where it has none; outside I, Z is w.  Then the write-back of Z over ALL positions (GrB_assign, not GxB_subassign)."""
    region = np.ones(w.n, bool)
    if index is not None:
        region = np.zeros(w.n, bool); region[np.asarray(index, np.int64)] = True
    atyp = w.typ if accum is None else accum[1]
    s = np.full(w.n, scalar, NP[atyp])
    inside = s if accum is None else np.where(w.pres, MM.binop(accum[0], atyp, w.val, s), s)
    Z = Vec(np.where(region, MM.cast(inside, w.typ), w.val), w.pres | region)
    return write_back(w, Z, mask, struct, comp, replace, None)


# ---- to a scalar ----------------------------------------------------------------------------------------------------------------------------------------------
_FOLD = {"PLUS": np.add, "TIMES": np.multiply, "MIN": np.minimum, "MAX": np.maximum, "LOR": np.logical_or, "LAND": np.logical_and, "LXOR": np.logical_xor,
         "BOR": np.bitwise_or, "BAND": np.bitwise_and, "BXOR": np.bitwise_xor}
_FOLD_FP = {"MIN": np.fmin, "MAX": np.fmax}


def identity(monoid, typ):
    t = NP[typ]
    if typ == "BOOL":
        return np.bool_(MM.BOOL_RENAME.get(monoid, monoid) in ("LAND", "EQ", "LXNOR"))
    if monoid in ("PLUS", "BOR", "BXOR"): return t(0)
    if monoid == "TIMES": return t(1)
    if monoid in ("BAND", "BXNOR"): return t(np.iinfo(t).max)
    lo, hi = (-np.inf, np.inf) if typ.startswith("FP") else (np.iinfo(t).min, np.iinfo(t).max)
    return t(hi if monoid == "MIN" else lo)


def reduce(monoid, typ, u):
    """The monoid of type `typ` folded over the present values, cast into that type first.  Integer PLUS and TIMES wrap (in any order); floating-point MIN and
    MAX are fmin / fmax from the first value on: NaN only when every value is NaN; no entry at all gives the identity."""
    x = MM.cast(u.val[u.pres], typ)
    if not len(x):
        return identity(monoid, typ)
    if typ == "BOOL":
        monoid = MM.BOOL_RENAME.get(monoid, monoid)
    with np.errstate(all="ignore"):
        if monoid == "BXNOR":                                  # (x xnor y = ~(x ^ y): an even number of complements cancels)
            r = np.bitwise_xor.reduce(x); return NP[typ](r if len(x) % 2 else ~r)
        if monoid in ("EQ", "LXNOR"):                          # (true iff an even number of the values is false)
            return np.bool_(np.count_nonzero(~x) % 2 == 0)
        uf = _FOLD_FP.get(monoid, _FOLD[monoid]) if typ.startswith("FP") else _FOLD[monoid]
        return NP[typ](uf.reduce(x, dtype=x.dtype))


def iseq(u, v):
    """Same size, type and pattern, and == values where present: NaN differs from NaN, -0.0 equals 0.0."""
    if u.n != v.n or u.typ != v.typ or not np.array_equal(u.pres, v.pres):
        return False
    with np.errstate(invalid="ignore"):
        return bool(np.all(u.val[u.pres] == v.val[v.pres]))
