"""Pins tests/vector_model.py (the numpy model the GPU parity tests of the O(n) vector kernels compare with) on the CPU against a per-position dictionary
transcription of the same rules — {position: value}, folded and written back one position at a time with explicit wrap-around; the operator tables, `wrap`,
`allows` and `finish` are the ones tests/test_matrix_model.py pins the matrix model with — on random vectors of at most 40 positions for INT64, INT8, UINT16
and FP32.  No test here needs the library or a GPU."""
import math
import random

import numpy as np
import pytest

import vector_model as VM
from test_matrix_model import BIN, UN, allows, draw, finish, wrap

TYPES = ["INT64", "INT8", "UINT16", "FP32"]
CASES_PER_TYPE = 150          # 600 cases in all
KEEP = {"NONZERO": lambda x, k: x != 0, "EQ_ZERO": lambda x, k: x == 0, "GT_ZERO": lambda x, k: x > 0, "GE_ZERO": lambda x, k: x >= 0, "LT_ZERO": lambda x, k: x < 0,
        "LE_ZERO": lambda x, k: x <= 0, "NE_THUNK": lambda x, k: x != k, "EQ_THUNK": lambda x, k: x == k, "GT_THUNK": lambda x, k: x > k, "GE_THUNK": lambda x, k: x >= k,
        "LT_THUNK": lambda x, k: x < k, "LE_THUNK": lambda x, k: x <= k}


def to_vec(d, n, typ):
    val = np.zeros(n, VM.NP[typ]); pres = np.zeros(n, bool)
    for i, x in d.items():
        val[i] = x; pres[i] = True
    return VM.Vec(val, pres)


def to_dict(v):
    out = {}
    for i in np.flatnonzero(v.pres).tolist():
        x = v.val[i]
        out[i] = float(x) if v.val.dtype.kind == "f" else bool(x) if v.val.dtype.kind == "b" else int(x)
    return out


def same_dict(a, b):
    return a.keys() == b.keys() and all(a[i] == b[i] or (isinstance(a[i], float) and math.isnan(a[i]) and math.isnan(b[i])) for i in a)


def rand_dict(rnd, n, dens, vals):
    return {i: vals() for i in range(n) if rnd.random() < dens}


def cast_value(src, dst, x):
    """One value of type `src` as a value of type `dst`: integers wrap, an integer rounds into FP32, an FP32 value (small here) truncates toward zero."""
    if dst == "FP32": return float(np.float32(x))
    return wrap(dst, int(x))


@pytest.mark.parametrize("typ", TYPES)
def test_model_agrees_with_the_dictionary_transcription(typ):
    rnd = random.Random(TYPES.index(typ) + 51)
    kinds = {}
    for case in range(CASES_PER_TYPE):
        n = rnd.choice([1, 2, 3, 7, 16, 17, rnd.randint(1, 40)])
        acc = rnd.choice([None, None, "PLUS", "MIN", "SECOND", "MINUS"])
        replace = rnd.random() < 0.3
        use_mask = rnd.random() < 0.6
        struct, comp = (rnd.random() < 0.4, rnd.random() < 0.4) if use_mask else (False, rnd.random() < 0.15)
        val = lambda: draw(rnd, typ)
        mtyp = rnd.choice(["BOOL", "INT8", "FP32"])
        mval = {"BOOL": lambda: rnd.random() < 0.7, "INT8": lambda: rnd.choice([0, 0, 1, -3]), "FP32": lambda: rnd.choice([0.0, -0.0, 1.5, float("nan")])}[mtyp]
        w = rand_dict(rnd, n, 0.4, val); m = rand_dict(rnd, n, 0.5, mval) if use_mask else None
        kind = rnd.choice(["ewise", "apply", "bind", "select", "cast", "assign"]); kinds[kind] = kinds.get(kind, 0) + 1
        a = rand_dict(rnd, n, 0.5, val); A = to_vec(a, n, typ)
        W = to_vec(w, n, typ); M = None if m is None else to_vec(m, n, mtyp)
        what = (typ, case, kind, n, acc, replace, use_mask, struct, comp)
        space = list(range(n))
        if kind == "assign":
            s = draw(rnd, typ); index = rnd.choice([None, sorted(rnd.sample(range(n), rnd.randint(0, n)))])
            region = set(space if index is None else index)
            z = dict(w)                                                           # Z: accum(w, s) inside the index list, w outside it
            for p in region:
                z[p] = wrap(typ, BIN[acc](w[p], s)) if (acc is not None and p in w) else s
            exp = finish(typ, w, z, space, m, struct, comp, replace, None)
            got = VM.assign_scalar(W, s, index, M, struct, comp, replace, None if acc is None else (acc, typ))
            assert got.typ == typ and same_dict(to_dict(got), exp), (what, s, index, w, m, to_dict(got), exp)
            continue
        if kind == "ewise":
            b = rand_dict(rnd, n, 0.5, val); op = rnd.choice(list(BIN)); union = rnd.random() < 0.5
            if op == "DIV":
                b = {p: (x if x != 0 else 3) for p, x in b.items()}
                if typ != "FP32": a = {p: max(x, -100) for p, x in a.items()}; A = to_vec(a, n, typ)      # (INT_MIN / -1 stays out)
            Tn = {p: (wrap(typ, BIN[op](a[p], b[p])) if p in a and p in b else (a[p] if p in a else b[p])) for p in (set(a) | set(b) if union else set(a) & set(b))}
            T = VM.ewise(op, typ, A, to_vec(b, n, typ), union); what += (op, union)
        elif kind == "apply":
            op = rnd.choice(list(UN)); Tn = {p: wrap(typ, UN[op](x)) for p, x in a.items()}; T = VM.apply(op, typ, A); what += (op,)
        elif kind == "bind":
            op = rnd.choice(["PLUS", "MINUS", "TIMES", "MIN"]); s = draw(rnd, typ); first = rnd.random() < 0.5
            Tn = {p: wrap(typ, BIN[op](s, x) if first else BIN[op](x, s)) for p, x in a.items()}
            T = VM.bind1st(op, typ, s, A) if first else VM.bind2nd(op, typ, A, s); what += (op, s, first)
        elif kind == "select":
            sel = rnd.choice(list(KEEP)); k = wrap(typ, rnd.choice([draw(rnd, typ), rnd.randint(0, 3)]))
            Tn = {p: x for p, x in a.items() if KEEP[sel](x, k)}; T = VM.select(sel, None if sel.endswith("ZERO") else k, A); what += (sel, k)
        else:
            src = rnd.choice(TYPES)
            a = rand_dict(rnd, n, 0.5, lambda: draw(rnd, src)); Tn = {p: cast_value(src, typ, x) for p, x in a.items()}
            T = VM.cast(to_vec(a, n, src), typ); what += (src,)
        assert T.n == n and T.typ == typ and same_dict(to_dict(T), Tn), (what, to_dict(T), Tn)
        exp = finish(typ, w, Tn, space, m, struct, comp, replace, acc)
        got = VM.write_back(W, T, M, struct, comp, replace, None if acc is None else (acc, typ))
        assert got.typ == typ and same_dict(to_dict(got), exp), (what, w, m, to_dict(got), exp)
    assert len(kinds) == 6


def fold(typ, mon, xs):
    """The present values folded in index order, one at a time."""
    if not xs:
        return {"PLUS": 0, "TIMES": 1, "MIN": math.inf if typ == "FP32" else int(np.iinfo(VM.NP[typ]).max), "MAX": -math.inf if typ == "FP32" else int(np.iinfo(VM.NP[typ]).min)}[mon]
    acc = xs[0]
    for x in xs[1:]:
        if typ == "FP32" and mon in ("MIN", "MAX"):                               # fmin / fmax: a NaN operand is omitted
            acc = x if math.isnan(acc) else acc if math.isnan(x) else BIN[mon](acc, x)
        else:
            acc = wrap(typ, BIN[mon](acc, x))
    return acc


@pytest.mark.parametrize("typ", TYPES)
def test_reduction_agrees_with_the_dictionary_transcription(typ):
    rnd = random.Random(TYPES.index(typ) + 71)
    small = lambda: rnd.choice([1, 2, 3, 0 if typ == "UINT16" else -1])
    nan_or = lambda: rnd.choice([float("nan"), float("nan"), draw(rnd, typ)])
    for case in range(60):
        n = rnd.choice([0, 1, 2, 5, 33, 40])
        for mon in ("PLUS", "MIN", "MAX", "TIMES"):
            vals = small if (case % 2 or (typ == "FP32" and mon == "TIMES")) else (lambda: draw(rnd, typ))
            if typ == "FP32" and mon in ("MIN", "MAX") and case % 3 == 0: vals = nan_or
            a = rand_dict(rnd, n, rnd.choice([0.0, 0.1, 0.5, 1.0]), vals)
            exp = fold(typ, mon, [a[i] for i in sorted(a)])
            got = VM.reduce(mon, typ, to_vec(a, n, typ))
            assert got.dtype == VM.NP[typ] and (got == exp or (math.isnan(exp) and np.isnan(got))), (typ, case, mon, a, got, exp)


def test_reduction_rules_for_nan_empty_bool_and_bitwise():
    nan = float("nan")
    for typ in ("FP32", "FP64"):
        assert np.isnan(VM.reduce("MIN", typ, to_vec({0: nan, 3: nan}, 5, typ))) and np.isnan(VM.reduce("MAX", typ, to_vec({0: nan}, 5, typ)))
        assert VM.reduce("MIN", typ, to_vec({0: nan, 3: nan, 4: 2.5}, 5, typ)) == 2.5 and VM.reduce("MAX", typ, to_vec({0: -1.0, 1: nan}, 5, typ)) == -1.0
        assert VM.reduce("MIN", typ, VM.empty(5, typ)) == np.inf and VM.reduce("MAX", typ, VM.empty(5, typ)) == -np.inf
        assert VM.reduce("PLUS", typ, VM.empty(0, typ)) == 0 and VM.reduce("TIMES", typ, VM.empty(3, typ)) == 1
    assert VM.reduce("MIN", "INT8", VM.empty(2, "INT8")) == 127 and VM.reduce("MAX", "UINT16", VM.empty(2, "UINT16")) == 0
    assert VM.reduce("PLUS", "INT8", to_vec({0: 100, 1: 100}, 2, "INT8")) == -56 and VM.reduce("TIMES", "UINT16", to_vec({0: 256, 1: 257}, 2, "UINT16")) == 256
    assert VM.reduce("PLUS", "FP64", to_vec({0: 100, 1: 100}, 2, "INT8")) == 200.0          # the values are cast into the monoid's type first
    t, f = True, False
    for d in ({}, {0: t}, {0: f}, {0: t, 1: f}, {0: f, 1: f}, {0: f, 1: t, 2: f, 3: f}):
        xs = [d[i] for i in sorted(d)]; v = to_vec(d, 4, "BOOL")
        acc = xs[0] if xs else True
        for x in xs[1:]: acc = acc == x
        assert VM.reduce("LOR", "BOOL", v) == any(xs) and VM.reduce("LAND", "BOOL", v) == all(xs) and VM.reduce("LXOR", "BOOL", v) == (sum(xs) % 2 == 1)
        assert VM.reduce("EQ", "BOOL", v) == acc and VM.reduce("LXNOR", "BOOL", v) == acc
        assert VM.reduce("PLUS", "BOOL", v) == any(xs) and VM.reduce("TIMES", "BOOL", v) == all(xs)
    u = to_vec({0: 0x0F0F, 2: 0x00FF, 3: 0x8001}, 4, "UINT16")
    assert VM.reduce("BOR", "UINT16", u) == 0x8FFF and VM.reduce("BAND", "UINT16", u) == 0x0001 and VM.reduce("BXOR", "UINT16", u) == (0x0F0F ^ 0x00FF ^ 0x8001)
    assert VM.reduce("BXNOR", "UINT16", u) == (~(~(0x0F0F ^ 0x00FF) ^ 0x8001)) & 0xFFFF and VM.reduce("BAND", "UINT16", VM.empty(3, "UINT16")) == 0xFFFF


def test_iseq_rules():
    for typ in ("FP32", "FP64"):
        a = to_vec({0: 0.0, 2: 1.5}, 4, typ)
        assert VM.iseq(a, to_vec({0: -0.0, 2: 1.5}, 4, typ)) and VM.iseq(a, a.copy())
        assert not VM.iseq(a, to_vec({0: 0.0, 3: 1.5}, 4, typ))                   # the same count, one entry moved
        assert not VM.iseq(a, to_vec({0: 0.0, 2: 1.25}, 4, typ)) and not VM.iseq(a, to_vec({0: 0.0}, 4, typ)) and not VM.iseq(a, to_vec({0: 0.0, 2: 1.5}, 5, typ))
        nanv = to_vec({1: float("nan")}, 4, typ)
        assert not VM.iseq(nanv, nanv.copy())
    a = to_vec({1: 7}, 3, "INT8"); b = a.copy(); b.val[0] = 99                     # the value of a position without an entry is not looked at
    assert VM.iseq(a, b) and not VM.iseq(a, VM.cast(a, "INT16")) and VM.iseq(VM.empty(0, "INT8"), VM.empty(0, "INT8"))


def test_mask_rules_and_scalar_assign():
    w = to_vec({0: 1, 1: 2, 2: 3, 3: 4}, 6, "INT8"); T = to_vec({0: 10, 4: 50}, 6, "INT8")
    assert to_dict(VM.write_back(w, T, None, comp=True)) == to_dict(w)            # no mask, complemented: nothing is written ...
    assert to_dict(VM.write_back(w, T, None, comp=True, replace=True)) == {}      # ... and replace deletes what may not be written
    M = to_vec({0: 0.0, 1: -0.0, 2: float("nan"), 4: 2.0}, 6, "FP32")
    assert VM.mask_allows(M, False, False, 6).tolist() == [False, False, True, False, True, False]
    assert VM.mask_allows(M, True, False, 6).tolist() == [True, True, True, False, True, False]
    assert VM.mask_allows(M, False, True, 6).tolist() == [True, True, False, True, False, True]
    assert to_dict(VM.write_back(w, T, M)) == {0: 1, 1: 2, 3: 4, 4: 50}             # position 2 is allowed and T has nothing there
    assert to_dict(VM.write_back(w, T, M, replace=True)) == {4: 50}
    assert to_dict(VM.write_back(w, T, M, accum=("PLUS", "INT8"))) == {0: 1, 1: 2, 2: 3, 3: 4, 4: 50}
    assert to_dict(VM.assign_scalar(w, 9)) == {i: 9 for i in range(6)}
    assert to_dict(VM.assign_scalar(w, 9, index=[0, 5])) == {0: 9, 1: 2, 2: 3, 3: 4, 5: 9}
    assert to_dict(VM.assign_scalar(w, 9, index=[0, 5], accum=("PLUS", "INT8"))) == {0: 10, 1: 2, 2: 3, 3: 4, 5: 9}
    assert to_dict(VM.assign_scalar(w, 9, mask=M)) == {0: 1, 1: 2, 2: 9, 3: 4, 4: 9}
    assert to_dict(VM.assign_scalar(w, 9, mask=M, replace=True)) == {2: 9, 4: 9}
    assert to_dict(VM.assign_scalar(w, 9, index=[2], mask=M, struct=True, replace=True)) == {0: 1, 1: 2, 2: 9}      # allowed and outside the list: kept
    assert to_dict(VM.assign_scalar(w, 100, mask=M, comp=True, accum=("PLUS", "INT8"))) == {0: 101, 1: 102, 2: 3, 3: 104, 5: 100}
