"""tests/union_model.py against (a) a dictionary transcription of the three-case rule of GxB_eWiseUnion on hand-written 4 x 4 cases, (b) the identity "the union
with fill values is eWiseAdd of the two operands padded with beta / alpha at the other's-only positions" on random patterns, and (c) "union(PLUS, 0, 0) is
eWiseAdd(PLUS)" for integer types.  No device, no library."""
import numpy as np
import pytest

import matrix_model as MM
import vector_model as VM
import union_model as UM

NP = MM.NP

PY = {"MINUS": lambda x, y: x - y, "DIV": lambda x, y: x / y, "FIRST": lambda x, y: x, "SECOND": lambda x, y: y, "ISGT": lambda x, y: float(x > y),
      "PLUS": lambda x, y: x + y}


def rule(op, a, alpha, b, beta):
    """The three cases, entry by entry, over dictionaries {position: value} of Python floats."""
    out = {}
    for k in sorted(set(a) | set(b)):
        if k in a and k in b: out[k] = PY[op](a[k], b[k])
        elif k in a: out[k] = PY[op](a[k], beta)
        else: out[k] = PY[op](alpha, b[k])
    return out


# hand-written 4 x 4 cases: {(i, j): value}; values on the 1/8 grid, no zero divisors
A4 = {(0, 0): 1.5, (0, 3): -2.0, (1, 1): 4.0, (2, 0): 0.25, (3, 3): 8.0}
B4 = {(0, 0): 0.5, (1, 1): -4.0, (1, 2): 2.0, (3, 0): 1.0, (3, 3): 8.0}
CASES = [("independent", A4, B4), ("same pattern", A4, {k: v + 1.0 for k, v in A4.items()}), ("disjoint", A4, {(0, 1): 3.0, (2, 2): -1.0}),
         ("B empty", A4, {}), ("A empty", {}, B4), ("both empty", {}, {})]


def mat_of(d, typ="FP64"):
    ks = sorted(d)
    return MM.from_coo(4, 4, [i for i, _ in ks], [j for _, j in ks], [d[k] for k in ks], typ) if ks else MM.empty(4, 4, typ)


def vec_of(d, typ="FP64"):
    val = np.zeros(16, NP[typ]); pres = np.zeros(16, bool)
    for (i, j), x in d.items(): val[4 * i + j] = x; pres[4 * i + j] = True
    return VM.Vec(val, pres)


@pytest.mark.parametrize("op", sorted(PY))
@pytest.mark.parametrize("label,a,b", CASES)
def test_the_three_case_rule_on_4_by_4(op, label, a, b):
    alpha, beta = 0.5, -2.0
    exp = rule(op, a, alpha, b, beta)
    T = UM.union(op, "FP64", mat_of(a), alpha, mat_of(b), beta)
    assert {(int(k) // 4, int(k) % 4): float(x) for k, x in zip(T.keys, T.vals)} == exp, (op, label)
    V = UM.union(op, "FP64", vec_of(a), alpha, vec_of(b), beta)
    assert {(int(k) // 4, int(k) % 4): float(V.val[k]) for k in np.flatnonzero(V.pres)} == exp, (op, label)


def test_the_side_and_the_order_are_both_right():
    """MINUS with alpha != beta at one A-only, one B-only and one shared position, written out."""
    T = UM.union("MINUS", "INT32", mat_of({(0, 0): 10, (1, 1): 20}, "INT32"), 7, mat_of({(1, 1): 1, (2, 2): 2}, "INT32"), 3)
    assert T.keys.tolist() == [0, 5, 10] and T.vals.tolist() == [10 - 3, 20 - 1, 7 - 2] and T.vals.dtype == np.int32


def test_scalars_and_operands_are_cast_into_the_operators_type():
    """FP64 2.75 into an INT32 operator acts as 2; FP64 operands are truncated the same way; INT8 wraps."""
    T = UM.union("MINUS", "INT32", mat_of({(0, 0): 5.75}), 2.75, mat_of({(3, 3): 1.5}), 0.5)
    assert T.vals.tolist() == [5 - 0, 2 - 1] and T.typ == "INT32"
    W = UM.union("MINUS", "INT8", mat_of({(0, 0): -128}, "INT8"), 0, mat_of({(1, 1): -128}, "INT8"), 1)
    assert W.vals.tolist() == [127, -128]
    F = UM.union(lambda x, y: x - 2 * y, "FP64", mat_of({(0, 0): 1.0}), 0.5, mat_of({(1, 1): 3.0}), -2.0)
    assert F.vals.tolist() == [1.0 + 4.0, 0.5 - 6.0]


def random_pair(rng, typ, nr, nc, density):
    n = nr * nc
    ka = np.flatnonzero(rng.random(n) < density); kb = np.flatnonzero(rng.random(n) < density)
    draw = lambda k: (rng.integers(1, 7, len(k)) * rng.choice([-1, 1], len(k)) if typ[0] != "U" and typ != "BOOL" else rng.integers(1, 7, len(k))).astype(NP[typ])
    return MM.Mat(nr, nc, ka, draw(ka)), MM.Mat(nr, nc, kb, draw(kb))


def as_vec(m):
    val = np.zeros(m.nrows * m.ncols, m.vals.dtype); pres = np.zeros(len(val), bool); val[m.keys] = m.vals; pres[m.keys] = True
    return VM.Vec(val, pres)


@pytest.mark.parametrize("typ", ["INT8", "UINT16", "INT32", "FP32", "INT64", "FP64"])
@pytest.mark.parametrize("op", ["MINUS", "DIV", "FIRST", "SECOND", "ISGT", "PLUS"])
def test_union_is_ewise_add_of_padded_operands(typ, op):
    """Pad A with alpha where only B holds an entry and B with beta where only A does: both then hold every entry of the union, and eWiseAdd calls the
    operator everywhere.  Non-zero values and scalars, so DIV never meets a zero."""
    rng = np.random.default_rng(sum(map(ord, typ + op)))
    alpha, beta = (7, 3) if "INT" in typ else (0.5, -2.0)
    for density in (0.0, 0.05, 0.5, 1.0):
        A, B = random_pair(rng, typ, 23, 17, density)
        keys = np.union1d(A.keys, B.keys)
        pad = lambda m, s: MM.Mat(m.nrows, m.ncols, keys, np.where(np.isin(keys, m.keys), np.zeros(len(keys), NP[typ]), NP[typ](s)))
        Ap, Bp = pad(A, alpha), pad(B, beta)
        Ap.vals[np.isin(keys, A.keys)] = A.vals; Bp.vals[np.isin(keys, B.keys)] = B.vals
        exp = MM.ewise(op, typ, Ap, Bp, True)
        T = UM.union(op, typ, A, alpha, B, beta)
        assert np.array_equal(T.keys, exp.keys) and T.vals.dtype == exp.vals.dtype and np.array_equal(T.vals, exp.vals), (typ, op, density)
        V = UM.union(op, typ, as_vec(A), alpha, as_vec(B), beta); Ve = VM.ewise(op, typ, as_vec(Ap), as_vec(Bp), True)
        assert np.array_equal(V.pres, Ve.pres) and np.array_equal(V.val[V.pres], Ve.val[Ve.pres]), (typ, op, density)


@pytest.mark.parametrize("typ", ["INT8", "UINT16", "INT32", "INT64", "UINT64"])
def test_plus_with_zero_fills_is_ewise_add(typ):
    rng = np.random.default_rng(11)
    A, B = random_pair(rng, typ, 31, 29, 0.3)
    lim = np.iinfo(NP[typ]); A.vals[::7] = lim.max; B.vals[::5] = lim.max; A.vals[1::9] = lim.min            # (the sums wrap)
    T = UM.union("PLUS", typ, A, 0, B, 0); exp = MM.ewise("PLUS", typ, A, B, True)
    assert np.array_equal(T.keys, exp.keys) and np.array_equal(T.vals, exp.vals)
    V = UM.union("PLUS", typ, as_vec(A), 0, as_vec(B), 0); Ve = VM.ewise("PLUS", typ, as_vec(A), as_vec(B), True)
    assert np.array_equal(V.pres, Ve.pres) and np.array_equal(V.val[V.pres], Ve.val[Ve.pres])
