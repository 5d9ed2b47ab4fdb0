"""Pins tests/matrix_model.py (the vectorised numpy model the GPU parity tests of the O(nnz) matrix kernels compare with) on the CPU:
  * against a plain dictionary transcription of the same rules — the `finish()` / `allows()` of tools/fuzz_companions.py typed again here, with explicit
    wrap-around — on random cases of at most 9 x 9 for INT64, INT8, UINT16 and FP32;
  * against the matrix cases of the reference's own companion vectors (tests/golden/reference_companion_vectors.json) that tests/companion_model.py replays.
No test here needs the library or a GPU."""
import random

import numpy as np
import pytest

import companion_model as CM
import matrix_model as MM

TYPES = ["INT64", "INT8", "UINT16", "FP32"]
CASES_PER_TYPE = 120          # 480 cases in all (the floor is 300)
BITS = {"INT64": 64, "INT8": 8, "UINT16": 16}


# ---- the dictionary transcription ----------------------------------------------------------------------------------------------------------------------
def wrap(typ, x):
    if typ == "FP32":
        return float(np.float32(x))                        # (1/8-grid operands: sums and products are exact; a quotient of two FP32 values rounds once)
    b = BITS[typ]; x = int(x) & ((1 << b) - 1)
    return x - (1 << b) if typ[0] == "I" and x >> (b - 1) else x


def tdiv(a, b):
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


BIN = {"PLUS": lambda a, b: a + b, "MIN": min, "MAX": max, "TIMES": lambda a, b: a * b, "FIRST": lambda a, b: a, "SECOND": lambda a, b: b,
       "MINUS": lambda a, b: a - b, "DIV": lambda a, b: a / b if isinstance(a, float) else tdiv(a, b)}
UN = {"AINV": lambda a: -a, "ABS": abs, "IDENTITY": lambda a: a, "ONE": lambda a: 1}
KEEP = {"TRIL": lambda i, j, x, k: j - i <= k, "TRIU": lambda i, j, x, k: j - i >= k, "DIAG": lambda i, j, x, k: j - i == k, "OFFDIAG": lambda i, j, x, k: j - i != k,
        "NONZERO": lambda i, j, x, k: x != 0, "EQ_ZERO": lambda i, j, x, k: x == 0, "GT_ZERO": lambda i, j, x, k: x > 0,
        "GT_THUNK": lambda i, j, x, k: x > k, "GE_THUNK": lambda i, j, x, k: x >= k, "LT_THUNK": lambda i, j, x, k: x < k, "LE_THUNK": lambda i, j, x, k: x <= k,
        "EQ_THUNK": lambda i, j, x, k: x == k, "NE_THUNK": lambda i, j, x, k: x != k}


def allows(mask, p, struct, comp):
    if mask is None:
        return not comp
    return (p in mask and (struct or bool(mask[p]))) != comp


def finish(typ, C, Tn, space, mask, struct, comp, replace, acc):
    Z = dict(Tn) if acc is None else dict(C)
    if acc is not None:
        for p, x in Tn.items():
            Z[p] = wrap(typ, BIN[acc](Z[p], x)) if p in Z else x
    out = {}
    for p in space:
        if allows(mask, p, struct, comp):
            if p in Z: out[p] = Z[p]
        elif not replace and p in C:
            out[p] = C[p]
    return out


def tr(d): return {(j, i): x for (i, j), x in d.items()}


# ---- moving between the two forms ------------------------------------------------------------------------------------------------------------------------
def to_mat(d, nr, nc, typ):
    ps = sorted(d)
    return MM.from_coo(nr, nc, [p[0] for p in ps], [p[1] for p in ps], np.array([d[p] for p in ps], MM.NP[typ]), typ)


def to_dict(m):
    assert np.all(np.diff(m.keys) > 0)
    return {(int(i), int(j)): (float(x) if m.vals.dtype.kind == "f" else bool(x) if m.vals.dtype.kind == "b" else int(x)) for i, j, x in zip(m.rows, m.cols, m.vals.tolist())}


def draw(rnd, typ):
    if typ == "FP32":
        return rnd.randint(-16, 16) / 8.0
    lo, hi = {"INT64": (-(1 << 63), (1 << 63) - 1), "INT8": (-128, 127), "UINT16": (0, 65535)}[typ]
    if rnd.random() < 0.25:                              # the type's extremes and their neighbours: PLUS / TIMES / MINUS wrap
        return rnd.choice([lo, lo + 1, hi, hi - 1, hi // 2 + 1])
    return rnd.randint(max(lo, -9), 9)


def rand_dict(rnd, nr, nc, dens, vals):
    return {(i, j): vals() for i in range(nr) for j in range(nc) if rnd.random() < dens}


@pytest.mark.parametrize("typ", TYPES)
def test_model_agrees_with_the_dictionary_transcription(typ):
    rnd = random.Random(TYPES.index(typ) + 11)
    kinds = {}
    for n in range(CASES_PER_TYPE):
        nr, nc = rnd.randint(1, 9), rnd.randint(1, 9)
        acc = rnd.choice([None, None, "PLUS", "MIN", "SECOND", "MINUS"])
        replace = rnd.random() < 0.3
        use_mask = rnd.random() < 0.6
        struct, comp = (rnd.random() < 0.4, rnd.random() < 0.4) if use_mask else (False, rnd.random() < 0.1)
        val = lambda: draw(rnd, typ)
        mtyp = rnd.choice(["BOOL", "INT8", "FP32"])
        mval = {"BOOL": lambda: rnd.random() < 0.7, "INT8": lambda: rnd.choice([0, 0, 1, -3]), "FP32": lambda: rnd.choice([0.0, -0.0, 1.5, float("nan")])}[mtyp]
        c = rand_dict(rnd, nr, nc, 0.4, val); m = rand_dict(rnd, nr, nc, 0.5, mval) if use_mask else None
        kind = rnd.choice(["ewise", "apply", "bind", "select", "transpose"]); kinds[kind] = kinds.get(kind, 0) + 1
        a = rand_dict(rnd, nr, nc, 0.5, val); A = to_mat(a, nr, nc, typ)
        what = (typ, n, kind, acc, replace, use_mask, struct, comp)
        if kind == "ewise":
            b = rand_dict(rnd, nr, nc, 0.5, val); op = rnd.choice(list(BIN)); union = rnd.random() < 0.5
            if op == "DIV":
                b = {p: (x if x != 0 else 3) for p, x in b.items()}
                if typ != "FP32": a = {p: max(x, -100) for p, x in a.items()}; A = to_mat(a, nr, nc, typ)      # (INT_MIN / -1 stays out)
            Tn = {p: (wrap(typ, BIN[op](a[p], b[p])) if p in a and p in b else (a[p] if p in a else b[p])) for p in (set(a) | set(b) if union else set(a) & set(b))}
            T = MM.ewise(op, typ, A, to_mat(b, nr, nc, typ), union); what += (op, union)
        elif kind == "apply":
            op = rnd.choice(list(UN)); Tn = {p: wrap(typ, UN[op](x)) for p, x in a.items()}; T = MM.apply(op, typ, A); what += (op,)
        elif kind == "bind":
            op = rnd.choice(["PLUS", "MINUS", "TIMES", "MIN"]); s = draw(rnd, typ); first = rnd.random() < 0.5
            Tn = {p: wrap(typ, BIN[op](s, x) if first else BIN[op](x, s)) for p, x in a.items()}
            T = MM.bind1st(op, typ, s, A) if first else MM.bind2nd(op, typ, A, s); what += (op, s, first)
        elif kind == "select":
            sel = rnd.choice(list(KEEP)); k = rnd.randint(-3, 3) if sel in ("TRIL", "TRIU", "DIAG", "OFFDIAG") else wrap(typ, rnd.choice([draw(rnd, typ), rnd.randint(0, 3)]))
            Tn = {p: x for p, x in a.items() if KEEP[sel](p[0], p[1], x, k)}; T = MM.select(sel, None if sel.endswith("ZERO") else k, A); what += (sel, k)
        else:
            at = rand_dict(rnd, nc, nr, 0.5, val); Tn = tr(at); T = MM.transpose(to_mat(at, nc, nr, typ))
        assert (T.nrows, T.ncols) == (nr, nc) and to_dict(T) == Tn, (what, to_dict(T), Tn)
        space = [(i, j) for i in range(nr) for j in range(nc)]
        exp = finish(typ, c, Tn, space, m, struct, comp, replace, acc)
        got = MM.write_back(to_mat(c, nr, nc, typ), T, None if m is None else to_mat(m, nr, nc, mtyp), struct, comp, replace, None if acc is None else (acc, typ))
        assert got.typ == typ and to_dict(got) == exp, (what, c, m, to_dict(got), exp)
    assert len(kinds) == 5


@pytest.mark.parametrize("typ", TYPES)
def test_row_reduction_agrees_with_the_dictionary_transcription(typ):
    rnd = random.Random(TYPES.index(typ) + 31)
    small = lambda: rnd.choice([1, 2, 3, 0 if typ == "UINT16" else -1])
    for n in range(40):
        nr, nc = rnd.randint(1, 9), rnd.randint(1, 9)
        for mon in ("PLUS", "MIN", "MAX", "TIMES"):
            # (FP32 products of 1/8-grid values leave the grid: TIMES folds small whole numbers there, and in every other case half of the time)
            a = rand_dict(rnd, nr, nc, 0.5, small if (n % 2 or (typ == "FP32" and mon == "TIMES")) else (lambda: draw(rnd, typ)))
            Tn = {}
            for (i, j), x in sorted(a.items()):
                Tn[(i, 0)] = wrap(typ, BIN[mon](Tn[(i, 0)], x)) if (i, 0) in Tn else x
            got = MM.reduce_rows(mon, typ, to_mat(a, nr, nc, typ))
            assert (got.nrows, got.ncols) == (nr, 1) and to_dict(got) == Tn, (typ, n, mon, a, to_dict(got), Tn)


def test_csr_export_of_the_model():
    m = MM.from_coo(4, 5, [3, 0, 0, 2], [4, 3, 1, 0], [7, 5, 6, 8], "INT8")
    rp, ci, x = MM.to_csr(m)
    assert rp.tolist() == [0, 2, 2, 3, 4] and ci.tolist() == [1, 3, 0, 4] and x.tolist() == [6, 5, 8, 7] and x.dtype == np.int8
    rp, ci, x = MM.to_csr(MM.transpose(m))
    assert rp.tolist() == [0, 1, 2, 2, 3, 4] and ci.tolist() == [2, 0, 0, 3] and x.tolist() == [8, 6, 5, 7]
    rp, ci, x = MM.to_csr(MM.empty(3, 2, "FP64"))
    assert rp.tolist() == [0, 0, 0, 0] and len(ci) == 0 and x.dtype == np.float64


def test_mask_truth_of_signed_zero_and_nan():
    """A stored -0.0 is false, a stored NaN is true; a structural mask asks only whether the entry is stored."""
    for typ in ("FP32", "FP64"):
        M = MM.from_coo(1, 5, [0] * 4, [0, 1, 2, 3], [0.0, -0.0, np.nan, 2.0], typ)
        keys = np.arange(5, dtype=np.int64)
        assert MM.mask_allows(M, False, False, keys).tolist() == [False, False, True, True, False]
        assert MM.mask_allows(M, False, True, keys).tolist() == [True, True, False, False, True]
        assert MM.mask_allows(M, True, False, keys).tolist() == [True, True, True, True, False]
    assert MM.mask_allows(None, False, False, np.arange(3)).all() and not MM.mask_allows(None, False, True, np.arange(3)).any()


def test_typecasts_and_operand_order():
    A = MM.from_coo(1, 3, [0, 0], [0, 1], [100, -7], "INT8"); B = MM.from_coo(1, 3, [0, 0], [0, 2], [100, 9], "INT8")
    T = MM.ewise("PLUS", "FP64", A, B, True)                                   # the operator's type is wider: no wrap inside it
    assert T.typ == "FP64" and T.vals.tolist() == [200.0, -7.0, 9.0]
    C = MM.from_coo(1, 3, [0], [0], [150], "INT16")
    got = MM.write_back(C, T, accum=("MIN", "INT32"))
    assert got.typ == "INT16" and got.vals.tolist() == [150, -7, 9]
    assert MM.ewise("MINUS", "INT8", A, B, False).vals.tolist() == [0] and MM.ewise("MINUS", "INT8", B, A, True).vals.tolist() == [0, -7, 9]
    assert MM.ewise("PLUS", "INT8", A, B, False).vals.tolist() == [-56]          # 200 wraps
    assert MM.bind1st("MINUS", "INT8", 1, A).vals.tolist() == [-99, 8] and MM.bind2nd("MINUS", "INT8", A, 1).vals.tolist() == [99, -8]
    U = MM.from_coo(1, 2, [0, 0], [0, 1], [5, 1 << 63], "UINT64")
    assert MM.select("GT_THUNK", (1 << 63) - 1, U).vals.tolist() == [1 << 63] and MM.select("LT_THUNK", (1 << 63) + 1, U).nvals == 2
    assert MM.binop("DIV", "INT64", np.array([-7, 7, -7, 7]), np.array([2, -2, -2, 2])).tolist() == [-3, -3, 3, 3]
    assert MM.binop("DIV", "INT8", np.array([-7, 7, -7, 7]), np.array([2, -2, -2, 2])).tolist() == [-3, -3, 3, 3]


# ---- the reference's own vectors ---------------------------------------------------------------------------------------------------------------------------
MATRIX_OPS = ("eadd", "emult", "apply", "apply_first", "apply_second", "select", "transpose", "reduce_vector")
GOLDEN = [c for c in CM.load() if c["kind"] == "matrix" and c["op"] in MATRIX_OPS]


def golden_operand(case, key):
    o = case[key]
    return MM.from_coo(o[3], o[4], o[0], o[1], np.array([CM.wrap(case["type"], x) for x in o[2]], MM.NP[case["type"]]), case["type"])


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{k:02d}-{c['op']}" for k, c in enumerate(GOLDEN)])
def test_model_reproduces_the_reference_vector(case):
    typ = case["type"]; A = golden_operand(case, "A"); op = case["op"]
    if op in ("eadd", "emult"):
        T = MM.ewise(case["binop"], typ, A, golden_operand(case, "B"), op == "eadd")
    elif op == "apply":
        T = MM.apply(case["unop"], case.get("unop_type", typ), A).cast(typ)
    elif op == "apply_first":
        T = MM.bind1st(case["binop"], typ, case["scalar"], A)
    elif op == "apply_second":
        T = MM.bind2nd(case["binop"], typ, A, case["scalar"])
    elif op == "select":
        T = MM.select(case["select"], case.get("thunk"), A)
    elif op == "transpose":
        T = A if "T0" in (case.get("desc") or "") else MM.transpose(A)
        assert [T.nrows, T.ncols] == case["expect_shape"]
    else:
        T = MM.reduce_rows(case["monoid"], typ, A)
    et = case.get("expect_type", typ)
    assert T.typ == et
    if op == "reduce_vector":
        got = sorted((int(i), CM.wrap(et, x)) for i, x in zip(T.rows, T.vals.tolist()))
    else:
        got = sorted(((int(i), int(j)), CM.wrap(et, x)) for i, j, x in zip(T.rows, T.cols, T.vals.tolist()))
    assert got == CM.expected(case), (case["cite"], got, CM.expected(case))


def test_the_golden_matrix_cases_are_all_there():
    assert {c["op"] for c in GOLDEN} == set(MATRIX_OPS) and len(GOLDEN) >= 30
