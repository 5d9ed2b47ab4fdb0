"""Comparison semirings on the device (pygraphblas_amd/csrc/grb_cmpsr.hip): GxB_{LOR,LAND,LXOR,EQ,ANY}_{EQ..LE}_<T> in mxv, vxm and mxm.

The model is tests/operator_model.py: both operands go into the semiring's type with M.cast, every term is M.binop(cmp, T, a, b) — mxv and mxm a = A(i,k),
b = B(k,j); vxm a = u(k), b = A(k,j) — and the monoid is a plain Python fold over the terms of a position (EQ: left to right with ==).  A position without a
term has no entry.  For ANY the value of any one term of the position is accepted.  Everything is BOOL: every comparison is bit-exact, there is no tolerance.
The oracle is not used: it keeps a comparison's 0 / 1 in the semiring's type.

Shapes: edge values, one and two entries per row over every ordered pair of M.edge_values(T); the rows kernel on 20 000 rows (a second round of the grid-stride
loop past 16 384 waves) with row lengths 0, 1, 63, 64, 65, 128, 129 and 4 097 (the lane stride, the early exits); the product kernel on rows of T of 1, 128, 129
and 600 entries (accumulators in LDS and in global memory), with and without a mask."""
import ctypes as C
import itertools
import zlib

import numpy as np
import pytest

import operator_model as M
from test_userop_gpu import VARIANTS, descriptor

pytestmark = pytest.mark.gpu

ADDS = ["LOR", "LAND", "LXOR", "EQ", "ANY"]
CMPS = ["EQ", "NE", "GT", "LT", "GE", "LE"]


# ---- the model --------------------------------------------------------------------------------------------------------------------------------------------------
def fold(add, terms):
    """The monoid over a non-empty list of bools; for ANY the set of accepted values."""
    assert terms
    if add == "LOR":
        return any(terms)
    if add == "LAND":
        return all(terms)
    if add == "LXOR":
        return sum(terms) % 2 == 1
    if add == "EQ":
        acc = terms[0]
        for x in terms[1:]:
            acc = acc == x
        return acc
    return set(terms)


def term(cmp_, t, a, b):
    (r,) = M.binop(cmp_, t, a, b)
    return r


def product_terms(cmp_, t, Ad, Bd):
    """{(i, j): [terms in ascending k]} of A (+).cmp B over dicts {(i, k): value}, {(k, j): value} of values already in type t: cmp(A(i,k), B(k,j))."""
    brows = {}
    for (k, j), b in sorted(Bd.items()):
        brows.setdefault(k, []).append((j, b))
    out = {}
    for (i, k), a in sorted(Ad.items()):
        for j, b in brows.get(k, ()):
            out.setdefault((i, j), []).append(term(cmp_, t, a, b))
    return out


def check_against(add, got, terms, what):
    """got: {position: bool}; terms: {position: [bool]}."""
    assert set(got) == set(terms), (what, "pattern", sorted(set(got) ^ set(terms))[:8])
    for p, ts in terms.items():
        want = fold(add, ts)
        if add == "ANY":
            assert got[p] in want, (what, p, got[p], ts[:8])
        else:
            assert got[p] == want, (what, p, got[p], want, ts[:8])


def vec_dict(w):
    idx, x = w.to_arrays()
    return {int(i): bool(v) for i, v in zip(idx, x)}


def mat_dict(Cm):
    i, j, x = Cm.to_arrays()
    return {(int(a), int(b)): bool(v) for a, b, v in zip(i, j, x)}


def np_values(t, vals):
    return np.array(vals, dtype=M.NP[t])


def matrix_of(gb, t, d, nr, nc):
    keys = sorted(d)
    i = np.array([k[0] for k in keys], np.uint64)
    j = np.array([k[1] for k in keys], np.uint64)
    return gb.Matrix.from_arrays(i, j, np_values(t, [d[k] for k in keys]), nr, nc, getattr(gb, t))


def vector_of(gb, t, d, n):
    keys = sorted(d)
    return gb.Vector.from_arrays(np.array(keys, np.uint64), np_values(t, [d[k] for k in keys]), n, getattr(gb, t))


def cast_dict(src, t, d):
    return {k: M.cast(src, t, v) for k, v in d.items()}


def last_error(gb):
    buf = C.create_string_buffer(1024)
    gb.lib.GrBX_last_error(buf, C.c_int(1024))
    return buf.value.decode()


# ---- edge values ------------------------------------------------------------------------------------------------------------------------------------------------
def edge_operands(src, entries):
    """Row r = (a, b) of A (n^2 x n) holds E[a] in column b — and, with two entries per row, E[a + 1] in column b + 1 (both mod n); u = E, full; B (n x 2) holds E in
    column 0 and E rotated by three in column 1.  Every ordered pair of edge values is a term of its own row."""
    E = M.edge_values(src)
    n = len(E)
    Ad = {}
    for a in range(n):
        for b in range(n):
            Ad[(a * n + b, b)] = E[a]
            if entries == 2:
                Ad[(a * n + b, (b + 1) % n)] = E[(a + 1) % n]
    ud = {k: E[k] for k in range(n)}
    Bd = {(k, 0): E[k] for k in range(n)}
    Bd.update({(k, 1): E[(k + 3) % n] for k in range(n)})
    return E, n, Ad, ud, Bd


def run_edge_case(gb, t, src):
    T = getattr(gb, t)
    seen_order = False
    for entries in (1, 2):
        E, n, Ad, ud, Bd = edge_operands(src, entries)
        At = {(k, r): v for (r, k), v in Ad.items()}
        A, Atm, u, B = matrix_of(gb, src, Ad, n * n, n), matrix_of(gb, src, At, n, n * n), vector_of(gb, src, ud, n), matrix_of(gb, src, Bd, n, 2)
        Ac, Atc, uc, Bc = cast_dict(src, t, Ad), cast_dict(src, t, At), cast_dict(src, t, ud), cast_dict(src, t, Bd)
        ucol, urow = {(k, 0): v for k, v in uc.items()}, {(0, k): v for k, v in uc.items()}
        for cmp_ in CMPS:
            mxv_terms = {p[0]: ts for p, ts in product_terms(cmp_, t, Ac, ucol).items()}
            vxm_terms = {p[1]: ts for p, ts in product_terms(cmp_, t, urow, Atc).items()}          # cmp(u(k), A(k,j))
            mxm_terms = product_terms(cmp_, t, Ac, Bc)
            if cmp_ in ("GT", "LE") and entries == 1:
                # the argument order shows: on unequal operands the two orders disagree, so a vxm that compared (A(k,j), u(k)) would fail below
                differ = [r for r in mxv_terms if mxv_terms[r] != vxm_terms[r]]
                assert len(differ) >= n, (t, cmp_)
                seen_order = True
            for add in ADDS:
                sr = getattr(T, f"{add}_{cmp_}")
                w = A.mxv(u, sr)
                assert w.type is gb.BOOL
                plan = gb.last_kernel_plan()
                assert plan.startswith(f"cmpsr<add={add},mul={cmp_},type={t},kind=mxv> ") and "k_cmpsr_rows" in plan, plan
                check_against(add, vec_dict(w), mxv_terms, (t, src, entries, add, cmp_, "mxv"))
                w = u.vxm(Atm, sr)
                plan = gb.last_kernel_plan()
                assert plan.startswith(f"cmpsr<add={add},mul={cmp_},type={t},kind=vxm> ") and "k_cmpsr_rows" in plan, plan
                check_against(add, vec_dict(w), vxm_terms, (t, src, entries, add, cmp_, "vxm"))
                Cm = A.mxm(B, sr)
                assert Cm.type is gb.BOOL
                plan = gb.last_kernel_plan()
                assert plan.startswith(f"cmpsr<add={add},mul={cmp_},type={t},kind=mxm> ") and "k_cmpsr_product" in plan, plan
                check_against(add, mat_dict(Cm), mxm_terms, (t, src, entries, add, cmp_, "mxm"))
    assert seen_order


@pytest.mark.parametrize("t", ["INT8", "UINT64", "INT64", "FP32", "FP64"])
def test_edge_values_every_monoid_and_comparison(gb, gpu, t):
    run_edge_case(gb, t, t)


@pytest.mark.parametrize("src,t", [("FP64", "UINT8"), ("INT64", "FP32")])
def test_operands_of_another_type_are_cast_into_the_semirings_type(gb, gpu, src, t):
    run_edge_case(gb, t, src)


def test_any_with_terms_that_agree_and_terms_that_disagree(gb, gpu):
    """Row 0: 5 == 5 and 6 == 6 (the terms agree); row 1: 5 == 5 and 6 == 7 (they disagree: either is accepted, and the model says so)."""
    A = gb.Matrix.from_lists([0, 0, 1, 1], [0, 1, 0, 1], [5, 6, 5, 6], 2, 2, gb.INT64)
    u, u2 = gb.Vector.from_lists([0, 1], [5, 6], 2, gb.INT64), gb.Vector.from_lists([0, 1], [5, 7], 2, gb.INT64)
    Ad = {(0, 0): 5, (0, 1): 6, (1, 0): 5, (1, 1): 6}
    agree = {p[0]: ts for p, ts in product_terms("EQ", "INT64", Ad, {(0, 0): 5, (1, 0): 6}).items()}
    disagree = {p[0]: ts for p, ts in product_terms("EQ", "INT64", Ad, {(0, 0): 5, (1, 0): 7}).items()}
    assert fold("ANY", agree[0]) == {True} and fold("ANY", disagree[0]) == {True, False}
    check_against("ANY", vec_dict(A.mxv(u, gb.INT64.ANY_EQ)), agree, "agree")
    check_against("ANY", vec_dict(A.mxv(u2, gb.INT64.ANY_EQ)), disagree, "disagree")
    assert vec_dict(A.mxv(u, gb.INT64.ANY_EQ)) == {0: True, 1: True}
    B = gb.Matrix.from_lists([0, 1], [0, 0], [5, 7], 2, 1, gb.INT64)
    check_against("ANY", mat_dict(A.mxm(B, gb.INT64.ANY_EQ)), product_terms("EQ", "INT64", Ad, {(0, 0): 5, (1, 0): 7}), "mxm disagree")


# ---- the rows kernel: row lengths, the deciding term's place, absent operands, two rounds of the grid ---------------------------------------------------------------
NROWS, NCOLS = 20000, 4200
LENGTHS = [0, 1, 63, 64, 65, 128, 129, 4097]
ROW_CMPS = ["EQ", "NE", "GT", "LE"]
SAME, OTHER, STALE = 5, 6, 6      # u(k) = 5 where present; an absent u(k) carries 6: read, it would make a 6 of A compare equal and a 5 of A unequal


def absent(k):
    return k % 10 == 9


def special_rows():
    """(columns, values) lists.  `one true`: every present term is 6 == 5 (false) but one; `one false`: every present term is 5 == 5 but one; the absent columns of
    a row hold the value that would flip the answer if the stale u(k) were read.  Then rows whose counts of true and of false terms are odd and even over more
    than one stride, and a row all of whose u(k) are absent."""
    rows = []
    for L in LENGTHS:
        places = sorted({p for p in (0, 63, 64, L - 1) if 0 <= p < L})
        assert not any(absent(p) for p in places)
        for place in places or [None]:
            for fill, decide in ((OTHER, SAME), (SAME, OTHER)):
                rows.append((list(range(L)), [decide if k == place else fill for k in range(L)]))
    for L, trues in ((129, [0, 70, 128]), (129, [0, 70, 100, 128]), (200, [3]), (200, [])):          # odd / even counts of true terms, spread over strides
        rows.append((list(range(L)), [SAME if k in trues else OTHER for k in range(L)]))
    for L, falses in ((130, [5, 100]), (130, [5, 100, 128]), (70, [66]), (70, [])):                   # ... and of false terms
        rows.append((list(range(L)), [OTHER if k in falses else SAME for k in range(L)]))
    rows.append(([9, 19, 4099], [SAME, OTHER, SAME]))                                                   # every u(k) absent: no entry
    return rows


@pytest.fixture(scope="module")
def rows_case():
    """The rows, u and the model's terms per comparison: computed once, shared, never modified."""
    rng = np.random.default_rng(17)
    spec = special_rows()
    rows = [None] * NROWS
    for r, row in enumerate(spec):
        rows[r] = row
    second = [row for row in spec if len(row[0]) <= 200] + [next(row for row in spec if len(row[0]) == 4097)]      # beyond 16 384 waves: the short special rows again, and one of 4 097
    for r, row in enumerate(second):
        rows[16400 + r] = row
    for r in range(NROWS):
        if rows[r] is None:
            ln = int(rng.integers(0, 4))
            cols = sorted(rng.choice(NCOLS, size=ln, replace=False).tolist())
            rows[r] = (cols, rng.integers(4, 8, ln).tolist())
    lens = {len(c) for c, _ in rows[:len(spec)]}
    assert set(LENGTHS) <= lens and len(rows) == NROWS
    uval = np.where([absent(k) for k in range(NCOLS)], STALE, SAME).astype(np.int64)
    upres = np.array([0 if absent(k) else 1 for k in range(NCOLS)], np.uint8)
    terms = {}
    for cmp_ in ROW_CMPS:
        for swap in (False, True):
            out = {}
            by_value = {v: term(cmp_, "INT64", SAME, v) if swap else term(cmp_, "INT64", v, SAME) for v in range(4, 8)}      # (A holds 4..7, u holds 5)
            for r, (cols, vals) in enumerate(rows):
                ts = [by_value[v] for k, v in zip(cols, vals) if not absent(k)]
                if ts:
                    out[r] = ts
            terms[(cmp_, swap)] = out
    assert len(spec) - 1 not in terms[("EQ", False)] and 0 not in terms[("EQ", False)]               # the all-absent row and the empty row: no entry
    return rows, uval, upres, terms


def test_rows_kernel_row_lengths_deciding_places_and_absent_operands(gb, gpu, rows_case):
    rows, uval, upres, terms = rows_case
    i = np.repeat(np.arange(NROWS, dtype=np.uint64), [len(c) for c, _ in rows])
    j = np.concatenate([np.array(c, np.uint64) for c, _ in rows])
    x = np.concatenate([np.array(v, np.int64) for _, v in rows])
    A = gb.Matrix.from_arrays(i, j, x, NROWS, NCOLS, gb.INT64)
    At = gb.Matrix.from_arrays(j, i, x, NCOLS, NROWS, gb.INT64)
    u = gb.Vector.from_dense_array(uval, gb.INT64, present=upres)
    assert u.nvals == int(upres.sum())
    for cmp_ in ROW_CMPS:
        for add in ADDS:
            sr = getattr(gb.INT64, f"{add}_{cmp_}")
            w = A.mxv(u, sr)
            assert "k_cmpsr_rows" in gb.last_kernel_plan()
            check_against(add, vec_dict(w), terms[(cmp_, False)], (add, cmp_, "mxv"))
    for add, cmp_ in (("LOR", "GT"), ("LAND", "LE"), ("LXOR", "GT"), ("EQ", "LE"), ("ANY", "EQ")):
        sr = getattr(gb.INT64, f"{add}_{cmp_}")
        check_against(add, vec_dict(u.vxm(At, sr)), terms[(cmp_, True)], (add, cmp_, "vxm"))
        check_against(add, vec_dict(At.mxv(u, sr, desc=gb.descriptor.T0)), terms[(cmp_, False)], (add, cmp_, "mxv T0"))


# ---- the product kernel: rows of T of 1, 128, 129 and 600 entries ---------------------------------------------------------------------------------------------------
PM, PKK, PN = 36, 60, 700


def product_operands(rng):
    """A 36 x 60, B 60 x 700, values in 4..7.  Row 0 of T has 1 entry, row 1 128 (columns 0..127 from three overlapping rows of B), row 2 129, row 3 600 (eleven
    rows of B of 100 columns each, shifted by 50, and ten of 20 columns shifted by ONE from k to k + 1: the same slot is written by a lane at k and by its
    neighbour at k + 1); the others are short."""
    Ad, Bd = {}, {}

    def brow(k, cols):
        for c in cols:
            Bd[(k, c)] = int(rng.integers(4, 8))

    def arow(i, ks):
        for k in ks:
            Ad[(i, k)] = int(rng.integers(4, 8))
    brow(0, [77]); arow(0, [0])
    brow(1, range(0, 100)); brow(2, range(50, 128)); brow(3, range(0, 128, 2)); arow(1, [1, 2, 3])
    brow(4, [128]); arow(2, [1, 2, 3, 4])
    for q in range(11):
        brow(5 + q, range(50 * q, 50 * q + 100))
    for q in range(10):
        brow(16 + q, range(300 + q, 320 + q))
    arow(3, list(range(5, 26)))
    for k in range(26, PKK):
        brow(k, sorted(rng.choice(PN, size=int(rng.integers(0, 12)), replace=False).tolist()))
    for i in range(4, PM):
        if i != 9:
            arow(i, sorted(rng.choice(np.arange(26, PKK), size=int(rng.integers(0, 6)), replace=False).tolist()))
    return Ad, Bd


@pytest.fixture(scope="module")
def product_case():
    rng = np.random.default_rng(23)
    Ad, Bd = product_operands(rng)
    terms = {cmp_: product_terms(cmp_, "INT32", Ad, Bd) for cmp_ in ("EQ", "GT", "NE")}
    lens = {}
    for (i, _j) in terms["EQ"]:
        lens[i] = lens.get(i, 0) + 1
    assert lens[0] == 1 and lens[1] == 128 and lens[2] == 129 and lens[3] == 600 and max(v for r, v in lens.items() if r > 3) < 128
    mask = {(i, j): int(rng.integers(0, 2)) for i in range(PM) for j in range(PN) if rng.random() < 0.5}
    for j in range(300):
        mask[(3, j)] = 1                                               # the masked long row stays beyond the LDS capacity
    return Ad, Bd, terms, mask


def test_product_kernel_lds_and_global_rows_with_and_without_a_mask(gb, gpu, product_case):
    Ad, Bd, terms, mask = product_case
    A, B, Mk = matrix_of(gb, "INT32", Ad, PM, PKK), matrix_of(gb, "INT32", Bd, PKK, PN), matrix_of(gb, "INT8", mask, PM, PN)
    allowed = {p for p, v in mask.items() if v}
    for cmp_, ts in terms.items():
        for add in ADDS:
            sr = getattr(gb.INT32, f"{add}_{cmp_}")
            for name, kw, keep in (("unmasked", {}, lambda p: True), ("mask", {"mask": Mk}, lambda p: p in allowed),
                                   ("complemented", {"mask": Mk, "desc": gb.descriptor.C}, lambda p: p not in allowed)):
                Cm = A.mxm(B, sr, **kw)
                plan = gb.last_kernel_plan()
                assert plan.startswith(f"cmpsr<add={add},mul={cmp_},type=INT32,kind=mxm> k_cmpsr_product"), plan
                want = {p: t for p, t in ts.items() if keep(p)}
                assert len(want) < len(ts) or name == "unmasked"       # the mask drops products
                check_against(add, mat_dict(Cm), want, (add, cmp_, name))


# ---- the write-back: masks, replace, the accumulator, an output of another type, transposed inputs --------------------------------------------------------------------
def write_back_model(Cd, Td, Md, structural, comp, replace, accum, out_t):
    """C<M, replace> = accum(C, T): Td {p: bool} (a fold's answer), Cd {p: value of out_t}; the accumulator is LOR of the output's type."""
    one = (lambda b: bool(b)) if out_t == "BOOL" else (lambda b: 1 if b else 0)
    out = {}
    for p in set(Cd) | set(Td):
        allow = True if Md is None else (p in Md and (structural or Md[p] != 0))
        if Md is not None and comp:
            allow = not allow
        if not allow:
            if p in Cd and not replace:
                out[p] = Cd[p]
            continue
        if p in Td and p in Cd and accum:
            out[p] = one(bool(Cd[p]) or Td[p])
        elif p in Td:
            out[p] = one(Td[p])
        elif accum:
            out[p] = Cd[p]
    return out


def rand_dict(rng, t, shape, density, lo=4, hi=8):
    d = {}
    for p in itertools.product(*[range(s) for s in shape]):
        if rng.random() < density:
            v = int(rng.integers(lo, hi))
            d[p if len(shape) == 2 else p[0]] = float(v) + 0.5 * int(rng.integers(0, 2)) if M.is_fp(t) else v
    return d


def transpose(d):
    return {(j, i): v for (i, j), v in d.items()}


@pytest.mark.parametrize("kind", ["mxv", "vxm", "mxm"])
@pytest.mark.parametrize("t,srname", [("INT64", "LXOR_GT"), ("FP32", "EQ_LE"), ("INT64", "LOR_EQ")])
def test_write_back_variants(gb, gpu, kind, t, srname):
    rng = np.random.default_rng(zlib.crc32(f"{kind} {t} {srname}".encode()))
    add, cmp_ = srname.split("_")
    sr = getattr(getattr(gb, t), srname)
    m, kk, n = 23, 31, 17
    for name, mask_kind, comp, replace, accum_lor, transposed, other in VARIANTS:
        src = ("FP64" if t == "INT64" else "INT64") if other else t      # an operand of another type ...
        out_t = "INT32" if other else "BOOL"                              # ... and an output that receives 0 / 1
        OT = getattr(gb, out_t)
        accum = OT.LOR if accum_lor else None
        Ad = rand_dict(rng, src, (m, kk), 0.3)
        Ac = cast_dict(src, t, Ad)
        if kind == "mxm":
            Bd = rand_dict(rng, t, (kk, n), 0.3)
            Td = {p: fold(add, ts) for p, ts in product_terms(cmp_, t, Ac, Bd).items()}
            shape = (m, n)
        elif kind == "mxv":
            ud = rand_dict(rng, t, (kk,), 0.5)
            Td = {p[0]: fold(add, ts) for p, ts in product_terms(cmp_, t, Ac, {(k, 0): v for k, v in ud.items()}).items()}
            shape = (m,)
        else:
            ud = rand_dict(rng, t, (m,), 0.5)
            Td = {p[1]: fold(add, ts) for p, ts in product_terms(cmp_, t, {(0, k): v for k, v in ud.items()}, Ac).items()}
            shape = (kk,)
        Cd = rand_dict(rng, out_t, shape, 0.3, 0, 2)
        if out_t == "BOOL":
            Cd = {p: bool(v) for p, v in Cd.items()}
        Md = rand_dict(rng, "INT32", shape, 0.5, 0, 3) if mask_kind else None
        want = write_back_model(Cd, Td, Md, mask_kind == "struct", comp, replace, accum_lor, out_t)
        if kind == "mxm":
            A = matrix_of(gb, src, transpose(Ad) if transposed else Ad, kk if transposed else m, m if transposed else kk)
            B = matrix_of(gb, t, transpose(Bd) if transposed else Bd, n if transposed else kk, kk if transposed else n)
            out = matrix_of(gb, out_t, Cd, m, n)
            Mk = matrix_of(gb, "INT32", Md, m, n) if Md is not None else None
            A.mxm(B, sr, out=out, mask=Mk, accum=accum, desc=descriptor(gb, mask_kind == "struct", comp, replace, transposed, transposed))
            ci, cj, cx = out.to_arrays()
            got = {(int(a), int(b)): (bool(v) if out_t == "BOOL" else int(v)) for a, b, v in zip(ci.tolist(), cj.tolist(), cx.tolist())}
        else:
            stored = transpose(Ad) if transposed else Ad
            A = matrix_of(gb, src, stored, kk if transposed else m, m if transposed else kk)
            u = vector_of(gb, t, ud, kk if kind == "mxv" else m)
            out = vector_of(gb, out_t, Cd, shape[0])
            Mk = vector_of(gb, "INT32", Md, shape[0]) if Md is not None else None
            if kind == "mxv":
                A.mxv(u, sr, out=out, mask=Mk, accum=accum, desc=descriptor(gb, mask_kind == "struct", comp, replace, transposed, False))
            else:
                u.vxm(A, sr, out=out, mask=Mk, accum=accum, desc=descriptor(gb, mask_kind == "struct", comp, replace, False, transposed))
            idx, x = out.to_arrays()
            got = {int(p): (bool(v) if out_t == "BOOL" else int(v)) for p, v in zip(idx.tolist(), x.tolist())}
        assert gb.last_kernel_plan().startswith(f"cmpsr<add={add},mul={cmp_},type={t},kind={kind}> "), gb.last_kernel_plan()
        assert got == want, (kind, srname, name, sorted(set(got.items()) ^ set(want.items()))[:8])


# ---- the plan string, and the table route left alone ------------------------------------------------------------------------------------------------------------------
def test_plan_string_and_the_table_route_is_unchanged(gb, gpu):
    A = gb.Matrix.from_lists([0, 1, 2, 2], [1, 2, 0, 1], [3, 4, 5, 6], 3, 3, gb.INT64)
    u = gb.Vector.from_lists([0, 1, 2], [5, 3, 4], 3, gb.INT64)
    w = A.mxv(u, gb.INT64.LOR_EQ)
    assert gb.last_kernel_plan().startswith("cmpsr<add=LOR,mul=EQ,type=INT64,kind=mxv> k_cmpsr_rows"), gb.last_kernel_plan()
    assert w.type is gb.BOOL and vec_dict(w) == {0: True, 1: True, 2: True}
    u.vxm(A, gb.INT64.EQ_GE)
    assert gb.last_kernel_plan().startswith("cmpsr<add=EQ,mul=GE,type=INT64,kind=vxm> k_cmpsr_rows"), gb.last_kernel_plan()
    Cm = A.mxm(A, gb.INT64.LXOR_LT)
    assert Cm.type is gb.BOOL
    plan = gb.last_kernel_plan()
    assert plan.startswith("cmpsr<add=LXOR,mul=LT,type=INT64,kind=mxm> k_cmpsr_product pattern: "), plan
    for call in (lambda: A.mxv(u, gb.INT64.MAX_ISEQ), lambda: u.vxm(A, gb.INT64.MAX_ISEQ), lambda: A.mxm(A, gb.INT64.MAX_ISEQ)):
        r = call()
        plan = gb.last_kernel_plan()
        assert r.type is gb.INT64 and plan and "cmpsr<" not in plan and "k_cmpsr" not in plan, plan
    assert vec_dict(A.mxv(u, gb.INT64.MAX_ISEQ)) == vec_dict(w)
    # dimensions are checked as for every built-in semiring
    with pytest.raises(gb.DimensionMismatch):
        A.mxv(gb.Vector.sparse(gb.INT64, 4), gb.INT64.LOR_EQ)
    with pytest.raises(gb.DimensionMismatch):
        A.mxm(gb.Matrix.sparse(gb.INT64, 4, 3), gb.INT64.ANY_NE)


# ---- the other places a semiring can go -------------------------------------------------------------------------------------------------------------------------------
def test_semiring_entry_points_use_the_semirings_operators(gb, gpu):
    lib = gb.lib
    rng = np.random.default_rng(31)
    sr = C.c_void_p(gb._capi.handle("GxB_LOR_GT_INT32"))
    gt, lor = C.c_void_p(gb._capi.handle("GrB_GT_INT32")), C.c_void_p(gb._capi.handle("GrB_LOR"))
    Ad, Bd = rand_dict(rng, "INT32", (9, 7), 0.5, 0, 4), rand_dict(rng, "INT32", (9, 7), 0.5, 0, 4)
    ud, vd = rand_dict(rng, "INT32", (40,), 0.5, 0, 4), rand_dict(rng, "INT32", (40,), 0.5, 0, 4)
    A, B, u, v = matrix_of(gb, "INT32", Ad, 9, 7), matrix_of(gb, "INT32", Bd, 9, 7), vector_of(gb, "INT32", ud, 40), vector_of(gb, "INT32", vd, 40)

    def both(fn_sr, fn_op, op, make, *operands):
        a, b = make(), make()
        i1, i2 = fn_sr(a._h, None, None, sr, *[o._h for o in operands], None), fn_op(b._h, None, None, op, *[o._h for o in operands], None)
        assert i1 == 0 and i2 == 0, (fn_sr.__name__, i1, i2, last_error(gb))
        assert a.nvals > 0 and a.to_lists() == b.to_lists(), fn_sr.__name__
        return a

    newm = lambda r, c: (lambda: gb.Matrix.sparse(gb.BOOL, r, c))      # noqa: E731
    newv = lambda: gb.Vector.sparse(gb.BOOL, 40)                        # noqa: E731
    em = both(lib.GrB_Matrix_eWiseMult_Semiring, lib.GrB_Matrix_eWiseMult_BinaryOp, gt, newm(9, 7), A, B)
    assert mat_dict(em) == {p: Ad[p] > Bd[p] for p in Ad if p in Bd}
    both(lib.GrB_Matrix_eWiseAdd_Semiring, lib.GrB_Matrix_eWiseAdd_BinaryOp, lor, newm(9, 7), A, B)
    ev = both(lib.GrB_Vector_eWiseMult_Semiring, lib.GrB_Vector_eWiseMult_BinaryOp, gt, newv, u, v)
    assert vec_dict(ev) == {p: ud[p] > vd[p] for p in ud if p in vd}
    both(lib.GrB_Vector_eWiseAdd_Semiring, lib.GrB_Vector_eWiseAdd_BinaryOp, lor, newv, u, v)
    kr = both(lib.GrB_Matrix_kronecker_Semiring, lib.GrB_Matrix_kronecker_BinaryOp, gt, newm(81, 49), A, B)
    assert mat_dict(kr) == {(ia * 9 + ib, ja * 7 + jb): a > b for (ia, ja), a in Ad.items() for (ib, jb), b in Bd.items()}
