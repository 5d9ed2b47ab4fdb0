"""The product kernels a masked or sparse GrB_mxv / GrB_vxm runs (grb_spmv_kernels.hpp) against the numpy model of tests/product_model.py, at the row lengths
and grid sizes where their loops change shape, for every value width.  Every comparison is bit-exact on pattern and values (library against model on
`to_dense_arrays()`); an ANY monoid may keep any contribution of its row, so there the pattern is exact and the value must be one of the row's contributions.
Every case asserts on `gb.last_kernel_plan()` that the kernel it is about ran.

  (a) k_spmv_rowlane      a lane per row for SPMV_LANE_E = 8 entries, then the wave in steps of 64: the automatic choice for a masked pull whose monoid has a
                          terminal and whose rows hold <= 96 entries on average;
  (b) k_spmv_rowgroup     G = 8 and G = 64, forced; G = 8 past its 65 536 workgroups x 32 groups;
  (c) k_spmv_adaptive     the row-block kernel under a mask over a bitmap operand: masked long-row parts, whole blocks masked, partial flags, tickets;
  (d) k_spmv_rowlane_k    the fused BOOL pull `q<v> = v lor.land A` (mask = operand): row heads, code bytes, the second round of its capped grid;
  (e) k_spmspv_push / k_spmspv_push_long   the host list of <= 64 entries, more operand entries than waves, hub rows at 4096 / 4097, both long-row modes,
                          and the positions the kernels exclude themselves (`excl_small`).

The ladder (built once): rows of exactly LADDER entries with runs of empty rows between them, the first row empty, the last row non-empty and the last lane
of a partial wave, padded with rows of 0 to 12 entries.  Values are small non-zero integers / the 1/8 grid (every summation order is exact: asserted by
`assert_exact_sums`), and the matrix values carry what PLAN plants (multipliers that pass the matrix value through: FIRST in mxv, SECOND in vxm, LAND / LOR):
the monoid's terminal inside the first 8 entries, between entry 9 and 72, in the last entry, at an entry whose operand position is absent (the row must go
on), in a row the mask rejects; decoys a wrong terminal would match (0, the identity, the negated extreme), each followed by a value that still changes the
result.  The values behind the operand's holes are terminals too.  The measurement hooks GRB_MI355X_LANE_K = 1 / 2 and G = 64 past its grid cap are left out."""
import functools
import os

import numpy as np
import pytest

import matrix_model as MM
import vector_model as VM
import product_model as PM
import pygraphblas_amd as gb
from helpers import TYPE
from test_matrix_kernels_at_size_gpu import desc_of, same_bits
from test_vector_kernels_at_size_gpu import check, dev

pytestmark = pytest.mark.gpu

TYPES = ["BOOL", "INT8", "UINT16", "INT32", "FP32", "INT64", "UINT64", "FP64"]      # one type per value width and kind
NP = MM.NP
LADDER = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 71, 72, 73, 136, 137, 2048, 2049, 4096, 4097, 8192, 8193, 16385]
NROWS, NCOLS = 30015, 20011
N_FUSED_BIG = 1048576 + 1000 + 37
N_ROWGROUP_BIG = 2097152 + 4099
N_PUSH = 70001
# what is planted into the row of a given length: (kind, entry).  T terminal, Ta terminal at an absent operand position, D the next decoy, B a value that is
# better than every decoy without being the terminal.  The row of MASKED_LEN entries is rejected by every mask.
PLAN = {4: [("D", 0), ("B", 3)], 5: [("T", 4)], 7: [("Ta", 2)], 8: [("T", 7)], 9: [("T", 8)], 63: [("T", 3)], 64: [("T", 40)], 65: [("T", 64)],
        71: [("D", 1), ("Ta", 5), ("B", 70)], 72: [("T", 71)], 73: [("T", 72)], 136: [("Ta", 100)], 137: [("D", 2), ("D", 20), ("D", 130), ("T", 136)],
        2048: [("D", 2), ("D", 20), ("B", 2047)], 2049: [("T", 2048)], 4096: [("T", 4)], 4097: [("D", 0), ("T", 4096)], 8192: [("T", 5000)],
        8193: [("D", 9), ("Ta", 30), ("B", 8192)], 16385: [("T", 16384)]}
MASKED_LEN = 4096
STRETCH = (12000, 17000)                # consecutive rows every mask rejects: whole row blocks of the row-block kernel


# ---- patterns, built once ------------------------------------------------------------------------------------------------------------------------------------
class Pattern:
    def __init__(self, nrows, ncols, lens, cols):
        self.nrows, self.ncols = nrows, ncols
        self.rp = np.zeros(nrows + 1, np.int64); np.cumsum(lens, out=self.rp[1:])
        self.ci = cols; self.rows = np.repeat(np.arange(nrows), lens); self.keys = self.rows * np.int64(ncols) + cols
        self.lens = lens; self.row_of = {}
        for a in (self.rp, self.ci, self.rows, self.keys, self.lens): a.setflags(write=False)

    @property
    def nnz(self): return len(self.ci)

    def at(self, length, entry): return int(self.rp[self.row_of[length]] + entry)


def short_rows(rng, n, ncols, most):
    """Rows of 0 .. `most` entries: entry k of a row falls into the k-th of `most` strata of the columns (distinct and ascending)."""
    lens = rng.integers(0, most + 1, n); lens[-1] = max(lens[-1], 1); width = ncols // most
    k = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    return lens, k * width + rng.integers(0, width, len(k))


def build(nrows, ncols, fixed, most, seed, run=40):
    """`fixed`: {row: length} rows of exactly that many entries (columns drawn without replacement), a run of `run` empty rows in front of each; every other
    row is short; the first row is empty and the last is not."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, most + 1, nrows)
    for r in fixed: lens[max(r - run, 0): r] = 0
    lens[0] = 0; lens[-1] = max(lens[-1], 1)
    for r, l in fixed.items(): lens[r] = l
    rp = np.concatenate(([0], np.cumsum(lens)))
    k = np.arange(rp[-1]) - np.repeat(rp[:-1], lens)
    cols = k * (ncols // most) + rng.integers(0, ncols // most, len(k))               # (short rows; the fixed rows are drawn below)
    for r, l in fixed.items():
        cols[rp[r]: rp[r + 1]] = np.sort(rng.choice(ncols, size=l, replace=False))
    p = Pattern(nrows, ncols, lens, cols)
    p.row_of = {l: r for r, l in fixed.items()}
    return p


@functools.lru_cache(maxsize=None)
def ladder(ncols=NCOLS):
    gaps = np.resize([41, 64, 70, 129, 47], len(LADDER))                            # (runs of 40 empty rows end inside and at the end of a wave)
    at = 1 + np.cumsum(gaps)
    return build(NROWS, ncols, {int(r): l for r, l in zip(at, LADDER) if l}, 12, 1)


@functools.lru_cache(maxsize=None)
def wide():
    """G = 64: 400 rows of 100 to 300 entries, every other row, and the ladder's long rows: more than 96 entries per row on average."""
    rng = np.random.default_rng(2)
    fixed = {int(r): int(l) for r, l in zip(range(1, 801, 2), rng.integers(100, 301, 400))}
    fixed.update({803 + 3 * k: l for k, l in enumerate(l for l in LADDER if l >= 2048)})
    return build(826, NCOLS, fixed, 12, 3, run=1)


@functools.lru_cache(maxsize=None)
def fused_big():
    """The ladder's rows in front of a million rows of 0 to 2 entries, square."""
    L = ladder(NROWS); n = N_FUSED_BIG
    lens, cols = short_rows(np.random.default_rng(4), n - NROWS, n, 2)
    p = Pattern(n, n, np.concatenate([L.lens, lens]), np.concatenate([L.ci, cols]))
    p.row_of = dict(L.row_of)
    return p


@functools.lru_cache(maxsize=None)
def rowgroup_big():
    rng = np.random.default_rng(5)
    lens, cols = short_rows(rng, N_ROWGROUP_BIG, NCOLS, 2)
    return Pattern(N_ROWGROUP_BIG, NCOLS, lens, cols)


PUSH_LISTED = np.array(sorted(set(range(5, 64 * 1000, 1000)) | {7}))[:64]            # the 64 positions of the host-list operands
N_HUBS_4097, N_HUBS_4096 = 140, 10


@functools.lru_cache(maxsize=None)
def push_pattern():
    """Square, >= 2^20 entries: 140 rows of 4097 entries (more than the gridDim / 8 = 128 that switch k_spmspv_push_long to one block per row), 10 rows of
    4096, rows of 0 to 14 entries elsewhere.  The first hub row is a listed position and holds every listed position among its columns."""
    rng = np.random.default_rng(6); n = N_PUSH
    hubs = [int(PUSH_LISTED[0])] + list(range(300, 300 + 450 * (N_HUBS_4097 + N_HUBS_4096 - 1), 450))
    fixed = {r: (4097 if k < N_HUBS_4097 else 4096) for k, r in enumerate(hubs)}
    p = build(n, n, fixed, 14, 7)
    ci = p.ci.copy(); r0 = hubs[0]
    rest = np.setdiff1d(rng.choice(n, size=5000, replace=False), PUSH_LISTED)[: 4097 - 64]
    ci[p.rp[r0]: p.rp[r0 + 1]] = np.sort(np.concatenate([PUSH_LISTED, rest]))
    # a short listed row whose first column is a listed position too (both in the first stratum of the columns): k_spmspv_push itself must skip it
    short = next(int(r) for r in PUSH_LISTED[1:5] if 0 < p.lens[r] <= 14)
    ci[p.rp[short]] = next(int(c) for c in PUSH_LISTED[1:6] if c != short)
    q = Pattern(n, n, p.lens, ci); q.row_of = {}; q.hubs = hubs; q.short_listed = short
    return q


def test_the_shapes_are_what_the_kernels_need(gpu):
    """The constants are those of grb_spmv_kernels.hpp and grb_spmv.hpp: SPMV_LANE_E = 8, a wave step of 64, four head columns and the "more" bit, 256 rows per
    workgroup of the lane-per-row kernel, <= 96 entries per row for it, 256 workgroups x 1024 threads x 4 rows of the fused kernel, 65 536 x 32 row groups,
    SPMV_NNZ = 2048 and SPMV_LONG_CHUNK = 8192 of the row-block kernel, PUSH_LONG = 4096, 16 384 workgroups x 4 waves and 1024 / 8 long rows of the push."""
    for L in (ladder(), ladder(NROWS)):
        assert sorted(L.row_of) == LADDER[1:] and all(L.lens[r] == l for l, r in L.row_of.items())
        assert L.lens[0] == 0 and L.lens[-1] > 0 and L.nrows % 256 and L.nrows % 64 and L.nrows > 100 * 256 and L.ncols >= 20000
        assert all((L.lens[r - 40: r] == 0).all() for r in L.row_of.values())          # runs of empty rows
        assert L.nnz / L.nrows <= 96 and all(np.all(np.diff(L.ci[L.rp[r]: L.rp[r + 1]]) > 0) for r in L.row_of.values())
        assert np.all(np.diff(L.keys) > 0)
        assert all(e < l for l, plan in PLAN.items() for _, e in plan) and set(PLAN) <= set(LADDER)
        assert (L.lens[STRETCH[0]: STRETCH[1]] > 0).sum() > 2048 and not any(STRETCH[0] <= r < STRETCH[1] for r in L.row_of.values())
    assert (16385 + 8191) // 8192 == 3 and 8193 > 8192 and 2049 > 2048                 # a three-part row, a two-part row, a one-part long row
    W = wide(); assert W.nnz / W.nrows > 96 and np.all(np.diff(W.keys) > 0) and ((W.lens >= 100) & (W.lens <= 300)).sum() >= 400
    F = fused_big(); assert F.nrows == F.ncols and F.nrows > 256 * 1024 * 4 and (F.nrows - 256 * 1024 * 4) % 256 and F.nnz >= 1 << 20 and F.nnz / F.nrows <= 96 and F.nrows >= 1 << 16
    assert np.all(np.diff(F.keys) > 0) and F.lens[-1] > 0
    R = rowgroup_big(); assert R.nrows > 65536 * 32 and R.lens.max() == 2 and R.nnz / R.nrows <= 96
    P = push_pattern(); assert P.nnz >= 1 << 20 and (P.lens == 4097).sum() == N_HUBS_4097 >= 128 and (P.lens == 4096).sum() == N_HUBS_4096 and np.all(np.diff(P.keys) > 0)
    s0 = P.short_listed; assert 0 < P.lens[s0] <= 14 and s0 in PUSH_LISTED and P.ci[P.rp[s0]] in PUSH_LISTED and P.ci[P.rp[s0]] != s0
    assert len(PUSH_LISTED) == 64 and np.isin(PUSH_LISTED, P.ci[P.rp[P.hubs[0]]: P.rp[P.hubs[0] + 1]]).all() and P.nrows > 65537 + 1000 and 65537 + 1000 > 16384 * 4


# ---- values -----------------------------------------------------------------------------------------------------------------------------------------------------
def specials(typ, add):
    """The monoid's terminal T, decoys D a wrong terminal would match (0, the identity, the negated extreme) and a value B better than all of them."""
    t = NP[typ]
    if typ == "BOOL":
        term = {"LOR": True, "LAND": False, "ANY": False, "LXOR": None}[MM.BOOL_RENAME.get(add, add)]
        return None if term is None else dict(T=np.bool_(term), D=[np.bool_(not term)], B=np.bool_(not term))
    fp = typ.startswith("FP"); signed = fp or typ[0] != "U"
    lo, hi, big = (t(-np.inf), t(np.inf), np.finfo(t).max) if fp else (t(np.iinfo(t).min), t(np.iinfo(t).max), t(np.iinfo(t).max))
    if add == "MIN": return dict(T=lo, D=[t(0), hi, t(-big)] if signed else [hi, t(1)], B=t(-100) if signed else t(1))
    if add == "MAX": return dict(T=hi, D=[t(0), lo, big if fp else t(hi - t(1))], B=t(100))
    if add == "TIMES" and not fp: return dict(T=t(0), D=[t(1), t(-1) if signed else hi], B=t(3))
    if add == "ANY": return dict(T=t(0), D=[t(1)], B=t(2))
    return None


def base_values(rng, typ, n, add):
    """Small, non-zero, away from every special value: 2 .. 7 in size (odd under TIMES, whose products then never wrap to 0); mostly the value that decides
    nothing under a BOOL monoid."""
    if typ == "BOOL":
        term = (specials(typ, add) or {}).get("T")
        return (rng.random(n) < 0.5) if term is None else np.where(rng.random(n) < 0.03, term, not term)
    mag = rng.choice([3, 5, 7], size=n) if add == "TIMES" else rng.integers(2, 8, n)
    sign = 1 if typ[0] == "U" else rng.choice([1, -1], size=n)
    return (mag * sign / (8.0 if typ.startswith("FP") else 1)).astype(NP[typ])


def plant(L, vals, typ, add):
    """PLAN into the matrix values; returns the columns that must be absent from an operand with holes, negated (-1 - c), and those that must be present."""
    s = specials(typ, add); absent = []; present = []
    if s is None: return np.zeros(0, np.int64)
    for length, plan in PLAN.items():
        if length not in L.row_of: continue
        d = 0
        for kind, e in plan:
            p = L.at(length, e)
            if kind == "D": vals[p] = s["D"][d % len(s["D"])]; d += 1
            elif kind == "B": vals[p] = s["B"]
            else: vals[p] = s["T"]
            (absent if kind == "Ta" else present).append(L.ci[p])
    assert not set(absent) & set(present)
    return np.array([-1 - c for c in absent] + present, np.int64)


@functools.lru_cache(maxsize=None)
def matrix(which, typ, add):
    """(model, device matrix) with PLAN planted for the monoid `add`; shared and never written to."""
    L = {"ladder": ladder, "wide": wide, "square": lambda: ladder(NROWS)}[which]()
    vals = base_values(np.random.default_rng([TYPES.index(typ), len(add)]), typ, L.nnz, add)
    absent = plant(L, vals, typ, add); vals.setflags(write=False)
    return L, MM.Mat(L.nrows, L.ncols, L.keys, vals), upload(L, typ, vals), absent


def upload(L, typ, vals):
    return gb.Matrix.from_csr(TYPE[typ], L.nrows, L.ncols, L.rp.astype(np.uint32), L.ci.astype(np.uint32), vals)


def operand(typ, n, add, holes, absent, seed):
    """Values at every position (what lies behind a hole is the monoid's terminal: it must not matter); a few present terminals and decoys as well."""
    rng = np.random.default_rng([seed, n % 1000003]); s = specials(typ, add)
    x = base_values(rng, typ, n, add)
    pres = np.ones(n, bool)
    if holes:
        pres = rng.random(n) < 0.7; pres[absent[absent >= 0]] = True; pres[-1 - absent[absent < 0]] = False
    if s is not None:
        if typ != "BOOL": x[rng.choice(n, size=6, replace=False)] = [s["T"], s["T"]] + [s["D"][k % len(s["D"])] for k in range(3)] + [s["B"]]
        x[~pres] = s["T"]
    return VM.Vec(x, pres)


def make_mask(allow, mtyp, struct, comp, rng):
    """A mask vector under which exactly the rows of `allow` may be written."""
    truth = allow != comp; n = len(allow); t = NP[mtyp]
    if struct: return VM.Vec(rng.choice(np.array([0, 1], t), size=n), truth)
    true_v = np.array([True] if mtyp == "BOOL" else [1.5, np.nan, -2.0] if mtyp == "FP64" else [1, 200], t)
    return VM.Vec(np.where(truth, rng.choice(true_v, size=n), t(0)), truth | (rng.random(n) < 0.3))


def allow_rows(L, rng):
    a = rng.random(L.nrows) < 0.6
    a[STRETCH[0]: STRETCH[1]] = False
    for l, r in L.row_of.items(): a[r] = l != MASKED_LEN
    a[-1] = True
    return a


MASKS = [("BOOL", False, False), ("UINT8", True, False), ("FP64", False, True), ("BOOL", True, True), ("UINT8", False, True), ("FP64", True, False)]


def assert_exact_sums(typ, sr, M, u):
    """Floating point: the sum of |products| of the longest row, in units of the grid (1/64: products of two values on the 1/8 grid), stays below 2^24 (FP32) /
    2^53 (FP64), so a PLUS monoid is exact in every order.  (MIN / MAX compare and round nothing in any order; the one addition of a MIN_PLUS product is the same
    IEEE operation in the kernel and in the model.)"""
    add, mul = sr.split("_")
    if not typ.startswith("FP") or add != "PLUS": return
    bound = 2.0 ** 24 if typ == "FP32" else 2.0 ** 53
    live = u.pres[M.cols]; x = np.abs(M.vals[live].astype(np.float64)); y = np.abs(u.val[M.cols[live]].astype(np.float64))
    assert mul == "TIMES" and np.isfinite(x).all() and np.isfinite(y).all()
    p = x * y * 64
    assert np.all(p == np.round(p)) and np.bincount(M.rows[live], weights=p).max() < bound


def run(form, a, A, U, sr, typ, W=None, mask=None, struct=False, comp=False, replace=False, accum=None, method=None, expect=(), what=""):
    """One product on the device and in the model.  `form`: "mxv" is w = A u, "vxm_t" is w' = u' A' (desc T1): both pull over the rows of A as stored;
    "vxm" is w' = u' A: the push walks the rows of A as stored."""
    add, mul = sr.split("_"); T = TYPE[typ]
    n_out = A.ncols if form == "vxm" else A.nrows
    W = VM.empty(n_out, typ) if W is None else W
    w, u = dev(W), dev(U, full=bool(U.pres.all())); m = None if mask is None else dev(mask)
    acc = None if accum is None else getattr(T, accum)
    if method: os.environ["GRB_MI355X_SPMV"] = method
    try:
        if form == "mxv": a.mxv(u, semiring=getattr(T, sr), out=w, mask=m, accum=acc, desc=desc_of(replace, struct, comp))
        else: u.vxm(a, semiring=getattr(T, sr), out=w, mask=m, accum=acc, desc=desc_of(replace, struct, comp, t1=form == "vxm_t"))
    finally:
        os.environ.pop("GRB_MI355X_SPMV", None)
    plan = gb.last_kernel_plan(); what = f"{what} {form} {typ}.{sr} mask={None if mask is None else mask.typ} struct={struct} comp={comp} replace={replace} accum={accum} plan={plan}"
    for e in expect: assert e in plan, what
    kw = dict(mask=mask, struct=struct, comp=comp, replace=replace, accum=(accum, typ) if accum else None)
    exp = PM.mxv(W, A, U, add, mul, typ, **kw) if form == "mxv" else PM.vxm(W, U, A, add, mul, typ, tran=form == "vxm_t", **kw)
    if add == "ANY" and typ != "BOOL": check_any(w, exp, form, A, U, mul, typ, W, mask, struct, comp, what)
    else: check(w, exp, what)
    return w, exp


def check_any(w, exp, form, A, U, mul, typ, W, mask, struct, comp, what):
    """An ANY monoid: the model's pattern; where the product wrote, the value of some contribution of the row; elsewhere the model's value."""
    x, p = w.to_dense_arrays(); p = p != 0
    assert np.array_equal(p, exp.pres), f"{what}: the pattern differs at {np.flatnonzero(p != exp.pres)[:6].tolist()}"
    M = A if form != "vxm" else MM.transpose(A)
    live = U.pres[M.cols]; rows = M.rows[live]
    a, b = M.vals[live], U.val[M.cols[live]]
    z = PM.mult(mul, typ, a, b) if form == "mxv" else PM.mult(mul, typ, b, a)
    hit = np.zeros(M.nrows, bool); hit[rows[same_bits(z, x[rows])]] = True
    wrote = VM.mask_allows(mask, struct, comp, M.nrows) & np.bincount(rows, minlength=M.nrows).astype(bool)
    assert hit[wrote].all(), f"{what}: {int((~hit[wrote]).sum())} values are no contribution of their row, first at {np.flatnonzero(wrote & ~hit)[:6].tolist()}"
    rest = p & ~wrote
    assert same_bits(x[rest], exp.val[rest]).all(), what


def passes_matrix_value(sr, form):
    """The multiplier hands the matrix value through: FIRST sees the matrix first in mxv, SECOND in vxm."""
    mul = sr.split("_")[1]
    return mul in ("LAND", "LOR") or mul == ("FIRST" if form == "mxv" else "SECOND")


def pull_cases(typ, which, semirings, method, expect, seed, forms=("mxv", "vxm_t"), unmasked=False):
    rng = np.random.default_rng(seed); k = 0
    for sr in semirings:
        add = sr.split("_")[0]
        L, A, a, absent = matrix(which, typ, add)
        allow = allow_rows(L, rng) if which != "wide" else rng.random(L.nrows) < 0.6
        for form in forms:
            for holes in (True, False):
                U = operand(typ, L.ncols, add, holes, absent, seed + k)
                assert_exact_sums(typ, sr, A, U)
                mtyp, struct, comp = MASKS[k % len(MASKS)]
                mask = None if (unmasked and k % 3 == 2) else make_mask(allow, mtyp, struct, comp, rng)
                if mask is None: struct = comp = False                                # (no mask, complemented: nothing may be written)
                accum = (None, None, "LOR" if typ == "BOOL" else "MIN", None, "LAND" if typ == "BOOL" else "PLUS")[k % 5] if add != "ANY" else None
                replace = bool(k % 2) and mask is not None
                W = operand(typ, L.nrows, "PLUS", True, np.zeros(0, np.int64), seed + 50 + k) if (accum or not replace) else None
                run(form, a, A, U, sr, typ, W, mask, struct, comp, replace, accum, method, expect, what=f"{which} holes={holes}")
                k += 1


# ---- (a) a lane per row, the automatic choice -------------------------------------------------------------------------------------------------------------------
def lane_semirings(typ):
    if typ == "BOOL": return ["LOR_LAND", "LAND_LOR", "ANY_PAIR"]
    return ["MIN_FIRST", "MAX_FIRST", "MIN_SECOND", "MAX_SECOND", "ANY_SECOND", "MIN_PLUS"] + ([] if typ.startswith("FP") else ["TIMES_FIRST", "TIMES_SECOND"])


@pytest.mark.parametrize("typ", TYPES)
def test_lane_per_row_on_the_ladder(gpu, typ):
    """k_spmv_rowlane by the automatic choice (a mask that is not the operand, a monoid with a terminal): every ladder row, full operands and operands with
    holes, six mask kinds in turn, with and without accumulator and replace, as mxv and as vxm.  FIRST (mxv) and SECOND (vxm) carry the planted matrix values."""
    assert all(passes_matrix_value(sr, f) for sr, f in (("MIN_FIRST", "mxv"), ("MIN_SECOND", "vxm_t"), ("LOR_LAND", "mxv"))) and not passes_matrix_value("MIN_FIRST", "vxm_t")
    pull_cases(typ, "ladder", lane_semirings(typ), None, ("k_spmv_rowlane<",), 100 + TYPES.index(typ))


# ---- (b) row groups, forced ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_row_groups_of_8_on_the_ladder(gpu, typ):
    srs = ["LOR_LAND", "LAND_LOR"] if typ == "BOOL" else ["MIN_FIRST", "MAX_SECOND", "ANY_SECOND", "PLUS_TIMES"]
    pull_cases(typ, "ladder", srs, "rowgroup", ("k_spmv_rowgroup<G=8",), 200 + TYPES.index(typ), unmasked=True)


@pytest.mark.parametrize("typ", ["BOOL", "UINT16", "FP32", "INT64"])
def test_row_groups_of_64_on_long_rows(gpu, typ):
    srs = ["LOR_LAND", "ANY_PAIR"] if typ == "BOOL" else ["MIN_FIRST", "MAX_SECOND", "PLUS_TIMES"]
    pull_cases(typ, "wide", srs, "rowgroup", ("k_spmv_rowgroup<G=64",), 300 + TYPES.index(typ), unmasked=True)


def test_row_groups_of_8_past_their_grid(gpu):
    """More rows than 65 536 workgroups x 32 groups: the row loop strides.  INT32 MIN_FIRST with terminals at one entry in a hundred, a valued mask, holes."""
    R = rowgroup_big(); rng = np.random.default_rng(8); s = specials("INT32", "MIN")
    vals = base_values(rng, "INT32", R.nnz, "MIN"); vals[rng.random(R.nnz) < 0.01] = s["T"]
    A = MM.Mat(R.nrows, R.ncols, R.keys, vals); a = upload(R, "INT32", vals)
    U = operand("INT32", R.ncols, "MIN", True, np.zeros(0, np.int64), 9)
    allow = rng.random(R.nrows) < 0.6; allow[-5000:] = True
    mask = make_mask(allow, "BOOL", False, False, rng)
    run("mxv", a, A, U, "MIN_FIRST", "INT32", None, mask, method="rowgroup", expect=("k_spmv_rowgroup<G=8",), what="past the grid")
    run("vxm_t", a, A, U, "MIN_SECOND", "INT32", None, mask, replace=True, method="rowgroup", expect=("k_spmv_rowgroup<G=8",), what="past the grid")


# ---- (c) the row-block kernel under a mask, over a bitmap operand -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_row_blocks_under_a_mask_over_a_bitmap_operand(gpu, typ):
    """k_spmv_adaptive<bitmap, mask>: PLUS_TIMES by the automatic choice (BOOL: LXOR_LAND, the monoid without a terminal) and MIN_FIRST (mxv) / MIN_SECOND (vxm) forced.  The mask rejects
    the 4096-entry row, a stretch of 5000 consecutive rows (whole row blocks) and — in the second half of the cases — the three-part row of 16 385 entries,
    whose part 0 then writes the absent byte; an operand present only at the columns of that row's middle part leaves its first and last partial flag clear;
    every product runs twice on the same matrix (the tickets re-arm) with equal results."""
    L = ladder(); rng = np.random.default_rng(400 + TYPES.index(typ))
    for sr, method in (("LXOR_LAND" if typ == "BOOL" else "PLUS_TIMES", None), ("LOR_LAND" if typ == "BOOL" else "MIN_FIRST", "adaptive")):
        add = sr.split("_")[0]
        _, A, a, absent = matrix("ladder", typ, add)
        r3 = L.row_of[16385]; mid = L.ci[L.rp[r3] + 8192: L.rp[r3] + 16384]
        for k, (kind, form) in enumerate((("holes", "mxv"), ("middle", "vxm_t"), ("holes, long row masked", "vxm_t"), ("middle, long row masked", "mxv"))):
            U = operand(typ, L.ncols, add, True, absent, 410 + k)
            if kind.startswith("middle"):
                pres = np.zeros(L.ncols, bool); pres[mid] = True; U = VM.Vec(U.val, pres)
            assert_exact_sums(typ, sr, A, U)
            allow = allow_rows(L, rng); allow[r3] = "masked" not in kind
            mtyp, struct, comp = MASKS[(k + TYPES.index(typ)) % len(MASKS)]
            mask = make_mask(allow, mtyp, struct, comp, rng)
            accum = (None, "LOR" if typ == "BOOL" else "PLUS")[k % 2]; replace = k >= 2
            W = operand(typ, L.nrows, "PLUS", True, np.zeros(0, np.int64), 420 + k)
            s_f = "MIN_SECOND" if (sr == "MIN_FIRST" and form == "vxm_t") else sr           # (the multiplier that hands the planted matrix value through)
            assert passes_matrix_value(s_f, form) or add not in ("MIN", "LOR")
            w1, exp = run(form, a, A, U, s_f, typ, W, mask, struct, comp, replace, accum, method, ("k_spmv_adaptive<", ",bitmap,mask>"), what=kind)
            w2, _ = run(form, a, A, U, s_f, typ, W, mask, struct, comp, replace, accum, method, ("k_spmv_adaptive<", ",bitmap,mask>"), what=kind + ", again")
            assert exp.pres[r3] == (allow[r3] or (W.pres[r3] and not replace))
            assert w1.iseq(w2)


# ---- (d) the fused BOOL pull --------------------------------------------------------------------------------------------------------------------------------------
def level_vector(n, seed):
    """A UINT8 level vector: half of the positions hold an entry, a third of the entries are explicit zeros."""
    rng = np.random.default_rng(seed)
    return VM.Vec(rng.choice(np.array([0, 1, 2], np.uint8), size=n), rng.random(n) < 0.5)


def fused_case(L, a_pull, a_t, A, V, source, flags, forms, code, what):
    """q<v> = v (+).(x) A with the mask the operand itself, as `v.vxm(A', mask=v)` and `A.mxv(v, mask=v)`: against the model, and `reduce_bool` against a scan."""
    sr = "ANY_PAIR" if source == "ANY_PAIR" else "LOR_LAND"; add, mul = sr.split("_")
    struct, comp = "S" in flags, "C" in flags
    for form in forms:
        v = dev(V); q = gb.Vector.sparse(gb.BOOL, L.nrows)
        if form == "vxm": v.vxm(a_t, semiring=getattr(gb.BOOL, sr), mask=v, out=q, desc=desc_of(True, struct, comp))
        else: a_pull.mxv(v, semiring=getattr(gb.BOOL, sr), mask=v, out=q, desc=desc_of(True, struct, comp))
        plan = gb.last_kernel_plan(); w = f"{what} {source} {flags} {form} plan={plan}"
        assert "k_spmv_rowlane<" in plan and "mask=operand" in plan and ("code bytes" in plan) == code, w
        t = PM.product(add, mul, "BOOL", A, V, flip=form == "vxm")
        exp = VM.write_back(VM.empty(L.nrows, "BOOL"), t, V, struct, comp, True)
        got = q.reduce_bool()
        check(q, exp, w)
        assert got is bool(np.any(exp.val[exp.pres])), w
    return exp


def fused_values(L, source, seed):
    """Matrix values with stored `false` everywhere: among the four head columns, at entries 4 to 7 and beyond 8 (nine entries in ten, and what PLAN plants
    for LOR: `true` is the terminal); INT64 for the cast source."""
    vals = np.random.default_rng(seed).random(L.nnz) < 0.1
    for length, plan in PLAN.items():
        for kind, e in plan: vals[L.at(length, e)] = kind in ("T", "Ta")
    for l in (5, 9, 65):                                                                 # (only the last entry decides: past the heads, the lane stage, a wave step)
        r = L.row_of[l]; vals[L.rp[r]: L.rp[r + 1] - 1] = False; vals[L.rp[r + 1] - 1] = True
    return np.where(vals, 7, 0).astype(np.int64) if source == "INT64" else vals


DECIDED_BY_LAST = (5, 9, 65)


def pin_level_vector(L, V):
    """The rows of 5, 9 and 65 entries, whose last entry alone is true: unvisited themselves (allowed under RC), every neighbour with a level, the last one's
    not zero — so the result of each is `true`, and only through the entry behind the "more" bit, the lane stage and the first wave step."""
    for l in DECIDED_BY_LAST:
        r = L.row_of[l]; cols = L.ci[L.rp[r]: L.rp[r + 1]]
        V.pres[cols] = True; V.val[cols[-1]] = 2
    rows = [L.row_of[l] for l in DECIDED_BY_LAST]
    V.pres[rows] = False
    assert all(V.pres[L.ci[L.rp[r]: L.rp[r + 1]]].all() for r in rows)
    return rows


def fused_upload(L, x):
    """The model, the pull matrix (rows as in L) and its transpose for the vxm form."""
    typ = MM.NAME[x.dtype]
    A = MM.Mat(L.nrows, L.ncols, L.keys, x); At = MM.transpose(A)
    rp, ci, xt = MM.to_csr(At)
    return A, upload(L, typ, x), gb.Matrix.from_csr(TYPE[typ], At.nrows, At.ncols, rp, ci, xt)


@pytest.mark.parametrize("source", ["BOOL", "INT64", "ANY_PAIR"])
def test_fused_pull_with_row_heads(gpu, source):
    """n = 30 015: row heads, no code bytes (the matrix is too small for them).  A BOOL matrix under LOR_LAND (heads with value bits), an INT64 matrix under
    LOR_LAND (cast: no heads), BOOL ANY_PAIR (heads without values); descriptors RC, RSC, R, RS; then one head entry of the matrix becomes `false` through
    setElement and the products repeat: stale row heads must not survive."""
    L = ladder(NROWS); x = fused_values(L, source, 500)
    V = level_vector(L.nrows, 501)
    r = L.row_of[3]; cols = L.ci[L.rp[r]: L.rp[r + 1]]                                  # the row of three entries: allowed under RC, decided by its first entry alone
    x[L.rp[r]: L.rp[r + 1]] = [1, 0, 0]
    pinned = pin_level_vector(L, V)
    V.pres[r] = False; V.pres[cols] = True; V.val[cols] = [2, 0, 1]
    assert not V.pres[pinned].any()
    A, a, a_t = fused_upload(L, x); zero = False if source != "INT64" else 0
    for flags in ("RC", "RSC", "R", "RS"):
        exp = fused_case(L, a, a_t, A, V, source, flags, ("vxm", "mxv"), False, "n=30015")
        if flags == "RC": assert exp.pres[[r] + pinned].all() and exp.val[[r] + pinned].all()
    a[r, int(cols[0])] = zero; a_t[int(cols[0]), r] = zero                                # the public API: GrB_Matrix_setElement
    x = x.copy(); x[L.rp[r]] = 0; A2 = MM.Mat(L.nrows, L.ncols, L.keys, x)
    for flags in ("RC", "RS"):
        exp = fused_case(L, a, a_t, A2, V, source, flags, ("vxm", "mxv"), False, "n=30015 after setElement")
        if flags == "RC": assert exp.pres[r] and (source == "ANY_PAIR" or not exp.val[r])


def test_fused_pull_with_code_bytes_past_one_round_of_the_grid(gpu):
    """n = 1 049 613 (> 256 workgroups x 1024 threads x 4 rows, the remainder no multiple of 256), >= 2^20 entries: code bytes on, a second, partial round."""
    L = fused_big(); V = level_vector(L.nrows, 511)
    V.pres[-3:] = False; c_last = int(L.ci[L.rp[L.nrows - 1]])                          # the last row is allowed under RC, and its first neighbour has a level
    assert c_last < L.nrows - 3
    V.pres[c_last] = True; V.val[c_last] = 1
    pinned = pin_level_vector(L, V)
    for source, flag_list in (("BOOL", ("RC", "RSC", "R", "RS")), ("INT64", ("RC",)), ("ANY_PAIR", ("RC",))):
        A, a, a_t = fused_upload(L, fused_values(L, source, 510))
        for flags in flag_list:
            exp = fused_case(L, a, a_t, A, V, source, flags, ("vxm", "mxv"), True, f"n={L.nrows}")
            if flags == "RC": assert exp.pres[256 * 1024 * 4:].any() and exp.pres[-1] and exp.val[pinned].all()      # the second round wrote entries
        if source == "BOOL":
            r = L.nrows - 1; c = int(L.ci[L.rp[r]])                                      # a head entry in the second round
            a[r, c] = False; a_t[c, r] = False
            x = A.vals.copy(); x[L.rp[r]] = False
            fused_case(L, a, a_t, MM.Mat(L.nrows, L.ncols, L.keys, x), V, source, "RC", ("vxm", "mxv"), True, "after setElement")


# ---- (e) push -------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def push_matrix(typ):
    P = push_pattern()
    vals = base_values(np.random.default_rng(600 + TYPES.index(typ) if typ in TYPES else 699), typ, P.nnz, "PLUS")
    if typ == "BOOL": vals = np.random.default_rng(601).random(P.nnz) < 0.8
    vals.setflags(write=False)
    return P, MM.Mat(P.nrows, P.ncols, P.keys, vals), upload(P, typ, vals)


def frontier(P, size, hubs, rng):
    """`size` positions: the first `hubs` rows of 4097 entries and no other of them, two rows of 4096, the rest among the short rows."""
    must = list(P.hubs[:hubs]) + (list(P.hubs[-2:]) if size >= hubs + 2 else [])
    rest = np.setdiff1d(np.arange(P.nrows), P.hubs)
    rng.shuffle(rest)
    return np.sort(np.concatenate([np.array(must[:size], np.int64), rest[: size - len(must[:size])]]))


def by_set_element(typ, n, at, x):
    u = gb.Vector.sparse(TYPE[typ], n)
    for i, v in zip(at.tolist(), x.tolist()): u[i] = v
    return u


@pytest.mark.parametrize("typ", ["INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64", "BOOL"])
def test_push_at_the_list_and_grid_edges(gpu, typ):
    """k_spmspv_push and k_spmspv_push_long, forced and by the automatic choice: 1, 64 and 65 operand entries built by setElement (the host list and the first
    size past it), 65 537 + 1000 entries (more than 16 384 workgroups x 4 waves); hub rows of 4096 (one wave) and 4097 entries (the long-row kernel), once 3
    of them (every block takes a slice of each) and once all 140 (one block per row); a valued mask, its complement, no mask; with and without accumulator."""
    P, A, a = push_matrix(typ); rng = np.random.default_rng(610 + len(typ)); At = MM.transpose(A)
    srs = ["LOR_LAND", "ANY_PAIR"] if typ == "BOOL" else ["PLUS_TIMES", "MIN_PLUS", "MAX_FIRST"]
    allow = rng.random(P.ncols) < 0.6
    k = 0
    for size, hubs, how in ((1, 1, "set"), (64, 3, "set"), (65, 3, "set"), (65537 + 1000, 3, "import"), (65537 + 1000, N_HUBS_4097, "import")):
        at = frontier(P, size, hubs, rng)
        assert len(at) == size and np.isin(P.hubs[:hubs], at).all() and int((P.lens[at] > 4096).sum()) == hubs and (hubs < 128) == (hubs != N_HUBS_4097)
        x = base_values(rng, typ, size, "PLUS") if typ != "BOOL" else rng.random(size) < 0.8
        U = VM.empty(P.nrows, typ); U.val[at] = x; U.pres[at] = True
        for sr in srs:
            add, mul = sr.split("_"); assert_exact_sums(typ, sr, At, U)
            for method in ("push", None) if size <= 65 else ("push",):
                mtyp, struct, comp = MASKS[k % len(MASKS)]
                mask = None if k % 4 == 3 else make_mask(allow, mtyp, struct, comp, rng)
                if mask is None: struct = comp = False
                accum = None if (k % 3 or add == "ANY") else ("LOR" if typ == "BOOL" else add); replace = bool(k % 2) and mask is not None
                W = operand(typ, P.ncols, "PLUS", True, np.zeros(0, np.int64), 620 + k) if (accum or not replace) else VM.empty(P.ncols, typ)
                u = by_set_element(typ, P.nrows, at, x) if how == "set" else dev(U)
                w = dev(W); m = None if mask is None else dev(mask)
                if method: os.environ["GRB_MI355X_SPMV"] = method
                try:
                    u.vxm(a, semiring=getattr(TYPE[typ], sr), out=w, mask=m, accum=getattr(TYPE[typ], accum) if accum else None, desc=desc_of(replace, struct, comp))
                finally:
                    os.environ.pop("GRB_MI355X_SPMV", None)
                plan = gb.last_kernel_plan(); what = f"push {typ}.{sr} size={size} hubs={hubs} method={method} mask={k % 4 != 3} struct={struct} comp={comp} replace={replace} accum={accum} plan={plan}"
                assert "k_spmspv_push<" in plan, what
                t = PM.product(add, mul, typ, At, U, flip=True)                             # (PM.vxm with the transpose made once)
                exp = VM.write_back(W, t, mask, struct, comp, replace, (accum, typ) if accum else None)
                check(w, exp, what)
                k += 1


def test_push_excludes_the_listed_positions_itself(gpu):
    """`w<!u, replace> = u lor.land A` with u a UINT8 vector built by setElement from 64 truthy entries, on a matrix of >= 2^20 entries (`excl_small`: no allow
    bytes are made, the kernels skip the listed positions and multiply by `true`).  The first hub row holds every listed position among its columns (k_spmspv_push_long)
    and a listed row of at most 14 entries holds one (k_spmspv_push), so each of them has a contribution and only the exclusion keeps it out.  With one listed value false the vector is no list of truthy entries any more: under
    the structural complement every listed position is still absent; under the valued complement the C API admits the position of the false value, and the
    result is the model's."""
    P, A, a = push_matrix("BOOL"); at = PUSH_LISTED
    for false_at in (None, 9):
        x = np.arange(1, 65, dtype=np.uint8)
        if false_at is not None: x[false_at] = 0
        U = VM.empty(P.nrows, "UINT8"); U.val[at] = x; U.pres[at] = True
        t = PM.product("LOR", "LAND", "BOOL", MM.transpose(A), U, flip=True)
        assert t.pres[at].all()                                                          # every listed position would get an entry
        for struct in (False, True):
            u = by_set_element("UINT8", P.nrows, at, x); w = dev(VM.Vec(np.ones(P.ncols, bool), np.ones(P.ncols, bool)))
            u.vxm(a, semiring=gb.BOOL.LOR_LAND, out=w, mask=u, desc=desc_of(True, struct, True))
            plan = gb.last_kernel_plan(); what = f"excl_small false_at={false_at} struct={struct} plan={plan}"
            assert "k_spmspv_push<" in plan, what
            exp = VM.write_back(VM.Vec(np.ones(P.ncols, bool), np.ones(P.ncols, bool)), t, U, struct, True, True)
            check(w, exp, what)
            _, p = w.to_dense_arrays()
            if false_at is None or struct: assert not p[at].any(), what
            else: assert not np.delete(p[at], false_at).any() and p[at[false_at]], what
            assert w.reduce_bool() is bool(np.any(exp.val[exp.pres])), what
