"""The O(n) kernels over the bitmap vector layout (grb_vecops.hip) and the deferred-chain kernel (grb_lazy_inst.hip, and its hipRTC twin of grb_chain_jit.cpp)
against the numpy model of tests/vector_model.py, at the sizes where their loops change shape, for every value width.

Every comparison is library against model on `to_dense_arrays()`: presence bytes as booleans, values bit-exact where present (one exception: FP64 POW, with the
operand ranges and the bound of test_math_library_operators).  Operands go in through `Vector.from_dense_array(values, typ, present=...)`: one copy, and the
entry count stays unknown, so counting runs.  Values follow helpers.rand_values (floating point on the 1/8 grid: exact in any order), with one entry in 64 at
the type's extremes for PLUS / MINUS / TIMES.

The sizes (from the launch lines of the kernels; the first test asserts them):
  N_MID = 524 288 + 256 * 37 + 5    past one round of grid_for (2048 workgroups of 256), no multiple of 4, 16 or 256: the plain grid-stride kernels
  N_BIG = 5 * 2 097 152 + 16 * 12 345 + 11 = 10 683 291: k_count's unrolled loop, single loop and byte tail all run; k_any_byte and k_vec_iseq take five sweeps
          and a part; k_assign_masked_bytes and k_copy2 wrap; the chain does at least five sweeps, n % 4 = 3, and some lane's next pack is the tail
  524 288, 2 097 152, 8 388 608     exact multiples: no tail at all
  63 64 65, 4095 4096 4097, 65 535 65 536    k_reduce_seq, the one-byte masked assign, its code bytes
  16 777 216 + 16 * 1000 + 5        k_init_small past one round of its 4096 workgroups

The element that decides a count, a MIN / MAX / LOR / LAND reduction or an `iseq` is planted in turn at `witnesses(n)`: position 0, the first position of the
second sweep (of each sweep length in use), the last full 16-byte group, inside the byte tail, position n - 1.

Routes the library does not report are taken under the conditions of grb_vector_ops.cpp: the one-pass k_vec_ewise_fused when a mask or an accumulator is given
and every type equals w's (unless GRB_MI355X_EWISE_FUSED=0); the three-kernel route k_allow / k_vec_ewise / k_vec_epilogue otherwise; the queued chain without
mask and accumulator for 4- and 8-byte types (asserted through GrBX_lazy_stats and GrBX_chain_jit_stats).  k_frontier_edges has no result a caller can
observe — only the direction choice of a product — and is left out."""
import ctypes as C
import functools

import numpy as np
import pytest

import matrix_model as MM
import vector_model as VM
import pygraphblas_amd as gb
from pygraphblas_amd import descriptor as D
from helpers import TYPE, rand_values
from test_matrix_kernels_at_size_gpu import desc_of, extremes, mask_values, same_bits

pytestmark = pytest.mark.gpu

TYPES = ["BOOL", "INT8", "UINT16", "INT32", "FP32", "INT64", "UINT64", "FP64"]
WIDTHS = ["INT8", "UINT16", "FP32", "INT64"]                 # one type per value width
NP = MM.NP
N_MID = 524288 + 256 * 37 + 5
N_BIG = 5 * 2097152 + 16 * 12345 + 11
N_INIT = 16777216 + 16 * 1000 + 5
PATTERNS = ["half", "sparse", "full", "full_unknown", "empty", "blocks", "edges"]


def test_the_sizes_are_what_the_kernels_need(gpu):
    """The constants are those of the launch lines: grid_for caps at 2048 workgroups of 256; k_count runs 128 workgroups of 16 B per lane, unrolled four times;
    k_any_byte 512 and k_vec_iseq 2048 workgroups of 16 B resp. 4 positions per lane; k_assign_masked_bytes 2048 of 16; k_init_small 4096 of 16; the chain at
    most CUs x 8 resident workgroups of 256 lanes of 4 positions."""
    assert N_BIG == 10683291 and N_MID == 533765
    assert N_MID > 2048 * 256 and N_MID % 4 and N_MID % 16 and N_MID % 256
    T = 128 * 256; n16 = N_BIG // 16
    assert n16 > 4 * T and (n16 - (n16 // (4 * T)) * 4 * T) % T != 0 and 0 < n16 % (4 * T) and N_BIG % 16 == 11       # unrolled loop, single loop, byte tail
    assert N_BIG // (512 * 256 * 16) == 5 and N_BIG // (2048 * 256 * 4) == 5 and N_BIG % (2048 * 256 * 4)                # five sweeps and a part
    assert N_BIG > 2048 * 256 * 16 and 2 * N_BIG // 16 > info_cus() * 8 * 256                                            # the masked assign and the copy wrap
    assert N_BIG // (info_cus() * 8 * 256 * 4) >= 5 and N_BIG % 4 == 3 and N_BIG - 3 >= info_cus() * 8 * 256 * 4       # the chain: sweeps, tail, a next pack that is the tail
    assert N_INIT > 4096 * 256 * 16 and N_INIT % 16 == 5
    for n in (N_MID, N_BIG):
        w = witnesses(n)
        assert w[0] == 0 and w[-1] == n - 1 and any(n // 16 * 16 <= p < n - 1 for p in w) and (n // 16 * 16 - 1) in w and any(0 < p <= 2097152 for p in w)


def info_cus():
    return int(gb.device_info()["compute_units"] or 256)


def witnesses(n):
    """Position 0, the first position of the second sweep for every sweep length in use, the end of the last full 16-byte group, the middle of the byte tail,
    the last position."""
    tail0 = n // 16 * 16
    ps = {0, n - 1, tail0 - 1, tail0 + (n - tail0) // 2}
    ps |= {s for s in (2048 * 256, 128 * 256 * 16, 2048 * 256 * 4, 2048 * 256 * 16) if s < n}
    return sorted(p for p in ps if 0 <= p < n)


# ---- presence patterns and operands, built once -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def presence(name, n, variant=0):
    """A read-only bool array; `full` is all ones and uploaded without presence bytes, `full_unknown` is all ones passed explicitly."""
    rng = np.random.default_rng([sum(map(ord, name)), n % 1000003, variant])
    if name == "half": p = rng.random(n) < 0.5
    elif name == "sparse": p = rng.random(n) < 0.001
    elif name in ("full", "full_unknown"): p = np.ones(n, bool)
    elif name == "empty": p = np.zeros(n, bool)
    elif name == "blocks":                                       # alternating runs of 16, 64 and 256: whole 16-byte loads all zero or all one
        runs = np.tile(np.array([16, 16, 64, 64, 256, 256]), n // 672 + 3); on = np.tile(np.array([True, False]), len(runs) // 2)
        p = np.repeat(on, runs)[variant % 42 * 16:][:n].copy()
    elif name == "edges":
        p = np.zeros(n, bool); p[[q for q in (0, 15, 16, 524287, 524288, n - 17, n - 16, n - 1) if 0 <= q < n]] = True
    else: raise ValueError(name)
    p.setflags(write=False)
    return p


def values(rng, typ, n, extreme=False):
    x = rand_values(rng, typ, n)
    if extreme and n and typ != "BOOL":
        at = rng.random(n) < 1 / 64
        x[at] = rng.choice(extremes(typ), size=int(at.sum()))
    return x


@functools.lru_cache(maxsize=None)
def operand(typ, n, pat, seed=0, extreme=False):
    """A model vector nobody writes to: a value at EVERY position (what lies behind a hole must not matter), the pattern `pat`."""
    x = values(np.random.default_rng([seed, TYPES.index(typ) if typ in TYPES else 99, n % 1000003]), typ, n, extreme)
    x.setflags(write=False)
    return VM.Vec(x, presence(pat, n, seed))


def dev(v, full=False):
    """One copy into HBM; the entry count is unknown afterwards unless `full` (no presence bytes passed: every position holds an entry)."""
    assert not full or v.pres.all()
    return gb.Vector.from_dense_array(v.val, TYPE[v.typ], present=None if full else v.pres.view(np.uint8))


def dev_of(typ, n, pat, seed=0, extreme=False):
    v = operand(typ, n, pat, seed, extreme)
    return v, dev(v, full=pat == "full")


def check(w, exp, what):
    assert w.type.__name__ == exp.typ and w.size == exp.n, (what, w, exp.typ, exp.n)
    x, p = w.to_dense_arrays(); p = p != 0
    if not np.array_equal(p, exp.pres):
        q = np.flatnonzero(p != exp.pres); raise AssertionError(f"{what}: the pattern differs at {len(q)} positions, first {q[:6].tolist()} (n = {exp.n}): got {p[q[:6]]}")
    ok = same_bits(x[p], exp.val[p])
    if not ok.all():
        q = np.flatnonzero(p)[~ok]; raise AssertionError(f"{what}: {len(q)} values differ, first at {q[:6].tolist()} (n = {exp.n}): got {x[q[:6]]} expected {exp.val[q[:6]]}")


def planted(v, at, val=None, present=True):
    """A copy of the model vector with one position changed."""
    x = v.val.copy(); p = v.pres.copy()
    if val is not None: x[at] = val
    p[at] = present
    return VM.Vec(x, p)


def lazy_stats():
    a = [C.c_uint64(0) for _ in range(4)]
    assert gb.lib.GrBX_lazy_stats(*[C.byref(x) for x in a]) == 0
    return dict(zip(("chains", "nodes", "fills_folded", "reduces_fused"), [x.value for x in a]))


def jit_stats():
    a = [C.c_uint64(0), C.c_uint64(0)]
    assert gb.lib.GrBX_chain_jit_stats(C.byref(a[0]), C.byref(a[1])) == 0
    return a[0].value, a[1].value


# ---- counting and copying ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_BIG, 2097152, N_MID, 17, 16, 15])
def test_nvals_after_import(gpu, n):
    """k_count over every pattern, then one entry alone and one hole alone at every witness position: a dropped tail, sweep or unrolled step miscounts one."""
    zeros = np.zeros(n, np.int8)
    for pat in PATTERNS:
        p = presence(pat, n)
        v = gb.Vector.from_dense_array(zeros, gb.INT8, present=None if pat == "full" else p.view(np.uint8))
        assert v.nvals == int(p.sum()), (pat, n)
    for at in witnesses(n):
        one = np.zeros(n, np.uint8); one[at] = 1
        assert gb.Vector.from_dense_array(zeros, gb.INT8, present=one).nvals == 1, (at, n)
        assert gb.Vector.from_dense_array(zeros, gb.INT8, present=1 - one).nvals == n - 1, (at, n)


@pytest.mark.parametrize("typ", WIDTHS + ["BOOL", "FP64"])
def test_dup_and_resize(gpu, typ):
    """k_copy2: values and presence bytes in one launch, the byte tails of both arrays (n * size % 16 and n % 16), past one round of its grid at N_BIG; resize
    copies the common prefix with the same kernel: shorter and longer across a 16-byte boundary."""
    for n, pat in ((N_BIG, "half"), (N_MID, "blocks"), (8388608, "half")):
        V, v = dev_of(typ, n, pat, seed=1)
        w = v.dup()
        assert w.nvals == V.nvals
        check(w, V, f"dup {typ} n={n}")
    V, v = dev_of(typ, N_MID, "half", seed=2)
    for m in (N_MID - 2, N_MID // 16 * 16, N_MID - 21, 4097):                   # inside the byte tail, to the 16-byte boundary, across it, far down
        v.resize(m); V = VM.Vec(V.val[:m], V.pres[:m])
        assert v.nvals == V.nvals
        check(v, V, f"resize to {m} {typ}")
    v.resize(4097 + 40); V = VM.Vec(np.concatenate([V.val, np.zeros(40, V.val.dtype)]), np.concatenate([V.pres, np.zeros(40, bool)]))
    assert v.nvals == V.nvals
    check(v, V, f"resize longer {typ}")


@pytest.mark.parametrize("byte", [0xFF, 0x80, 0x02])
def test_any_non_zero_presence_byte_is_an_entry(gpu, byte):
    """The contract of GrBX_Vector_import_Bitmap (include/grb_mi355x.h): a presence byte that is not zero is an entry, whatever its bits.  nvals, iseq,
    reduce_bool, an eWise result and the exported bytes all agree.  (k_count looked at bit 0 only in its 16-byte loads: nvals of such a vector was the count of
    its last n % 16 positions for 0x80 and 0x02; smallest n that fails: 16.)"""
    for n in (N_BIG, 16, 37):
        U = operand("BOOL", n, "half", seed=3); Vv = operand("BOOL", n, "blocks", seed=4)
        raw = np.where(U.pres, np.uint8(byte), np.uint8(0))
        u = gb.Vector.from_dense_array(U.val, gb.BOOL, present=raw); u01 = dev(U); v = dev(Vv)
        assert u.nvals == U.nvals, (n, byte)
        assert u.iseq(u01) and u01.iseq(u), (n, byte)
        at = int(np.flatnonzero(U.pres[1:] & ~U.pres[:-1])[-1]) + 1                  # the last entry behind a hole moves into the hole: the same count
        moved = planted(planted(U, at, present=False), at - 1, U.val[at], present=True)
        assert moved.nvals == U.nvals and not u.iseq(dev(moved)), (n, byte)
        x, p = u.to_dense_arrays()
        assert np.array_equal(p != 0, U.pres) and np.array_equal(x[U.pres], U.val[U.pres]), (n, byte)
        check(u.eadd(v, gb.BOOL.LXOR), VM.ewise("LXOR", "BOOL", U, Vv, True), f"eadd LXOR with presence bytes {byte:#x} n={n}")
        check(u.emult(v, gb.BOOL.LOR), VM.ewise("LOR", "BOOL", U, Vv, False), f"emult LOR with presence bytes {byte:#x} n={n}")
        for w_at in witnesses(n):                                                  # the one true value, present under the odd byte
            x = np.zeros(n, np.bool_); x[w_at] = True; pr = raw.copy(); pr[w_at] = byte
            t = gb.Vector.from_dense_array(x, gb.BOOL, present=pr)
            assert t.reduce_bool() is True and t.reduce_bool(gb.BOOL.LAND_MONOID) is (int((pr != 0).sum()) == 1), (n, byte, w_at)
            pr[w_at] = 0
            assert gb.Vector.from_dense_array(x, gb.BOOL, present=pr).reduce_bool() is False, (n, byte, w_at)


# ---- reductions ----------------------------------------------------------------------------------------------------------------------------------------------------
def monoids(typ):
    if typ == "BOOL": return ["LOR", "LAND", "LXOR", "EQ", "LXNOR"]
    return ["PLUS", "TIMES", "MIN", "MAX"] + (["BOR", "BAND", "BXOR", "BXNOR"] if typ[0] == "U" else [])


def reduce_values_for(rng, typ, mon, n):
    """Values under which the monoid's result is the same in every order, and under which it changes when any one entry is left out or taken twice
    (PLUS / TIMES); the conditions are asserted where the values are made."""
    if typ == "BOOL": return rng.random(n) < (0.999 if mon in ("LAND",) else 0.5)
    fp = typ.startswith("FP")
    if mon == "PLUS":
        if typ == "FP32":                                        # every partial sum in any order is a multiple of 1/8 below 2^24 / 8: exact
            x = rng.choice(np.array([-0.125, 0.125, 0.125], np.float32), size=n); assert n < 1 << 24 and set(np.unique(x).tolist()) <= {-0.125, 0.125}
            return x
        x = values(rng, typ, n, extreme=not fp)
        return np.where(x == 0, NP[typ](1), x)                 # FP64 on the 1/8 grid: |sum| < 2^53 / 8; integers wrap, which is order-free
    if mon == "TIMES":
        if fp:                                                   # +-1 with at most 40 factors of 2 and of 1/2: every partial product is +-2^k, |k| <= 40 — exact
            x = -np.ones(n, NP[typ]); at = rng.choice(n, size=min(80, n // 2), replace=False); x[at[: len(at) // 2]] = 2; x[at[len(at) // 2:]] = -0.5
            assert (np.abs(x) == 2).sum() <= 40 and (np.abs(x) == 0.5).sum() <= 40
            return x
        odd = np.array([3, 5, 7, 11, 13] if typ[0] == "U" else [3, -3, 5, -5, 7], NP[typ])      # odd factors: invertible modulo 2^k, none of them 1
        return rng.choice(odd, size=n)
    if mon in ("MIN", "MAX"):
        if fp: return (rng.integers(10 * 8, 40 * 8, n) / 8.0).astype(NP[typ])
        return rng.integers(10, 40, n, endpoint=True).astype(NP[typ])
    return rng.integers(0, np.iinfo(NP[typ]).max, n, endpoint=True, dtype=NP[typ])      # the bitwise monoids


def lib_reduce(v, typ, mon):
    m = getattr(TYPE[typ], mon + "_MONOID")
    if typ == "BOOL": return np.bool_(v.reduce_bool(m))
    if typ.startswith("FP"): return NP[typ](v.reduce_float(m))
    return np.int64(v.reduce_int(m))


def assert_reduces(v, V, typ, mon, what):
    exp = VM.reduce(mon, typ, V); got = lib_reduce(v, typ, mon)
    if not typ.startswith("FP") and typ != "BOOL": exp = MM.cast(exp, "INT64")      # (the typed entry point hands an integer result over as INT64)
    assert same_bits(np.array([got]), np.array([exp])).all(), f"reduce {mon} {typ} {what}: got {got!r} expected {exp!r}"


@pytest.mark.parametrize("typ", TYPES)
def test_every_monoid_at_n_mid_and_around_the_sequential_threshold(gpu, typ):
    """Every monoid of the type through k_reduce at N_MID (522 workgroups of four positions per lane, then the one-workgroup second level over their partials;
    the second round of the grid is the at-size test below), k_reduce_seq at n = 63 and 64 (one lane, index order) and k_reduce again at 65."""
    rng = np.random.default_rng(TYPES.index(typ) + 20)
    for n in (N_MID, 63, 64, 65):
        for pat in ("half", "full", "edges") if n == N_MID else ("half", "full"):
            for mon in monoids(typ):
                p = presence(pat, n)
                V = VM.Vec(reduce_values_for(rng, typ, mon, n), p)
                assert_reduces(dev(V, full=pat == "full"), V, typ, mon, f"n={n} {pat}")
        assert_reduces(dev(VM.empty(n, typ)), VM.empty(n, typ), typ, monoids(typ)[0], f"n={n} empty")
    V = VM.Vec(reduce_values_for(rng, typ, "MIN" if typ != "BOOL" else "LOR", N_MID), presence("half", N_MID))
    got = lib_reduce(dev(V), typ, "ANY")                                           # ANY: some present value
    assert got in MM.cast(V.val[V.pres], "INT64" if not typ.startswith("FP") and typ != "BOOL" else typ)


@pytest.mark.parametrize("typ", WIDTHS + ["FP64"])
def test_reductions_at_n_big(gpu, typ):
    """PLUS, TIMES, MIN, MAX past the second round of k_reduce's 2048 workgroups (2048 partials into the one-workgroup second level: n >= 2 097 152), on `half`
    and on the exact multiple 8 388 608 without presence bytes.  PLUS and TIMES change when any one entry is dropped or taken twice; for MIN and MAX the
    deciding entry is planted at each witness position in turn."""
    rng = np.random.default_rng(WIDTHS.index(typ) + 40 if typ in WIDTHS else 49)
    for n, pat in ((N_BIG, "half"), (8388608, "full")):
        for mon in ("PLUS", "TIMES"):
            V = VM.Vec(reduce_values_for(rng, typ, mon, n), presence(pat, n))
            assert_reduces(dev(V, full=pat == "full"), V, typ, mon, f"n={n} {pat}")
    base = VM.Vec(reduce_values_for(rng, typ, "MIN", N_BIG), presence("half", N_BIG))
    ws = witnesses(N_BIG)
    for k, at in enumerate(ws):                                                    # the minimum at one witness, the maximum at the next one round
        hi = ws[(k + 1) % len(ws)]
        V = planted(planted(base, at, NP[typ](3)), hi, NP[typ](45))
        v = dev(V)
        assert_reduces(v, V, typ, "MIN", f"minimum planted at {at}"); assert_reduces(v, V, typ, "MAX", f"maximum planted at {hi}")
        assert VM.reduce("MIN", typ, V) == 3 and VM.reduce("MAX", typ, V) == 45


@pytest.mark.parametrize("n", [N_BIG, N_MID, 2097152])
def test_fp32_reduced_in_fp64(gpu, n):
    """`reduce_float` of an FP32 vector: k_reduce_f32_f64 widens on the fly (PLUS, MIN, MAX, TIMES of FP64 over FP32 values)."""
    rng = np.random.default_rng(n % 1000)
    for mon in ("PLUS", "TIMES", "MIN", "MAX"):
        for pat in ("half", "full"):
            x = reduce_values_for(rng, "FP32", mon, n) if mon != "PLUS" else values(rng, "FP32", n)      # (PLUS: the 1/8 grid, |sum| < 2^53 / 8 in FP64)
            V = VM.Vec(np.where(x == 0, np.float32(0.125), x), presence(pat, n))
            exp = VM.reduce(mon, "FP64", V)
            got = dev(V, full=pat == "full").reduce_float(getattr(gb.FP64, mon + "_MONOID")) if mon != "PLUS" else dev(V, full=pat == "full").reduce_float()
            assert got == exp, (mon, pat, n, got, exp)
    base = VM.Vec(reduce_values_for(rng, "FP32", "MIN", n), presence("half", n))
    for at in witnesses(n):
        V = planted(base, at, np.float32(3)); assert dev(V).reduce_float(gb.FP64.MIN_MONOID) == 3.0, at


@pytest.mark.parametrize("n", [N_BIG, 2097152, N_MID])
def test_bool_lor_and_land_with_one_deciding_byte(gpu, n):
    """k_any_byte: every present value false but one (LOR), true but one (LAND), the one at each witness position; true resp. false values behind holes."""
    p = presence("half", n); rng = np.random.default_rng(5)
    for at in witnesses(n):
        for want in (True, False):                                                 # want: the deciding value; LOR looks for a true one, LAND for a false one
            x = np.where(p, not want, rng.random(n) < 0.5); pr = p.copy()
            V0 = VM.Vec(x, pr); V1 = planted(V0, at, want)
            for V in (V0, V1) if at == 0 else (V1,):
                v = dev(V)
                assert v.reduce_bool() is bool(VM.reduce("LOR", "BOOL", V)) and v.reduce_bool(gb.BOOL.LAND_MONOID) is bool(VM.reduce("LAND", "BOOL", V)), (n, at, want)
            assert bool(VM.reduce("LOR" if want else "LAND", "BOOL", V1)) is want and bool(VM.reduce("LOR" if want else "LAND", "BOOL", V0)) is (not want)


@pytest.mark.parametrize("typ", ["FP32", "FP64"])
def test_fp_min_max_with_nan_and_without_entries(gpu, typ):
    """Start from the first value: every value NaN gives NaN, one number among NaNs (in the byte tail) gives the number, no entry gives the identity."""
    for n in (N_BIG, N_MID, 64, 65):
        p = presence("half", n); nan = np.full(n, np.nan, NP[typ])
        for mon in ("MIN", "MAX"):
            V = VM.Vec(nan, p); assert_reduces(dev(V), V, typ, mon, f"all NaN n={n}")
            assert np.isnan(VM.reduce(mon, typ, V))
            V = planted(V, n - 2, NP[typ](-2.5)); assert_reduces(dev(V), V, typ, mon, f"one number in the tail n={n}")
            assert VM.reduce(mon, typ, V) == -2.5
            V = VM.Vec(nan, presence("empty", n)); assert_reduces(dev(V), V, typ, mon, f"no entry n={n}")
            assert VM.reduce(mon, typ, V) == (np.inf if mon == "MIN" else -np.inf)


# ---- iseq ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", WIDTHS + ["BOOL", "FP64"])
def test_iseq(gpu, typ):
    """k_vec_iseq: equal vectors; one differing value and one moved entry (the same count) at each witness position; NaN differs from NaN and -0.0 equals 0.0."""
    for n in (N_BIG, N_MID, 2097152):
        if n != N_BIG and typ in ("BOOL", "FP64"): continue
        U = operand(typ, n, "half", seed=6); u = dev(U)
        assert u.iseq(dev(U)) is True and VM.iseq(U, U.copy())
        for at in witnesses(n):
            U1 = planted(U, at); u1 = dev(U1)                                      # an entry at the witness position in both
            other = NP[typ](not U1.val[at]) if typ == "BOOL" else NP[typ](U1.val[at] + NP[typ](1))
            D1 = planted(U1, at, other)
            nb = at - 1 if at else 1
            M1 = planted(planted(U1, nb, present=False), at, present=True); M2 = planted(planted(U1, nb, U1.val[at], present=True), at, present=False)
            assert u1.iseq(dev(D1)) is False and not VM.iseq(U1, D1), (typ, n, at, "value")
            m1, m2 = dev(M1), dev(M2)
            assert M1.nvals == M2.nvals and m1.iseq(m2) is False and not VM.iseq(M1, M2), (typ, n, at, "moved entry")
            if typ == "FP32" or (typ == "FP64" and at in (0, n - 1)):
                Z0, Z1, Nn = planted(U1, at, NP[typ](0.0)), planted(U1, at, NP[typ](-0.0)), planted(U1, at, NP[typ](np.nan))
                assert dev(Z0).iseq(dev(Z1)) is True and VM.iseq(Z0, Z1) and dev(Nn).iseq(dev(Nn)) is False and not VM.iseq(Nn, Nn.copy()), (typ, n, at)


# ---- element-wise, on four routes ---------------------------------------------------------------------------------------------------------------------------------
EW_OPS = ["PLUS", "MINUS", "TIMES", "MIN", "DIV", "ISGT"]


def ewise_cases(route, seed, count):
    """Pairwise, not the full product: a seeded generator draws `count` combinations; every value of every factor occurs (asserted)."""
    rng = np.random.default_rng(seed); cases = []
    chain = route in ("interpreter", "compiled")
    for k in range(count):
        typ = str(rng.choice(["FP32", "FP64", "INT32", "INT64"] if chain else ["INT8", "UINT16", "BOOL"] if route == "narrow" else TYPES[1:]))
        mask = "none" if chain else str(rng.choice(["none", "valued", "structural", "complemented"]))
        accum = None if chain else (None, "PLUS", "SECOND")[int(rng.integers(0, 3))]
        if route == "one pass" and mask == "none" and accum is None: accum = "PLUS"
        alias = str(rng.choice(["none", "u", "v"] + (["mask"] if mask != "none" else [])))
        cases.append(dict(typ=typ, op=EW_OPS[k % len(EW_OPS)], union=bool((k // len(EW_OPS) + k) % 2), mask=mask, replace=bool(rng.integers(0, 2)) and mask != "none", accum=accum, alias=alias))
    assert {c["op"] for c in cases} == set(EW_OPS) and {c["union"] for c in cases} == {True, False}
    return cases


def run_ewise_case(c, n, what):
    typ, op = c["typ"], c["op"]; T = TYPE[typ]
    U = operand(typ, n, "half", seed=7, extreme=op in ("PLUS", "MINUS", "TIMES")); V = operand(typ, n, "blocks", seed=8, extreme=op in ("PLUS", "MINUS", "TIMES"))
    if op == "DIV" and typ != "BOOL": V = VM.Vec(np.where(V.val == 0, NP[typ](3), V.val), V.pres)      # non-zero divisors
    W = operand(typ, n, "half", seed=9)
    mt = ("BOOL", "INT8", "FP32", "INT64")[sum(map(ord, op)) % 4]
    M = None if c["mask"] == "none" else VM.Vec(mask_values(np.random.default_rng(10), mt, n), presence("half", n, 11))
    u, v = dev(U), dev(V)
    m = None if M is None else dev(M)
    if c["alias"] == "u": w, W = u, U
    elif c["alias"] == "v": w, W = v, V
    elif c["alias"] == "mask" and M is not None and mt == typ: w, W = m, M
    else: w = dev(W)
    (u.eadd if c["union"] else u.emult)(v, getattr(T, op), out=w, mask=m, accum=getattr(T, c["accum"]) if c["accum"] else None,
                                        desc=desc_of(c["replace"], c["mask"] == "structural", c["mask"] == "complemented"))
    exp = VM.write_back(W, VM.ewise(op, typ, U, V, c["union"]), M, c["mask"] == "structural", c["mask"] == "complemented", c["replace"], (c["accum"], typ) if c["accum"] else None)
    check(w, exp, f"{what}: {c}")
    if w is not u: check(u, U, f"{what}: the first operand is unchanged")


def test_ewise_through_the_chain_interpreter(gpu, monkeypatch):
    """GRB_MI355X_CHAIN_JIT=0: every queued eWise runs through k_vec_chain as compiled ahead of time (the interpreter, and SPEC 2 for an FP `x / y` on the intersection)."""
    monkeypatch.setenv("GRB_MI355X_CHAIN_JIT", "0")
    s0 = lazy_stats(); j0 = jit_stats()
    for c in ewise_cases("interpreter", 31, 12): run_ewise_case(c, N_MID, "interpreter")
    assert lazy_stats()["chains"] - s0["chains"] >= 12 and jit_stats() == j0


def test_ewise_through_the_compiled_chains(gpu, monkeypatch, tmp_path):
    """The default setting with an empty code-object cache: a chain is compiled by hipRTC at its second appearance; each case runs three times, the second and
    third through the compiled kernel."""
    monkeypatch.delenv("GRB_MI355X_CHAIN_JIT", raising=False); monkeypatch.setenv("GRB_MI355X_CACHE_DIR", str(tmp_path))
    c0, l0 = jit_stats()
    cases = ewise_cases("compiled", 32, 6)
    for c in cases:
        for appearance in range(3): run_ewise_case(c, N_MID, f"compiled, appearance {appearance + 1}")
    c1, l1 = jit_stats()
    assert c1 > c0 and l1 - l0 >= len(cases), (c0, c1, l0, l1)


def test_ewise_in_one_pass(gpu, monkeypatch):
    """k_vec_ewise_fused: a mask or an accumulator, every type w's own (grb_vector_ops.cpp: `same && (mask || accum)`).  A mask of another type is read in place."""
    monkeypatch.delenv("GRB_MI355X_EWISE_FUSED", raising=False)
    for c in ewise_cases("one pass", 33, 18): run_ewise_case(c, N_MID, "one pass")


def test_ewise_on_the_three_kernel_route(gpu, monkeypatch):
    """k_allow, k_vec_ewise, k_vec_epilogue: GRB_MI355X_EWISE_FUSED=0 with masks and accumulators, the 1- and 2-byte types without either (no chain kernel for them),
    and operands of another type than the operator's (`cast=`: k_cast on the way in and out)."""
    monkeypatch.setenv("GRB_MI355X_EWISE_FUSED", "0")
    for c in ewise_cases("general", 34, 12): run_ewise_case(c, N_MID, "EWISE_FUSED=0")
    monkeypatch.delenv("GRB_MI355X_EWISE_FUSED", raising=False)
    for c in ewise_cases("narrow", 35, 6):
        c.update(mask="none", accum=None, replace=False, alias="none" if c["alias"] == "mask" else c["alias"]); run_ewise_case(c, N_MID, "1- and 2-byte types")
    U = operand("INT8", N_MID, "half", seed=7, extreme=True); V = operand("INT8", N_MID, "blocks", seed=8, extreme=True)
    for op, otyp, union in (("PLUS", "FP64", True), ("TIMES", "INT32", False), ("MINUS", "INT64", True)):
        got = (dev(U).eadd if union else dev(U).emult)(dev(V), getattr(TYPE[otyp], op), cast=TYPE[otyp])
        check(got, VM.ewise(op, otyp, U, V, union), f"INT8 operands under {otyp}.{op}")


def test_ewise_pow_within_the_math_library_bound(gpu):
    """FP64 POW (MATH = true instantiations; never queued): bases in [0.5, 2.5], exponents in [0, 0.5], rtol = 1e-12 against np.power as in
    test_math_library_operators — the one comparison here that is not bit-exact; the pattern and the passed-through entries are."""
    rng = np.random.default_rng(12); n = N_MID
    U = VM.Vec(0.5 + 2.0 * rng.random(n), presence("half", n, 12)); V = VM.Vec(0.5 * rng.random(n), presence("blocks", n, 13))
    for union in (True, False):
        for accum in (None, "PLUS"):                                               # (with an accumulator: the one-pass kernel)
            W = VM.Vec(rng.random(n), presence("half", n, 14)); w = dev(W)
            (dev(U).eadd if union else dev(U).emult)(dev(V), gb.FP64.POW, out=w, accum=gb.FP64.PLUS if accum else None)
            exp = VM.write_back(W, VM.ewise("POW", "FP64", U, V, union), accum=("PLUS", "FP64") if accum else None)
            x, p = w.to_dense_arrays(); both = U.pres & V.pres
            assert np.array_equal(p != 0, exp.pres) and np.allclose(x[both], exp.val[both], rtol=1e-12, atol=0.0), (union, accum)
            rest = exp.pres & ~both
            assert np.array_equal(x[rest], exp.val[rest]), (union, accum)


# ---- the chain at N_BIG --------------------------------------------------------------------------------------------------------------------------------------------
def chain_programs(typ):
    """(name, stored operands, steps): a step is (kind, operator, a, b): a / b index the operands, "t" is the result of the step before, a number is a bound scalar."""
    return [("x - y", 2, [("eadd", "MINUS", 0, 1)]),
            ("reduce(+, abs(x - y)): SPEC 1 on full operands", 2, [("eadd", "MINUS", 0, 1), ("apply", "ABS", "t", None)]),
            ("x / y on the intersection: SPEC 2", 2, [("emult", "DIV", 0, 1)]),
            ("-((x + y) * z)", 3, [("eadd", "PLUS", 0, 1), ("emult", "TIMES", "t", 2), ("apply", "AINV", "t", None)]),
            ("max(min(x, y) + z) * 2, w)", 4, [("eadd", "MIN", 0, 1), ("eadd", "PLUS", "t", 2), ("bind2nd", "TIMES", "t", 2), ("eadd", "MAX", "t", 3)])]


def chain_operands(typ, n, pat):
    """The four stored operands (the second one without zeros: it is a divisor), uploaded once for all the chains of a case."""
    Vs = [operand(typ, n, "full" if pat == "full_unknown" else pat, seed=20 + k) for k in range(4)]
    Vs[1] = VM.Vec(np.where(Vs[1].val == 0, NP[typ](3), Vs[1].val), Vs[1].pres)
    ds = [dev(V, full=pat == "full") for V in Vs]
    if pat == "full_unknown": assert all(d.nvals == n for d in ds)               # (counted: from here on the library knows they are full, as after a product)
    return Vs, ds


def run_chain(typ, Vs, ds, prog, fused_variants, what):
    """The chain once per variant of `fused_variants`: None (the result is looked at), "in type" / "widened" (first reduced — the reduction fused into the
    chain's kernel — then looked at).  PLUS where every partial sum is exact (integers wrap; FP64 on the 1/64 grid; FP32 widened into FP64), MAX for FP32 in
    its own type and for the quotients of `x / y`."""
    name, nops, steps = prog; T = TYPE[typ]; n = Vs[0].n; Tm = None
    fp = typ.startswith("FP")
    for kind, op, a, b in steps:                                                   # the model, once
        A = Tm if a == "t" else Vs[a]
        if kind in ("eadd", "emult"): Tm = VM.ewise(op, typ, A, Tm if b == "t" else Vs[b], kind == "eadd")
        elif kind == "apply": Tm = VM.apply(op, typ, A)
        else: Tm = VM.bind2nd(op, typ, A, b)
    for fused in fused_variants:
        t = gb.Vector.sparse(T, n); s0 = lazy_stats()
        for kind, op, a, b in steps:
            da = t if a == "t" else ds[a]
            if kind in ("eadd", "emult"): (da.eadd if kind == "eadd" else da.emult)(t if b == "t" else ds[b], getattr(T, op), out=t)
            elif kind == "apply": da.apply(getattr(T, op), out=t)
            else: da.apply_second(getattr(T, op), b, out=t)
        if fused:
            mon = "MAX" if fp and (any(st[1] == "DIV" for st in steps) or (typ == "FP32" and fused == "in type")) else "PLUS"
            if fp:
                mt = "FP64" if fused == "widened" else typ
                got = t.reduce_float(getattr(TYPE[mt], mon + "_MONOID")); exp = VM.reduce(mon, mt, Tm)
            else:
                got = t.reduce_int(T.PLUS_MONOID); exp = MM.cast(VM.reduce("PLUS", typ, Tm), "INT64")
            assert lazy_stats()["reduces_fused"] == s0["reduces_fused"] + 1, (what, name, fused)
            assert got == exp, f"{what}: {fused} reduction fused into {name}: got {got!r} expected {exp!r}"
        check(t, Tm, f"{what}: {name} (fused reduction: {fused})")
        s2 = lazy_stats()
        assert s2["nodes"] - s0["nodes"] == len(steps) and s2["chains"] > s0["chains"], (what, name, fused, s0, s2)


def chain_case(typ, n, pat, what, programs=None):
    Vs, ds = chain_operands(typ, n, pat)
    for prog in programs or chain_programs(typ):
        run_chain(typ, Vs, ds, prog, (None, "widened" if typ == "FP32" else "in type") + (("in type",) if typ == "FP32" and prog[1] == 2 else ()), what)
    for d, V in zip(ds, Vs): check(d, V, f"{what}: a stored operand is unchanged")


@pytest.mark.parametrize("pat", ["half", "full", "full_unknown", "half, no tail"])
@pytest.mark.parametrize("typ", ["FP32", "FP64", "INT32", "INT64"])
def test_chains_at_n_big_ahead_of_time(gpu, monkeypatch, typ, pat):
    """GRB_MI355X_CHAIN_JIT=0: the interpreter kernel and the two ahead-of-time shapes, at N_BIG (n % 4 = 3: the `nv < VEC` loads and stores, a lane whose next
    pack is the tail reloads its own) and at 2 * 2 097 152 (no tail), each chain with and without the reduction fused into it."""
    monkeypatch.setenv("GRB_MI355X_CHAIN_JIT", "0")
    j0 = jit_stats()
    if pat == "half, no tail": chain_case(typ, 2 * 2097152, "half", f"{typ} n=4194304 half")
    else: chain_case(typ, N_BIG, pat, f"{typ} n={N_BIG} {pat}")
    assert jit_stats() == j0


@pytest.mark.parametrize("typ", ["FP32", "INT64"])
def test_chains_at_n_big_compiled(gpu, monkeypatch, tmp_path, typ):
    """GRB_MI355X_CHAIN_JIT=2: the same chains through the kernels hipRTC compiles for exactly their steps, at their first appearance."""
    monkeypatch.setenv("GRB_MI355X_CHAIN_JIT", "2"); monkeypatch.setenv("GRB_MI355X_CACHE_DIR", str(tmp_path))
    c0, l0 = jit_stats()
    chain_case(typ, N_BIG, "half", f"compiled {typ}")
    c1, l1 = jit_stats()
    assert c1 > c0 and l1 - l0 >= 2 * len(chain_programs(typ)), (c0, c1, l0, l1)


@pytest.mark.parametrize("n", [3, 4, 5])
def test_chains_on_three_four_and_five_positions(gpu, monkeypatch, n):
    monkeypatch.setenv("GRB_MI355X_CHAIN_JIT", "0")
    for typ in ("FP32", "FP64", "INT32", "INT64"):
        for pat in ("half", "full"):
            chain_case(typ, n, pat, f"{typ} n={n} {pat}")


# ---- apply, select, cast ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_apply_select_at_n_mid(gpu, typ):
    """k_vec_apply (unary; a bound first and second scalar) once into an empty output — the chain for 4- and 8-byte types — and once accumulated under a valued
    mask (k_allow, k_vec_apply, k_vec_epilogue); k_select_value: all twelve value selects with a zero, a positive and a negative thunk."""
    T = TYPE[typ]; n = N_MID; s = True if typ == "BOOL" else 5
    U = operand(typ, n, "half", seed=30, extreme=typ != "BOOL")
    if typ[0] == "I": U = VM.Vec(np.where(U.val == np.iinfo(NP[typ]).min, NP[typ](-7), U.val), U.pres)      # (-INT_MIN is not a value of the type)
    u = dev(U); W = operand(typ, n, "blocks", seed=31); M = VM.Vec(mask_values(np.random.default_rng(32), "INT8", n), presence("half", n, 33)); m = dev(M)
    acc = "LOR" if typ == "BOOL" else "PLUS"
    for label, run, model in (("AINV", lambda **k: u.apply(T.AINV, **k), VM.apply("AINV", typ, U)), ("ABS", lambda **k: u.apply(T.ABS, **k), VM.apply("ABS", typ, U)),
                              ("first MINUS", lambda **k: u.apply_first(s, T.MINUS, **k), VM.bind1st("MINUS", typ, s, U)),
                              ("second MINUS", lambda **k: u.apply_second(T.MINUS, s, **k), VM.bind2nd("MINUS", typ, U, s))):
        check(run(), model, f"apply {label} {typ}")
        w = dev(W); run(out=w, mask=m, accum=getattr(T, acc), desc=D.R)
        check(w, VM.write_back(W, model, M, False, False, True, (acc, typ)), f"apply {label} {typ} masked, accumulated, replace")
    thunks = [False, True] if typ == "BOOL" else [0, 7, 7 if typ[0] == "U" else -3]
    for sel in ("NONZERO", "EQ_ZERO", "GT_ZERO", "GE_ZERO", "LT_ZERO", "LE_ZERO"):
        check(u.select(sel), VM.select(sel, None, U), f"select {sel} {typ}")
    for sel in ("NE_THUNK", "EQ_THUNK", "GT_THUNK", "GE_THUNK", "LT_THUNK", "LE_THUNK"):
        for t in thunks: check(u.select(sel, t), VM.select(sel, t, U), f"select {sel} thunk={t} {typ}")


@pytest.mark.parametrize("src", WIDTHS)
def test_cast_between_the_widths(gpu, src):
    """k_cast for the 4 x 4 pairs of value widths (every value stays inside both types: the plain C conversion)."""
    U = operand(src, N_MID, "half", seed=34)
    if src == "FP32": U = VM.Vec(np.abs(U.val), U.pres)                          # (a negative floating-point value has no UINT16 image; integers wrap)
    u = dev(U)
    for dst in WIDTHS:
        check(u.cast(TYPE[dst]), VM.cast(U, dst), f"cast {src} -> {dst}")


# ---- scalar assign ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPES)
def test_scalar_assign_at_n_mid(gpu, typ):
    """k_vec_assign_scalar (all positions; an index list with the first, the last and the sweep-boundary indices; through allow bytes with another accumulator
    type) and k_vec_assign_scalar_masked (the mask read in place), with and without accumulator and replace."""
    T = TYPE[typ]; n = N_MID; s = True if typ == "BOOL" else 9; acc = "LXOR" if typ == "BOOL" else "PLUS"
    W = operand(typ, n, "half", seed=40)
    w = dev(W); w.assign_scalar(s); check(w, VM.assign_scalar(W, s), f"assign all {typ}")
    w = dev(W); w.assign_scalar(s, accum=getattr(T, acc)); check(w, VM.assign_scalar(W, s, accum=(acc, typ)), f"assign all accumulated {typ}")
    idx = [0, 15, 16, 524287, 524288, n - 17, n - 16, n - 1, 12345]
    w = dev(W); w.assign_scalar(s, index=idx); check(w, VM.assign_scalar(W, s, index=idx), f"assign index list {typ}")
    w = dev(W); w.assign_scalar(s, index=idx, accum=getattr(T, acc)); check(w, VM.assign_scalar(W, s, index=idx, accum=(acc, typ)), f"assign index list accumulated {typ}")
    for k, mt in enumerate(("BOOL", "FP32", "INT64", "INT8")):
        M = VM.Vec(mask_values(np.random.default_rng(41 + k), mt, n), presence("half", n, 42)); m = dev(M)
        for struct, comp, replace, a in ((False, False, False, None), (True, True, True, None), (False, True, False, acc), (False, False, True, acc)):
            w = dev(W); w.assign_scalar(s, mask=m, accum=getattr(T, a) if a else None, desc=desc_of(replace, struct, comp))
            check(w, VM.assign_scalar(W, s, None, M, struct, comp, replace, (a, typ) if a else None), f"assign masked {typ} mask {mt} struct={struct} comp={comp} replace={replace} accum={a}")


@pytest.mark.parametrize("n", [4095, 4096, 4097, 65535, 65536, N_MID, 8388608 + 7, N_BIG])
def test_one_byte_masked_assign(gpu, n):
    """k_assign_masked_bytes (n >= 4096, both types one byte, no accumulator): 16 positions per lane, the n % 16 tail by one thread, past one round of 2048
    workgroups at 8 388 608 + 7; below 4096 the generic kernel.  Valued / structural / complemented / replace, for BOOL / UINT8 / INT8 under BOOL / UINT8."""
    combos = [("BOOL", "BOOL"), ("UINT8", "BOOL"), ("INT8", "UINT8"), ("UINT8", "UINT8")] if n < 1 << 23 else [("UINT8", "BOOL"), ("INT8", "UINT8")]
    for wt, mt in combos:
        W = operand(wt, n, "half", seed=50)
        M = VM.Vec(mask_values(np.random.default_rng(51), "BOOL" if mt == "BOOL" else "INT8", n).astype(NP[mt]), presence("blocks", n, 52)); m = dev(M)
        s = True if wt == "BOOL" else 7
        for struct, comp, replace in ((False, False, False), (True, False, True), (False, True, True), (True, True, False)) if n < 1 << 23 else ((False, False, False), (False, True, True)):
            w = dev(W); w.assign_scalar(s, mask=m, desc=desc_of(replace, struct, comp))
            check(w, VM.assign_scalar(W, s, None, M, struct, comp, replace), f"one-byte assign {wt} under {mt} n={n} struct={struct} comp={comp} replace={replace}")
    W = VM.Vec(np.zeros(n, np.uint8), presence("empty", n)); w = dev(W)         # s = 0: a stored zero is an entry
    w.assign_scalar(0, mask=m); check(w, VM.assign_scalar(W, 0, None, M), f"one-byte assign of a zero n={n}")


def test_code_bytes_after_the_masked_assign_and_from_scratch(gpu, monkeypatch):
    """A masked pull `q<!v, replace> = v lor.land A` over an R-MAT-17 pattern (>= 2^20 entries, n = 131 072 >= 65 536) gathers one code byte per neighbour: the
    bytes the masked assign left behind (k_assign_masked_bytes, n >= 65 536), those k_vec_code_bytes builds for an imported vector, and — with
    GRB_MI355X_CODE_BYTES=0 — the value and presence bytes themselves must all give the model's result."""
    from pygraphblas_amd import rmat
    n = 1 << 17; rp, ci = rmat.csr_numpy(17); rp = rp.astype(np.int64)
    assert len(ci) >= 1 << 20
    A = gb.Matrix.from_csr(gb.BOOL, n, n, rp.astype(np.uint32), ci, np.ones(len(ci), np.bool_))
    rows = np.repeat(np.arange(n), np.diff(rp)); cols = ci.astype(np.int64)
    rng = np.random.default_rng(60)
    V0 = VM.Vec(rng.integers(0, 3, n).astype(np.uint8), presence("half", n, 60)); Q = VM.Vec(rng.random(n) < 0.7, presence("blocks", n, 61))
    V1 = VM.assign_scalar(V0, 7, None, Q)

    def model(V):
        has = np.bincount(cols, weights=V.pres[rows].astype(np.float64), minlength=n) > 0            # some stored neighbour
        val = np.bincount(cols, weights=(V.pres & (V.val != 0))[rows].astype(np.float64), minlength=n) > 0
        return VM.write_back(VM.empty(n, "BOOL"), VM.Vec(val, has), V, False, True, True)
    for setting in (None, "0"):
        if setting is None: monkeypatch.delenv("GRB_MI355X_CODE_BYTES", raising=False)
        else: monkeypatch.setenv("GRB_MI355X_CODE_BYTES", setting)
        v = dev(V0); v.assign_scalar(7, mask=dev(Q)); check(v, V1, "v[q] = 7")
        for label, vec, Vm in (("after the masked assign", v, V1), ("imported", dev(V0), V0)):
            q = gb.Vector.sparse(gb.BOOL, n)
            vec.vxm(A, mask=vec, out=q, desc=D.RC)
            plan = gb.last_kernel_plan()
            assert "mask=operand" in plan and ("code bytes" in plan) == (setting is None), plan
            check(q, model(Vm), f"masked pull {label}, GRB_MI355X_CODE_BYTES={setting}")


@pytest.mark.parametrize("typ", ["BOOL", "INT64"])
def test_a_few_entries_into_a_long_vector(gpu, typ):
    """k_init_small: at most 16 entries handed over as kernel arguments, zeros everywhere else, past one round of its 4096 workgroups of 16 positions."""
    n = N_INIT; idx = np.array([0, 15, 16, 17, 4096 * 256 * 16 - 1, 4096 * 256 * 16, n - 6, n - 1], np.uint64)
    x = np.array([True] * 8) if typ == "BOOL" else np.array([5, -6, 7, 1 << 62, -(1 << 63), 9, 10, -11], np.int64)
    v = gb.Vector.from_arrays(idx, x, n, TYPE[typ])
    exp = VM.empty(n, typ); exp.val[idx.astype(np.int64)] = x; exp.pres[idx.astype(np.int64)] = True
    got, p = v.to_dense_arrays()
    assert np.array_equal(p != 0, exp.pres) and np.array_equal(got, exp.val) and v.nvals == 8          # (the values behind the holes are zeros here: the kernel's promise)


# ---- big holes -------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_per_row(n):
    rng = np.random.default_rng(70)
    c0 = rng.integers(0, n, n); c1 = (c0 + 1 + rng.integers(0, n - 1, n)) % n
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    return np.arange(0, 2 * n + 1, 2, dtype=np.uint32), np.stack([lo, hi], 1).reshape(-1).astype(np.uint32)


@pytest.mark.parametrize("typ", ["INT32", "INT64", "FP32", "FP64"])
def test_min_plus_and_max_plus_over_an_operand_with_holes(gpu, typ):
    """`u vxm A` under MIN_PLUS and MAX_PLUS, A with two entries per row (2 * N_MID >= 2^20 entries): k_value_range over u (ordered-integer atomics, the sign-flip
    encoding of floats), k_cast_fill and k_big_to_absent on the "big holes" route for `half`; `edges` is too sparse for it; an infinity in the byte tail makes
    k_value_range refuse.  Against a numpy reference (values on the 1/8 grid: every sum is exact)."""
    n = N_MID; T = TYPE[typ]; rp, ci = two_per_row(n)
    ax = values(np.random.default_rng(71), typ, 2 * n); A = gb.Matrix.from_csr(T, n, n, rp, ci, ax)
    rows = np.repeat(np.arange(n), 2); cols = ci.astype(np.int64); order = np.argsort(cols, kind="stable")
    for pat, inf in (("half", False), ("edges", False)) + ((("half", True),) if typ.startswith("FP") else ()):
        U = operand(typ, n, pat, seed=72)
        if inf: U = planted(U, n - 2, NP[typ](np.inf))
        for add, uf in (("MIN", np.minimum), ("MAX", np.maximum)):
            got = dev(U).vxm(A, semiring=getattr(T, add + "_PLUS"))
            live = U.pres[rows][order]; cs = cols[order][live]; s = (U.val[rows] + ax)[order][live]
            starts = np.flatnonzero(np.concatenate(([True], cs[1:] != cs[:-1])))
            exp = VM.empty(n, typ); exp.pres[cs[starts]] = True; exp.val[cs[starts]] = uf.reduceat(s, starts)
            check(got, exp, f"{add}_PLUS {typ} {pat} infinity={inf}")
