"""Facts about a vector's device image (grb_vecfacts.hpp) must not outlive the image: every producer of a fact crossed with every writer that voids it, then
the consumer that would use the fact, against tests/vector_model.py and the oracle — values and patterns exact.

One square matrix, n = 65 536 with a little over 2^20 entries (INT32 weights 1..255, and its pattern as BOOL): the smallest sizes at which the code-byte route
(n >= 2^16, nnz >= 2^20) and the big-holes route (nnz >= 2^20, 64 * nvals >= n) of grb_mxv.cpp engage.

  producers   chain      the output of a deferred element-wise chain                                  holes_zero
              sweep      `v<accum MIN> = v MIN_PLUS A`                                                holes_big, abs_bound, the edge bound kept
              short      `v.assign_scalar(level, mask=q)`, q three entries made from lists            the small list
              long       the same with n / 5 entries in q, v a one-byte level vector                  code bytes, the edge bound taken from q
              frontier   a BOOL `vxm` with replace under the level vector as mask and operand         lor_state, the edge summary
  writers     setElement + removeElement (flushed by the consumer), apply in place, unmasked assign_scalar, output of eWiseAdd, output of mxv, resize, clear
  consumers   the next product with the vector as operand (and as mask for the level vectors), then nvals, reduce and the whole content
"""
import numpy as np
import pytest

from oracle import oracle as O
import pygraphblas_amd as gb
from pygraphblas_amd import descriptor as D
from helpers import TYPE, to_matrix
import vector_model as VM

pytestmark = pytest.mark.gpu

N = 1 << 16
PRODUCERS = ["chain", "sweep", "short", "long", "frontier"]
WRITERS = ["edits", "apply", "assign", "ewise_out", "mxv_out", "resize", "clear"]


@pytest.fixture(scope="module")
def graph(gpu):
    rng = np.random.default_rng(101)
    key = np.unique(rng.integers(0, N * N, size=1_080_000, dtype=np.int64))
    assert len(key) > 1 << 20
    I, J = np.divmod(key.astype(np.uint64), np.uint64(N))
    At = O.Tuples("INT32", N, N, I, J, rng.integers(1, 256, len(key)).astype(np.int32))
    Bt = O.Tuples("BOOL", N, N, I, J, np.ones(len(key), np.bool_))
    return {"A": to_matrix(At), "At": At, "B": to_matrix(Bt), "Bt": Bt}


# ---- model <-> library <-> oracle ------------------------------------------------------------------------------------------------------------------------
def rand_vec(rng, typ, count, lo, hi):
    pres = np.zeros(N, bool); pres[rng.choice(N, size=count, replace=False)] = True
    return VM.Vec(np.where(pres, rng.integers(lo, hi, N), 0).astype(VM.NP[typ]), pres)


def on_device(m):
    return gb.Vector.from_dense_array(m.val, TYPE[m.typ], present=m.pres.astype(np.uint8))


def row(m, typ=None):
    at = np.flatnonzero(m.pres)
    return O.row_vector(typ or m.typ, N, at, m.val[at])


def col(m):
    at = np.flatnonzero(m.pres)
    return O.col_vector(m.typ, N, at, m.val[at])


def from_oracle(t, typ):
    idx = (t.J if t.nrows == 1 else t.I).astype(np.int64)
    val = np.zeros(N, VM.NP[typ]); pres = np.zeros(N, bool)
    val[idx] = t.X; pres[idx] = True
    return VM.Vec(val, pres)


def same(x, m, what):
    val, pres = x.to_dense_arrays()
    assert np.array_equal(pres != 0, m.pres), (what, "pattern", gb.last_kernel_plan())
    assert np.array_equal(val[m.pres], m.val[m.pres]), (what, "values", gb.last_kernel_plan())


def content(x, m, what):
    """nvals first (a stale count shows here), then reduce (a stale `any true`), then every position."""
    assert x.nvals == m.nvals, (what, "nvals")
    if m.typ == "BOOL":
        assert x.reduce_bool() == bool(VM.reduce("LOR", "BOOL", m)), (what, "reduce")
    else:
        assert x.reduce_int() == int(VM.reduce("PLUS", "INT64", m)), (what, "reduce")
    same(x, m, what)


# ---- the products the loops run --------------------------------------------------------------------------------------------------------------------------
def sweep(g, x, m):
    """`v<accum MIN> = v MIN_PLUS A` in place; the plan it took."""
    x.vxm(g["A"], semiring=gb.INT32.MIN_PLUS, accum=gb.INT32.MIN, out=x)
    plan = gb.last_kernel_plan()
    return from_oracle(O.vxm(row(m), row(m), g["At"], "MIN", "PLUS", "INT32", accum="MIN", accum_type="INT32"), "INT32"), plan


def level_pull(g, v, m):
    """`q<!v, replace> = v lor.land A` with the level vector as mask and operand; q, its model and the plan."""
    q = gb.Vector.sparse(gb.BOOL, N)
    v.vxm(g["B"], semiring=gb.BOOL.LOR_LAND, mask=v, out=q, desc=D.RC)
    plan = gb.last_kernel_plan()
    want = O.vxm(O.row_vector("BOOL", N), row(m), g["Bt"], "LOR", "LAND", "BOOL", mask=row(m), replace=True, mask_comp=True)
    return q, from_oracle(want, "BOOL"), plan


# ---- producers: (vector, model) with the fact recorded ---------------------------------------------------------------------------------------------------
def produce(name, g, rng):
    if name == "chain":
        a, b = rand_vec(rng, "INT32", N // 2, 1, 50), rand_vec(rng, "INT32", N // 2, 1, 50)
        x = on_device(a).emult(on_device(b), gb.INT32.TIMES).apply_second(gb.INT32.PLUS, 1)
        return x, VM.bind2nd("PLUS", "INT32", VM.ewise("TIMES", "INT32", a, b, False), 1)
    if name == "sweep":
        m = rand_vec(rng, "INT32", N // 4, 0, 1000)
        x = on_device(m)
        m, plan = sweep(g, x, m)
        assert "k_spmv_xcd" in plan or "k_spmv_wavepipe" in plan, plan      # the big-holes route, not the row-block fallback
        return x, m
    if name == "short":
        at = [5, 30000, N - 3]
        q = gb.Vector.from_lists(at, [True] * 3, N, gb.BOOL)
        x = gb.Vector.sparse(gb.UINT8, N)
        x.assign_scalar(1, mask=q)
        m = VM.empty(N, "UINT8"); m.val[at] = 1; m.pres[at] = True
        return x, m
    m = rand_vec(rng, "UINT8", N // 4, 0, 3)                                  # a third of the entries are explicit zeros
    qm = rand_vec(rng, "BOOL", N // 5, 0, 2)
    x = on_device(m)
    x.assign_scalar(7, mask=on_device(qm))
    m = VM.assign_scalar(m, 7, mask=qm)
    if name == "long":
        return x, m
    q, qmodel, plan = level_pull(g, x, m)                                     # "frontier"
    assert "mask=operand" in plan and "code bytes" in plan, plan
    return q, qmodel


# ---- writers: the vector is written, the model follows ---------------------------------------------------------------------------------------------------
def write(name, g, rng, x, m):
    typ = m.typ; T = TYPE[typ]; m = m.copy()
    if name == "edits":
        gone, changed = np.flatnonzero(m.pres)[[0, -1]]
        new = np.flatnonzero(~m.pres)[[1, -2]]
        del x[int(gone)]; m.pres[gone] = False
        for i, s in ((changed, 0), (new[0], 1), (new[1], 0)):               # an explicit zero over an entry, an entry and an explicit zero into holes
            x[int(i)] = VM.NP[typ](s).item(); m.val[i] = s; m.pres[i] = True
        return m
    if name == "apply":
        if typ == "BOOL":                                                     # (the model has no LNOT: every stored value flips)
            x.apply(gb.BOOL.LNOT, out=x)
            return VM.Vec(~m.val, m.pres)
        x.apply(T.AINV, out=x)
        return VM.apply("AINV", typ, m)
    if name == "assign":
        x.assign_scalar(VM.NP[typ](1).item())
        return VM.assign_scalar(m, 1)
    if name == "ewise_out":
        a, b = rand_vec(rng, typ, N // 3, 0, 2), rand_vec(rng, typ, N // 3, 0, 2)
        op = "LOR" if typ == "BOOL" else "PLUS"
        on_device(a).eadd(on_device(b), getattr(T, op), out=x)
        return VM.ewise(op, typ, a, b, True)
    if name == "mxv_out":
        u = rand_vec(rng, typ, N // 8, 1, 2)
        g["B"].mxv(on_device(u), semiring=getattr(T, "ANY_PAIR"), out=x)
        return from_oracle(O.mxv(O.col_vector(typ, N), g["Bt"], col(u), "ANY", "PAIR", typ), typ)
    if name == "resize":
        x.resize(N // 2); x.resize(N)
        m.pres[N // 2:] = False
        return m
    x.clear()
    return VM.empty(N, typ)


# ---- consumers ---------------------------------------------------------------------------------------------------------------------------------------------
def consume(g, x, m, what):
    if m.typ == "INT32":
        # `r<accum PLUS> = r + A plus.times x` into a full r: an operand whose holes hold zeros is gathered as it stands
        r = gb.Vector.dense(gb.INT32, N, fill=3)
        g["A"].mxv(x, semiring=gb.INT32.PLUS_TIMES, out=r, accum=gb.INT32.PLUS)
        full = VM.Vec(np.full(N, 3, np.int32), np.ones(N, bool))
        same(r, from_oracle(O.mxv(col(full), g["At"], col(m), "PLUS", "TIMES", "INT32", accum="PLUS", accum_type="INT32"), "INT32"), what + " / plus.times")
        assert x.nvals == m.nvals, (what, "nvals")
        # the next sweep of the shortest-path loop: holes that hold a BIG value and the bound of |x| are taken as they stand
        before = m
        m, plan = sweep(g, x, m)
        pipeline = "k_spmv_xcd" in plan or "k_spmv_wavepipe" in plan
        assert pipeline == (before.nvals * 64 >= N), (what, plan)            # big holes (or a full operand) against the row-block fallback
        content(x, m, what + " / sweep")
    elif m.typ == "UINT8":
        q, qmodel, plan = level_pull(g, x, m)
        # a handful of entries is pushed from the list (or counted and pushed); from a few thousand on the level is pulled with the code bytes
        assert m.nvals <= 64 or m.nvals >= 8000, what
        assert ("push" in plan) if m.nvals <= 64 else ("mask=operand" in plan and "code bytes" in plan), (what, plan)
        same(q, qmodel, what + " / level pull")
        assert q.reduce_bool() == bool(qmodel.val[qmodel.pres].any()), (what, "frontier reduce")
        content(x, m, what)
    else:
        assert x.reduce_bool() == bool(m.val[m.pres].any()), (what, "reduce")
        assert x.nvals == m.nvals, (what, "nvals")
        w = x.vxm(g["B"], semiring=gb.BOOL.LOR_LAND)
        same(w, from_oracle(O.vxm(O.row_vector("BOOL", N), row(m), g["Bt"], "LOR", "LAND", "BOOL"), "BOOL"), what + " / lor.land")
        # the level vector takes the frontier: `v[q] = level`, then the next level's pull
        lv = rand_vec(np.random.default_rng(7), "UINT8", N // 4, 1, 3)
        v = on_device(lv)
        v.assign_scalar(9, mask=x)
        lv = VM.assign_scalar(lv, 9, mask=m)
        q, qmodel, plan = level_pull(g, v, lv)
        assert "mask=operand" in plan and "code bytes" in plan, (what, plan)
        same(q, qmodel, what + " / next level")
        content(x, m, what)


@pytest.mark.parametrize("producer", PRODUCERS)
def test_facts_do_not_outlive_the_image(graph, producer):
    rng = np.random.default_rng(PRODUCERS.index(producer) + 11)
    for writer in WRITERS:
        what = producer + " -> " + writer
        x, m = produce(producer, graph, rng)
        m = write(writer, graph, rng, x, m)
        consume(graph, x, m, what)
    x, m = produce(producer, graph, rng)                                      # no writer: the consumer uses the fact
    consume(graph, x, m, producer + " -> (none)")
