"""What a product derives from a matrix's device CSR (grb_devcsr.hpp: the row-block plan, kernel W's and kernel X's plans, the transpose cache) is not used after
the matrix changed — on a matrix large enough for kernel W and kernel X to build their plans.

One INT64 matrix, 4096 x 4096, 32 entries per row: 131 072 entries, at least 2^16 (`A[i, j] = x` on a stored entry overwrites in place) and at least 64 x 256
(GRB_MI355X_SPMV=wavepipe / xcd run their kernels).  Values and the full operand are small integers: every product is exact and is compared with a numpy model.
Per route, `A.mxv(u)` and `u.vxm(A)` (so the CSR and the transpose cache both hold derived data) run before and after each way a matrix can change:
an overwrite in place, a queue of value-only edits, a structural queue, a resize to fewer rows and to fewer columns, and an operation whose result A adopts."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, PER_ROW = 4096, 32


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def residency(gb, A):
    w = C.c_int(-1)
    assert gb.lib.GrBX_Matrix_residency(A._h, C.byref(w)) == 0
    return w.value


@pytest.fixture(scope="module")
def base():
    """rowptr, columns (sorted within a row, never column 0 or the last one), values 1 .. 49; left unchanged by the tests."""
    rng = np.random.default_rng(23)
    col = np.concatenate([np.sort(rng.choice(N - 2, size=PER_ROW, replace=False) + 1) for _ in range(N)]).astype(np.uint32)
    val = rng.integers(1, 50, N * PER_ROW).astype(np.int64)
    rp = (np.arange(N + 1) * PER_ROW).astype(np.uint32)
    for a in (rp, col, val):
        a.setflags(write=False)
    return rp, col, val


class Case:
    """The matrix in HBM and its model {(i, j): value} with the current dimensions."""

    def __init__(self, gb, base, kernel):
        rp, col, val = base
        self.gb, self.kernel, self.nr, self.nc = gb, kernel, N, N
        self.A = gb.Matrix.from_csr(gb.INT64, N, N, rp, col, val)
        assert residency(gb, self.A) == 2 and self.A.nvals == N * PER_ROW >= 1 << 16
        rows = np.repeat(np.arange(N), PER_ROW)
        self.model = {(int(i), int(j)): int(x) for i, j, x in zip(rows, col, val)}

    def products(self):
        """A.mxv(u) and u.vxm(A), PLUS_TIMES over a full operand u[k] = 1 + k % 7, against the model; returns the plan of the first product."""
        gb, nr, nc = self.gb, self.nr, self.nc
        keys = np.array(list(self.model.keys()), np.int64).reshape(-1, 2)
        vals = np.fromiter(self.model.values(), np.int64, len(self.model))
        ur, uc = 1 + np.arange(nc, dtype=np.int64) % 7, 1 + np.arange(nr, dtype=np.int64) % 7
        want_r, want_c, has_r, has_c = np.zeros(nr, np.int64), np.zeros(nc, np.int64), np.zeros(nr, bool), np.zeros(nc, bool)
        np.add.at(want_r, keys[:, 0], vals * ur[keys[:, 1]]); has_r[keys[:, 0]] = True
        np.add.at(want_c, keys[:, 1], vals * uc[keys[:, 0]]); has_c[keys[:, 1]] = True
        plans = []
        for want, has, run in ((want_r, has_r, lambda: self.A.mxv(gb.Vector.from_dense_array(ur, gb.INT64), semiring=gb.INT64.PLUS_TIMES)),
                               (want_c, has_c, lambda: gb.Vector.from_dense_array(uc, gb.INT64).vxm(self.A, semiring=gb.INT64.PLUS_TIMES))):
            w = run()
            plans.append(gb.last_kernel_plan())
            if self.kernel:                                       # the forced kernel ran: its plan is what this case is about
                assert self.kernel in plans[-1], plans[-1]
            x, p = w.to_dense_arrays()
            assert np.array_equal(p != 0, has), plans[-1]
            assert np.array_equal(np.where(has, x, 0), want), plans[-1]
        assert residency(gb, self.A) == 2
        return plans[0]

    def set(self, i, j, x):
        self.A[i, j] = x
        self.model[(i, j)] = x

    def delete(self, i, j):
        del self.A[i, j]
        self.model.pop((i, j), None)

    def resize(self, nr, nc):
        self.A.resize(nr, nc)
        self.nr, self.nc = nr, nc
        self.model = {k: v for k, v in self.model.items() if k[0] < nr and k[1] < nc}
        assert self.A.shape == (nr, nc) and residency(self.gb, self.A) == 2


# (GRB_MI355X_SPMV, the kernel its plan string must name, products before the first change: the unforced route runs twice, past the plan policy's first use)
ROUTES = [("adaptive", None, 1), ("wavepipe", "k_spmv_wavepipe", 1), ("xcd", "k_spmv_xcd", 1), (None, None, 2)]


@pytest.mark.parametrize("route,kernel,warm", ROUTES, ids=[r[0] or "unforced" for r in ROUTES])
def test_derived_data_follows_the_matrix(gb, base, route, kernel, warm):
    with env(GRB_MI355X_SPMV=route):
        c = Case(gb, base, kernel)
        for _ in range(warm):
            c.products()
        stored = sorted(c.model)

        # 1. an overwrite of a stored entry, applied in place: nothing is queued, so the next product's plan does not begin with a flush
        c.set(*stored[len(stored) // 2], 1000)
        assert not c.products().startswith("edit<"), "the overwrite was queued, not applied in place"

        # 2. value-only edits, queued (a delete of an absent entry opens the queue: an overwrite behind it is not applied in place) and flushed by the product
        c.delete(0, 0)
        for k in range(0, len(stored), 1999):
            c.set(*stored[k], 2000 + k % 13)
        plan = c.products()
        assert plan.startswith("edit<on=matrix,") and ",ins=0,del=0>" in plan and "k_edit_values" in plan, plan

        # 3. a structural queue: inserts (a new first column, a new last column, inside a row) and deletes
        c.set(5, 0, 7); c.set(N - 1, N - 1, 9); c.set(100, next(j for j in range(1, N) if (100, j) not in c.model), 11)
        c.delete(*stored[50]); c.delete(*stored[-1])
        plan = c.products()
        assert plan.startswith("edit<on=matrix,") and "k_edit_rowptr" in plan, plan
        assert c.A.nvals == len(c.model)
        c.products()

        # 4. fewer rows, then fewer columns
        c.resize(3000, N)
        c.products()
        c.resize(3000, 3500)
        c.products()
        c.products()

        # 5. A adopts the result of an operation on itself
        c.A.apply(gb.INT64.AINV, out=c.A)
        c.model = {k: -v for k, v in c.model.items()}
        c.products()
        c.products()
        assert c.A.nvals == len(c.model)
