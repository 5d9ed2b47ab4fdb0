"""Host-side logic of the backend that needs no GPU: the object model behind the C ABI (build / setElement /
extract / remove / resize / dup on the host mirror), descriptors, the type registry and promotion table,
context managers, the R-MAT generator (numpy == torch) and the row-block partitioner."""
import os
import numpy as np
import pytest

from pygraphblas_amd_rmat import rmat


def test_matrix_container_roundtrip(gb):
    from pygraphblas_amd import Matrix, INT64, FP64, NoValue, InvalidIndex, OutputNotEmpty
    m = Matrix.from_lists([2, 0, 1], [0, 1, 2], [3, 1, 2])
    assert (m.nrows, m.ncols, m.nvals) == (3, 3, 3) and m.type is INT64
    assert m.to_lists() == [[0, 1, 2], [1, 2, 0], [1, 2, 3]]            # row-major order
    assert m[0, 1] == 1 and m.get(0, 0) is None
    with pytest.raises(NoValue):
        m[0, 0]
    m[0, 0] = 7; m[0, 0] = 9                                             # last write wins
    assert m[0, 0] == 9 and m.nvals == 4
    del m[0, 0]; del m[1, 2]
    assert m.to_lists() == [[0, 2], [1, 0], [1, 3]]
    with pytest.raises(InvalidIndex):
        m[5, 0] = 1
    d = m.dup(); d[1, 1] = 5
    assert m.nvals == 2 and d.nvals == 3
    d.clear(); assert d.nvals == 0
    f = Matrix.from_lists([0], [0], [1.5]); assert f.type is FP64 and f[0, 0] == 1.5
    with pytest.raises(OutputNotEmpty):
        gb.lib.GrB_Matrix_build_INT64.restype = int
        from pygraphblas_amd.base import check
        import ctypes as C
        I = np.array([0], np.uint64); X = np.array([1], np.int64)
        check(gb.lib.GrB_Matrix_build_INT64(m._h, I.ctypes.data_as(C.c_void_p), I.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p), C.c_uint64(1), None), m)


def test_build_combines_duplicates_with_dup_op(gb):
    from pygraphblas_amd import Matrix, Vector, INT64, InvalidValue
    I = np.array([0, 0, 1, 0], np.uint64); J = np.array([1, 1, 2, 1], np.uint64); X = np.array([5, 7, 1, 2], np.int64)
    assert Matrix.from_arrays(I, J, X, 2, 3, INT64, dup=INT64.PLUS).to_lists() == [[0, 1], [1, 2], [14, 1]]
    assert Matrix.from_arrays(I, J, X, 2, 3, INT64, dup=INT64.MIN).to_lists() == [[0, 1], [1, 2], [2, 1]]
    assert Matrix.from_arrays(I, J, X, 2, 3, INT64, dup=INT64.SECOND).to_lists() == [[0, 1], [1, 2], [2, 1]]
    with pytest.raises(InvalidValue):
        Matrix.from_arrays(I, J, X, 2, 3, INT64)
    assert Vector.from_arrays(I, X, 4, INT64, dup=INT64.PLUS).to_lists() == [[0, 1], [14, 1]]


def test_vector_container_and_casts(gb):
    from pygraphblas_amd import Vector, UINT8, BOOL, FP32, INT8
    v = Vector.from_lists([3, 1], [2, 4], size=5)
    assert v.size == 5 and v.nvals == 2 and v.to_lists() == [[1, 3], [4, 2]]
    v[4] = 9; del v[1]
    assert list(v) == [(3, 2), (4, 9)] and 3 in v and 1 not in v
    u = Vector.sparse(UINT8, 4); u[0] = 300 % 256; assert u[0] == 44
    b = Vector.sparse(BOOL, 4); b[2] = True; assert b.to_lists() == [[2], [True]]
    # extractElement typecasts like C with float->int saturation
    import ctypes as C
    f = Vector.sparse(FP32, 2); f[0] = 1e10
    out = C.c_int8(0); gb.lib.GrB_Vector_extractElement_INT8(C.byref(out), f._h, C.c_uint64(0)); assert out.value == 127
    assert Vector.sparse(INT8).size == gb.GxB_INDEX_MAX                      # default dimension (pygraphblas/__init__.py:366-367)


def test_resize_and_huge_dimensions(gb):
    from pygraphblas_amd import Matrix, INT64
    m = Matrix.sparse(INT64)                                                  # 2^60 x 2^60 host-only hypersparse container
    m[2 ** 40, 5] = 1; m[3, 2 ** 50] = 2
    assert m.nvals == 2 and m[2 ** 40, 5] == 1
    import ctypes as C
    from pygraphblas_amd.base import check
    check(gb.lib.GrB_Matrix_resize(m._h, C.c_uint64(10), C.c_uint64(10)), m)
    assert (m.nrows, m.ncols, m.nvals) == (10, 10, 0)


def test_descriptors(gb):
    from pygraphblas_amd import descriptor as D
    assert D.T1 in D.CT1 and D.C in D.CT1 and D.T0 not in D.CT1 and D.T0 not in D.RC
    assert D.CT1 == (D.C & D.T1) and D.RSCT0T1 == (D.R & D.S & D.C & D.T0 & D.T1)
    assert D.T1 != D.T0 and repr(D.RC) == "<Descriptor RC>"
    with D.T0:
        assert D.current_desc.get() is D.T0
    assert D.current_desc.get(None) is None


def test_type_registry_and_promotion(gb):
    from pygraphblas_amd import BOOL, INT8, UINT8, INT16, UINT16, INT32, UINT32, INT64, UINT64, FP32, FP64, promote
    assert INT64.PLUS_TIMES is INT64.plus_times and INT64.PLUS_TIMES.ztype is INT64 and BOOL.LOR_LAND.ztype is BOOL
    assert FP32.PLUS_SECOND.ztype is FP32 and UINT8.MIN_PLUS.ztype is UINT8
    assert INT64._default_semiring() is INT64.PLUS_TIMES and BOOL._default_semiring() is BOOL.LOR_LAND
    order = [FP64, FP32, INT64, UINT64, INT32, UINT32, INT16, UINT16, INT8, UINT8]   # pygraphblas/types.py:465-482
    for i, a in enumerate(order):
        for j, b in enumerate(order):
            assert promote(a, b) is order[min(i, j)]
        assert promote(a, BOOL) is a and promote(BOOL, a) is a
    assert promote(BOOL, BOOL) is BOOL


def test_context_managers(gb):
    from pygraphblas_amd import INT64, Accum, types
    with INT64.MIN_PLUS:
        assert types.current_semiring.get() is INT64.MIN_PLUS
    assert types.current_semiring.get(None) is None
    with Accum(INT64.MIN):
        assert types.current_accum.get() is INT64.MIN
    assert types.current_accum.get(None) is None


def test_rmat_numpy_equals_torch_and_is_sliceable():
    import torch
    s, d = rmat.edges_numpy(11, seed=7)
    s2, d2 = rmat.edges_torch(11, "cpu", seed=7)
    assert np.array_equal(s.astype(np.int64), s2.numpy()) and np.array_equal(d.astype(np.int64), d2.numpy())
    s3, d3 = rmat.edges_numpy(11, seed=7, first=1000, count=500)
    assert np.array_equal(s3, s[1000:1500]) and np.array_equal(d3, d[1000:1500])
    for kw in (dict(), dict(symmetric=True, drop_self_loops=True), dict(symmetric=True, drop_self_loops=True, lower=True), dict(row_range=(256, 1024))):
        rp, c = rmat.csr_numpy(11, **kw); rp2, c2 = rmat.csr_torch(11, "cpu", **kw)
        assert np.array_equal(rp, rp2.numpy().view(np.uint32)) and np.array_equal(c, c2.numpy().view(np.uint32))
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))
        assert np.all(np.diff(rows * (1 << 32) + c.astype(np.int64)) > 0)       # sorted, no duplicates
    assert np.array_equal(rmat.values_numpy(100), rmat.values_torch(100, "cpu").numpy())
    # skew sanity: (a+b)=0.76 of the edges land in the top half of the rows
    assert abs((s < 1024).mean() - 0.76) < 0.01


def test_balanced_row_blocks(gb):
    from pygraphblas_amd.dist import balanced_row_blocks, rmat_expected_row_prefix
    rp, _ = rmat.csr_numpy(12)
    b = balanced_row_blocks(rp.astype(np.int64), 8)
    assert b[0] == 0 and b[-1] == 4096 and all(x <= y for x, y in zip(b, b[1:]))
    per = np.diff(rp.astype(np.int64)[b]); assert per.max() < 1.35 * per.mean()
    # the analytic prefix every rank can compute without the graph gives nearly the same split
    b2 = balanced_row_blocks(rmat_expected_row_prefix(12), 8)
    per2 = np.diff(rp.astype(np.int64)[b2]); assert per2.max() < 1.6 * per2.mean()
    assert balanced_row_blocks(rp.astype(np.int64), 1) == [0, 4096]


# ---- text readers ---------------------------------------------------------------------------------
import pygraphblas_amd as gb

# the 7x7 matrix of the reference's doctests (pygraphblas/matrix.py:381-394 from_mm, :415-425 from_tsv): entries 0..11
_DOC_I = [0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 6, 6]
_DOC_J = [1, 3, 4, 6, 5, 0, 2, 5, 2, 2, 3, 4]
_DOC_V = list(range(12))


def _doc_lines(sep):
    return "".join(f"{i + 1}{sep}{j + 1}{sep}{v}\n" for i, j, v in zip(_DOC_I, _DOC_J, _DOC_V))


def test_from_mm_matches_reference_doctest(tmp_path):
    p = tmp_path / "t.mm"
    p.write_text("%%MatrixMarket matrix coordinate integer general\n%%GraphBLAS GrB_INT64\n7 7 12\n" + _doc_lines(" "))
    M = gb.Matrix.from_mm(p)
    assert M.type is gb.INT64 and (M.nrows, M.ncols, M.nvals) == (7, 7, 12)
    I, J, V = M.to_lists()
    assert (list(I), list(J), list(V)) == (_DOC_I, _DOC_J, _DOC_V)


def test_from_mm_symmetric_pattern_and_real(tmp_path):
    p = tmp_path / "s.mm"
    p.write_text("%%MatrixMarket matrix coordinate real symmetric\n% a comment\n3 3 3\n1 1 2.5\n2 1 -1.0\n3 2 4.0\n")
    M = gb.Matrix.from_mm(p)
    assert M.type is gb.FP64 and M.nvals == 5
    I, J, V = M.to_lists()
    assert sorted(zip(I, J, V)) == [(0, 0, 2.5), (0, 1, -1.0), (1, 0, -1.0), (1, 2, 4.0), (2, 1, 4.0)]
    q = tmp_path / "p.mm"
    q.write_text("%%MatrixMarket matrix coordinate pattern general\n2 3 2\n1 3\n2 1\n")
    P = gb.Matrix.from_mm(q)
    assert P.type is gb.BOOL and sorted(zip(*P.to_lists())) == [(0, 2, True), (1, 0, True)]


def test_from_tsv_matches_reference_doctest(tmp_path):
    p = tmp_path / "t.tsv"
    p.write_text(_doc_lines("\t"))
    M = gb.Matrix.from_tsv(p, gb.INT32, 7, 7)
    assert M.type is gb.INT32
    I, J, V = M.to_lists()
    assert (list(I), list(J), list(V)) == (_DOC_I, _DOC_J, _DOC_V)


def test_readers_on_the_reference_fixture_files():
    """The reference's docs/test_mm.mm and docs/test_tsvfile.tsv, copied byte for byte to tests/golden/."""
    golden = os.path.join(os.path.dirname(__file__), "golden")
    M = gb.Matrix.from_mm(os.path.join(golden, "reference_docs_test_mm.mm"))
    assert M.type is gb.INT64 and [list(x) for x in M.to_lists()] == [_DOC_I, _DOC_J, _DOC_V]
    T = gb.Matrix.from_tsv(os.path.join(golden, "reference_docs_test_tsvfile.tsv"), gb.INT32, 7, 7)
    assert [list(x) for x in T.to_lists()] == [_DOC_I, _DOC_J, _DOC_V]


def test_matrix_random_is_the_reference_generator(gb):
    """Matrix.random draws like the reference's (pygraphblas/matrix.py:499-571): its own test
    (tests/test_matrix.py:1060-1064) expects these four INT8 values for seed 42; host side only."""
    v = gb.Matrix.random(gb.INT8, 4, 10, 10, seed=42)
    assert len(v) == 4
    I, J, X = v.to_arrays()
    assert (I.tolist(), J.tolist(), X.tolist()) == ([1, 2, 4, 8], [0, 1, 3, 1], [62, 46, -70, 24])
    m = gb.Matrix.random(gb.FP64, 10_000, 1000, 1000, seed=42)       # BASELINE.json configs[0]
    assert m.nvals == 9949                                            # 51 of the 10 000 coordinates repeat
    assert gb.Matrix.random(gb.UINT8, 20, 5, 5, make_symmetric=True, no_diagonal=True, seed=42).nvals <= 20


def test_dist_partition_helpers_on_cpu():
    """split_csr_columns / flop_balanced_row_blocks (pygraphblas_amd/dist.py) against plain numpy on a small R-MAT."""
    import torch
    from pygraphblas_amd import rmat, dist as gdist
    scale = 9; n = 1 << scale
    rp, col = rmat.csr_numpy(scale, symmetric=True, drop_self_loops=True, lower=True)
    trp, tcol = torch.from_numpy(rp.view(np.int32)), torch.from_numpy(col.view(np.int32))
    c0, c1 = 100, 300
    (rpd, cd, vd), (rpo, co, vo) = gdist.split_csr_columns(trp, tcol, c0, c1, torch.arange(len(col)))
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    inside = (col >= c0) & (col < c1)
    assert np.array_equal(cd.numpy().view(np.uint32), col[inside]) and np.array_equal(co.numpy().view(np.uint32), col[~inside])
    assert np.array_equal(np.diff(rpd.numpy()), np.bincount(rows[inside], minlength=n))
    assert np.array_equal(np.diff(rpo.numpy()), np.bincount(rows[~inside], minlength=n))
    assert np.array_equal(vd.numpy(), np.flatnonzero(inside))                 # values travel with their entries
    b = gdist.flop_balanced_row_blocks(trp, tcol, 4)
    deg = np.diff(rp.astype(np.int64))
    rowflops = np.add.reduceat(np.append(deg[col], 0), rp[:-1].astype(np.int64)) * (deg > 0)
    parts = [rowflops[b[i]:b[i + 1]].sum() for i in range(4)]
    assert b[0] == 0 and b[-1] == n and sum(parts) == rowflops.sum()
    assert max(parts) <= rowflops.sum() / 4 + rowflops.max()                  # balanced up to one row
    # transpose option of the generator: rows of A' are the columns of A
    rpa, ca = rmat.csr_numpy(scale); rpt, ct = rmat.csr_numpy(scale, transpose=True)
    import scipy.sparse as sp
    M = sp.csr_matrix((np.ones(len(ca)), ca.astype(np.int64), rpa.astype(np.int64)), shape=(n, n))
    Mt = sp.csr_matrix((np.ones(len(ct)), ct.astype(np.int64), rpt.astype(np.int64)), shape=(n, n))
    assert (M.T != Mt).nnz == 0


def test_pagerank_partition_of_an_rmat25_shaped_run_on_eight_ranks():
    """BASELINE.json configs[4] as the driver's N = 8 run cuts it (bench.py: `balanced_row_blocks(rmat_expected_row_prefix(25), 8)`), on the CPU and
    without generating 5.3e8 edges: the bounds every rank derives are identical and monotone, the EXPECTED entries per rank are within 2 % of
    one eighth (R-MAT's skew is in the row labels: equal row COUNTS would give the first rank 3.2 x the average), a rank's share fits its GPU many times
    over, and at a scale small enough to build (R-MAT-16, the same generator) the actual entries follow the expected split and the diagonal /
    off-diagonal split of every block adds up to the block."""
    import torch
    from pygraphblas_amd import rmat, dist as gdist
    world = 8
    prefix = gdist.rmat_expected_row_prefix(25)
    bounds = gdist.balanced_row_blocks(prefix, world)
    assert bounds == gdist.balanced_row_blocks(gdist.rmat_expected_row_prefix(25), world)           # every rank computes the same cut
    assert bounds[0] == 0 and bounds[-1] == 1 << 25 and all(a < b for a, b in zip(bounds, bounds[1:]))
    share = np.diff(prefix[bounds].astype(np.float64)) / float(prefix[-1])
    assert np.all(np.abs(share * world - 1.0) < 0.02), share
    rows = np.diff(np.array(bounds)); assert rows.max() > 2.5 * rows.min()                          # balanced by entries, not by rows
    nnz_total = 5.3e8                                                                                # distinct entries of R-MAT-25 (measured: 5.29e8)
    # bytes a rank holds: its rows of A' twice (diagonal + off-diagonal CSR, 4 B columns), kernel X's panel-major copy (4 B words), the operand and a few vectors
    per_rank = share.max() * nnz_total * (4 + 4 + 4) + 4 * (1 << 25) * 6
    assert per_rank < 0.05 * 288e9, per_rank
    # the same cut on a graph that can be built here
    scale = 16; n = 1 << scale
    b16 = gdist.balanced_row_blocks(gdist.rmat_expected_row_prefix(scale), world)
    rpt, ct = rmat.csr_numpy(scale, transpose=True)
    actual = np.diff(rpt.astype(np.int64)[b16]) / float(len(ct))
    assert np.all(np.abs(actual * world - 1.0) < 0.25), actual                                       # the transpose's rows (in-degrees) follow the same label skew
    seen = 0
    for r in range(world):
        r0, r1 = b16[r], b16[r + 1]
        rp, col = rmat.csr_numpy(scale, transpose=True, row_range=(r0, r1))
        (rpd, cd, _), (rpo, co, _) = gdist.split_csr_columns(torch.from_numpy(rp.view(np.int32)), torch.from_numpy(col.view(np.int32)), r0, r1)
        cdn, con = cd.numpy().view(np.uint32), co.numpy().view(np.uint32)
        assert len(cdn) + len(con) == len(col) and ((cdn >= r0) & (cdn < r1)).all() and ((con < r0) | (con >= r1)).all()
        assert int(rpd[-1]) == len(cdn) and int(rpo[-1]) == len(con)
        seen += len(col)
    assert seen == len(ct)


def test_grb_binary_reader_against_the_references_fixture(tmp_path):
    """Matrix.binread on the reference's docs/test_binfile.grb (copied byte for byte to tests/golden/) gives the matrix of
    docs/test_mm.mm:1-15 (7x7 INT64, 12 entries with values 0..11, transcribed below 0-based); binwrite round-trips."""
    import pygraphblas_amd as gb
    path = os.path.join(os.path.dirname(__file__), "golden", "reference_docs_test_binfile.grb")
    M = gb.Matrix.from_binfile(path)
    assert M.type is gb.INT64 and M.shape == (7, 7) and M.nvals == 12
    mm = [(1, 2, 0), (1, 4, 1), (2, 5, 2), (2, 7, 3), (3, 6, 4), (4, 1, 5), (4, 3, 6), (5, 6, 7), (6, 3, 8), (7, 3, 9), (7, 4, 10), (7, 5, 11)]
    I, J, X = M.to_lists()
    assert sorted(zip(I, J, X)) == sorted((i - 1, j - 1, x) for i, j, x in mm)
    out = tmp_path / "roundtrip.grb"
    M.to_binfile(str(out))
    M2 = gb.Matrix.binread(str(out))
    assert M2.to_lists() == M.to_lists() and M2.type is M.type and M2.shape == M.shape
    F = gb.Matrix.from_lists([0, 2, 2], [1, 0, 3], [1.5, -2.0, 0.25], 3, 4, gb.FP32)
    F.binwrite(str(out)); F2 = gb.Matrix.binread(str(out))
    assert F2.type is gb.FP32 and F2.shape == (3, 4) and F2.to_lists() == F.to_lists()
    with pytest.raises(ValueError):
        (tmp_path / "bad.grb").write_bytes(b"not a matrix"); gb.Matrix.binread(str(tmp_path / "bad.grb"))


def test_mirror_slicing_surface_runs_on_the_host_mirror(gb):
    """`M[i]`, `M[:, j]`, `M[a:b, c:d]` (stop inclusive, as in the reference), `M[i] = v`, `M[:, j] = v`, `M[I, J] = A`, `v[a:b]`,
    `v[I] = u`, from_diag / vector_diag, kronecker — the index operations of the C ABI edit the host mirror, so they work (and are
    checked here) without a device.  Reference: pygraphblas/matrix.py:2807-3130, vector.py:1454-1575."""
    import numpy as np
    rng = np.random.default_rng(3)
    n = 12
    dense = rng.integers(-9, 10, (n, n)); keep = rng.random((n, n)) < 0.4
    I, J = np.nonzero(keep)
    A = gb.Matrix.from_lists(I.tolist(), J.tolist(), dense[keep].tolist(), n, n, gb.INT64)

    def mat(M):
        out = np.zeros((M.nrows, M.ncols), np.int64); pres = np.zeros((M.nrows, M.ncols), bool)
        for i, j, x in M:
            out[i, j] = x; pres[i, j] = True
        return out, pres

    def vec(v):
        out = np.zeros(v.size, np.int64); pres = np.zeros(v.size, bool)
        for i, x in zip(*v.to_lists()):
            out[i] = x; pres[i] = True
        return out, pres
    D = np.where(keep, dense, 0)
    r, rp = vec(A[3]); assert (r == D[3]).all() and (rp == keep[3]).all()
    c, cp = vec(A[:, 5]); assert (c == D[:, 5]).all() and (cp == keep[:, 5]).all()
    s, sp = mat(A[2:6, 1:4]); assert s.shape == (5, 4) and (s == D[2:7, 1:5]).all() and (sp == keep[2:7, 1:5]).all()      # stop inclusive
    s, sp = mat(A[[7, 1, 1], [0, 11]]); assert (s == D[[7, 1, 1]][:, [0, 11]]).all() and (sp == keep[[7, 1, 1]][:, [0, 11]]).all()
    s, sp = mat(A.extract_matrix(slice(0, 3), None, desc=gb.descriptor.T0)); assert (s == D.T[0:4]).all() and (sp == keep.T[0:4]).all()
    seg, segp = vec(A[3, 2:8]); assert (seg == D[3, 2:9]).all() and (segp == keep[3, 2:9]).all()
    # assignments
    v = gb.Vector.from_lists([0, 4, 9], [5, 6, 7], n, gb.INT64)
    B = A.dup(); B[3] = v
    want, wp = D.copy(), keep.copy(); want[3] = 0; wp[3] = False; want[3, [0, 4, 9]] = [5, 6, 7]; wp[3, [0, 4, 9]] = True
    got, gp = mat(B); assert (got == want).all() and (gp == wp).all()
    B = A.dup(); B[:, 5] = v
    want, wp = D.copy(), keep.copy(); want[:, 5] = 0; wp[:, 5] = False; want[[0, 4, 9], 5] = [5, 6, 7]; wp[[0, 4, 9], 5] = True
    got, gp = mat(B); assert (got == want).all() and (gp == wp).all()
    B = A.dup(); B.assign_row(3, v, accum=gb.INT64.PLUS)
    want, wp = D.copy(), keep.copy(); want[3, [0, 4, 9]] += [5, 6, 7]; wp[3, [0, 4, 9]] = True
    got, gp = mat(B); assert (got == want).all() and (gp == wp).all()
    S = gb.Matrix.from_lists([0, 1], [1, 0], [100, 200], 2, 2, gb.INT64)
    B = A.dup(); B[[2, 8], [3, 4]] = S
    want, wp = D.copy(), keep.copy(); want[np.ix_([2, 8], [3, 4])] = [[0, 100], [200, 0]]; wp[np.ix_([2, 8], [3, 4])] = [[False, True], [True, False]]
    got, gp = mat(B); assert (got == want).all() and (gp == wp).all()
    # vectors
    u = gb.Vector.from_lists([1, 2, 5, 8], [10, 20, 50, 80], 10, gb.INT64)
    assert u[2:5].to_lists() == [[0, 3], [20, 50]] and u[[8, 8, 0]].to_lists() == [[0, 1], [80, 80]]
    w = gb.Vector.sparse(gb.INT64, 10); w[[9, 3, 4, 7]] = gb.Vector.from_lists([0, 2], [1, 2], 4, gb.INT64)
    assert w.to_lists() == [[4, 9], [2, 1]]
    # diagonals and kronecker
    d = gb.Vector.from_lists([0, 2], [3, 4], 3, gb.INT64)
    Dm = gb.Matrix.from_diag(d, -1); assert Dm.shape == (4, 4) and sorted(Dm) == [(1, 0, 3), (3, 2, 4)]
    assert Dm.vector_diag(-1).to_lists() == [[0, 2], [3, 4]] and Dm.vector_diag(2).size == 2 and Dm.vector_diag(9).size == 0
    K = gb.Matrix.from_lists([0, 1], [1, 0], [2, 3], 2, 2, gb.INT64).kronecker(gb.Matrix.from_lists([0], [1], [5], 1, 2, gb.INT64), gb.INT64.TIMES)
    assert K.shape == (2, 4) and sorted(K) == [(0, 3, 10), (1, 1, 15)]


def test_grb_all_is_never_materialised_on_hypersparse_containers(gb):
    """`H[1]` / `H[:, 2]` on a default-dimension (2^60) matrix expanded GrB_ALL into a vector of 2^60 indices
    (Panic from the allocator).  GrB_ALL is the identity map now, and a list that cannot exist is refused with an error."""
    H = gb.Matrix.sparse(gb.INT64)
    H[1, 2] = 3
    H[5, 2] = 7
    assert H[1].to_lists() == [[2], [3]]
    assert H[:, 2].to_lists() == [[1, 5], [3, 7]]
    v = gb.Vector.sparse(gb.INT64)
    v[4] = 9
    H[7] = v                                  # GrB_Row_assign over GrB_ALL
    assert H[7].to_lists() == [[4], [9]]
    H[:, 11] = v                              # GrB_Col_assign over GrB_ALL
    assert H[:, 11].to_lists() == [[4], [9]]
    w = v.extract(slice(None))                # GrB_Vector_extract over GrB_ALL
    assert w.to_lists() == [[4], [9]]

