"""loops.connected_components: min-label propagation whose pointer jump g = g(g) takes its index list from HBM (GrBX_Vector_extract_Vector).
The reference is scipy.sparse.csgraph.connected_components: every vertex must carry the smallest vertex id of its component, exactly."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components as scipy_components

pytestmark = pytest.mark.gpu

PATH, CLIQUE, SPARSE, ISOLATED = 300, 20, 810, 50


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if isinstance(obj, gb.Matrix) else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def no_jump_sweeps(path_ids):
    """A lower bound of the sweeps of plain min-label propagation (no pointer jump) on a path whose vertices carry `path_ids` in path order: a label moves one
    edge per sweep, so the smallest id needs as many sweeps as its distance to the farther end, at least half the path.  Fewer sweeps than this cannot happen
    unless the jump ran."""
    pos = int(np.argmin(path_ids))
    return max(pos, len(path_ids) - 1 - pos)


def graph(rng):
    """a path of 300 (a long diameter), two cliques of 20, a random sparse part, 50 isolated vertices; ids shuffled, symmetrised"""
    n = PATH + 2 * CLIQUE + SPARSE + ISOLATED
    edges = [(i, i + 1) for i in range(PATH - 1)]
    base = PATH
    for _ in range(2):
        edges += [(base + a, base + b) for a in range(CLIQUE) for b in range(a + 1, CLIQUE)]
        base += CLIQUE
    edges += [(base + int(a), base + int(b)) for a, b in rng.integers(0, SPARSE, (SPARSE * 3 // 4, 2)) if a != b]
    perm = rng.permutation(n)
    e = perm[np.array(edges, np.int64)]
    S = sp.coo_matrix((np.ones(len(e), np.bool_), (e[:, 0], e[:, 1])), shape=(n, n))
    S = ((S + S.T) > 0).tocsr()
    S.sort_indices()
    return n, S, perm


def test_labels_are_the_component_minima(gb, gpu):
    from pygraphblas_amd import loops
    rng = np.random.default_rng(7)
    n, S, perm = graph(rng)
    assert 1150 <= n <= 1250
    A = gb.Matrix.from_csr(gb.BOOL, n, n, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), np.ones(S.nnz, np.bool_))
    assert residency(gb, A) == 2
    plans = []
    f, sweeps = loops.connected_components(A, plans=plans)
    assert residency(gb, A) == 2, "A stays in HBM only"
    assert len(plans) == sweeps and all(p.startswith("extract_vector<index=list@hbm>") and "k_index_parse" in p for p in plans), plans[:2]
    ncomp, lab = scipy_components(S, directed=False)
    assert ncomp > ISOLATED + 3
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    gi, gx = f.to_arrays()
    assert np.array_equal(gi, np.arange(n, dtype=np.uint64)) and gx.dtype == np.int64
    assert np.array_equal(gx, smallest[lab])
    assert sweeps < PATH, f"{sweeps} sweeps: the pointer jump did not shorten the path of {PATH}"
    assert sweeps < no_jump_sweeps(perm[:PATH]), (sweeps, no_jump_sweeps(perm[:PATH]))


def test_path_alone_needs_fewer_sweeps_than_propagation_without_the_jump(gb, gpu):
    from pygraphblas_amd import loops
    n = PATH
    rng = np.random.default_rng(8)
    perm = rng.permutation(n)
    a, b = perm[:-1], perm[1:]
    S = sp.coo_matrix((np.ones(2 * (n - 1), np.bool_), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    S.sort_indices()
    A = gb.Matrix.from_csr(gb.BOOL, n, n, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), np.ones(S.nnz, np.bool_))
    f, sweeps = loops.connected_components(A)
    assert np.array_equal(f.to_arrays()[1], np.zeros(n, np.int64)) and sweeps < n
    assert sweeps < no_jump_sweeps(perm), (sweeps, no_jump_sweeps(perm))
    assert residency(gb, A) == 2
