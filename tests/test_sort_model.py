"""The numpy model of the sort tests (tests/sort_model.py) on cases worked out by hand: one per rule of the order, then the matrix and vector forms."""
import numpy as np

import sort_model as M

NAN = float("nan")


def test_ties_keep_the_smaller_index_first():
    v, idx = np.array([2, 1, 2, 1], np.int32), np.array([0, 1, 2, 3])
    assert M.order(v, idx, gt=False).tolist() == [1, 3, 0, 2]           # 1@1, 1@3, 2@0, 2@2
    assert M.order(v, idx, gt=True).tolist() == [0, 2, 1, 3]            # 2@0, 2@2, 1@1, 1@3: descending values, ASCENDING indices among equals
    # the index decides, not the place in the array
    assert M.order(v, np.array([9, 8, 3, 2]), gt=False).tolist() == [3, 1, 2, 0]


def test_negative_zero_ties_positive_zero():
    v = np.array([0.0, -0.0, -1.0, -0.0], np.float64)
    assert M.order(v, np.arange(4), gt=False).tolist() == [2, 0, 1, 3]   # -1, then the three zeros by index
    assert M.order(v, np.arange(4), gt=True).tolist() == [0, 1, 3, 2]    # the three zeros by index, then -1
    v32 = np.array([-0.0, 0.0], np.float32)
    assert M.order(v32, np.arange(2), gt=False).tolist() == [0, 1] and M.order(v32, np.arange(2), gt=True).tolist() == [0, 1]


def test_nans_come_last_under_both_operators_and_tie():
    other_nan = np.array([0xFFF8000000000123], np.uint64).view(np.float64)[0]           # negative sign, a payload
    v = np.array([NAN, 1.0, np.inf, other_nan, -np.inf], np.float64)
    assert M.order(v, np.arange(5), gt=False).tolist() == [4, 1, 2, 0, 3]               # -inf, 1, +inf, then the NaNs by index
    assert M.order(v, np.arange(5), gt=True).tolist() == [2, 1, 4, 0, 3]                # +inf, 1, -inf, then the NaNs by index — not first


def test_values_are_never_negated():
    u = np.array([2**64 - 1, 0, 2**63], np.uint64)
    assert M.order(u, np.arange(3), gt=False).tolist() == [1, 2, 0] and M.order(u, np.arange(3), gt=True).tolist() == [0, 2, 1]
    s = np.array([-2**63, 2**63 - 1, -1], np.int64)
    assert M.order(s, np.arange(3), gt=False).tolist() == [0, 2, 1] and M.order(s, np.arange(3), gt=True).tolist() == [1, 2, 0]
    b = np.array([True, False, True], np.bool_)
    assert M.order(b, np.arange(3), gt=False).tolist() == [1, 0, 2] and M.order(b, np.arange(3), gt=True).tolist() == [0, 2, 1]


# the 3 x 4 matrix      col 0   1   2   3
#               row 0    5   .   1   5
#               row 1    .   .   .   .
#               row 2    2   7   .   2
I = np.array([0, 0, 0, 2, 2, 2], np.uint64)
J = np.array([0, 2, 3, 0, 1, 3], np.uint64)
X = np.array([5, 1, 5, 2, 7, 2], np.int32)


def test_matrix_sort_by_row():
    ci, cj, cx, px = M.matrix_sort(I, J, X, gt=False)
    assert ci.tolist() == [0, 0, 0, 2, 2, 2] and cj.tolist() == [0, 1, 2, 0, 1, 2]
    assert cx.tolist() == [1, 5, 5, 2, 2, 7] and px.tolist() == [2, 0, 3, 0, 3, 1] and px.dtype == np.int64
    ci, cj, cx, px = M.matrix_sort(I, J, X, gt=True)
    assert cx.tolist() == [5, 5, 1, 7, 2, 2] and px.tolist() == [0, 3, 2, 1, 0, 3]


def test_matrix_sort_by_column():
    # column 0 holds 5@row0, 2@row2; column 1 7@2; column 2 1@0; column 3 5@0, 2@2.  C(k, j) = k-th value of column j, P(k, j) = its row.
    ci, cj, cx, px = M.matrix_sort(I, J, X, gt=False, by_col=True)
    assert ci.tolist() == [0, 0, 0, 0, 1, 1] and cj.tolist() == [0, 1, 2, 3, 0, 3]
    assert cx.tolist() == [2, 7, 1, 2, 5, 5] and px.tolist() == [2, 2, 0, 2, 0, 0]


def test_matrix_topk():
    i, j, x = M.matrix_topk(I, J, X, 2, gt=True)                      # row 0: 5@0, 5@3 (1 dropped); row 2: 7@1 and the 2 with the SMALLER column
    assert list(zip(i.tolist(), j.tolist(), x.tolist())) == [(0, 0, 5), (0, 3, 5), (2, 0, 2), (2, 1, 7)]
    i, j, x = M.matrix_topk(I, J, X, 1, gt=False)
    assert list(zip(i.tolist(), j.tolist(), x.tolist())) == [(0, 2, 1), (2, 0, 2)]
    assert len(M.matrix_topk(I, J, X, 0)[0]) == 0 and len(M.matrix_topk(I, J, X, 9)[0]) == 6
    i, j, x = M.matrix_topk(I, J, X, 1, gt=True, by_col=True)         # per column: 5@(0,0), 7@(2,1), 1@(0,2), 5@(0,3)
    assert list(zip(i.tolist(), j.tolist(), x.tolist())) == [(0, 0, 5), (0, 2, 1), (0, 3, 5), (2, 1, 7)]


def test_vector_forms():
    idx, x = np.array([1, 4, 6, 9], np.uint64), np.array([3.0, NAN, -2.0, 3.0], np.float32)
    wx, px = M.vector_sort(idx, x, gt=False)
    assert M.bits(wx).tolist() == M.bits(np.array([-2.0, 3.0, 3.0, NAN], np.float32)).tolist() and px.tolist() == [6, 1, 9, 4]
    wx, px = M.vector_sort(idx, x, gt=True)
    assert px.tolist() == [1, 9, 6, 4]
    ki, kx = M.vector_topk(idx, x, 1, gt=True)
    assert ki.tolist() == [1] and kx.tolist() == [3.0]                 # of the two 3.0 the smaller index
    ki, kx = M.vector_topk(idx, x, 3, gt=True)
    assert ki.tolist() == [1, 6, 9]
    assert len(M.vector_topk(idx, x, 0)[0]) == 0 and M.vector_topk(idx, x, 10)[0].tolist() == [1, 4, 6, 9]


def test_the_comparison_type_is_the_operators():
    x = np.array([1.75, 1.25, -0.5, 0.5, 3e10, NAN], np.float64)      # as INT32: 1, 1, 0, 0, INT32_MAX, 0
    assert M.cast(x, np.int32).tolist() == [1, 1, 0, 0, 2**31 - 1, 0]
    wx, px = M.vector_sort(np.arange(6), x, gt=False, key_dtype=np.int32)
    assert px.tolist() == [2, 3, 5, 0, 1, 4] and M.bits(wx).tolist() == M.bits(x[[2, 3, 5, 0, 1, 4]]).tolist()      # the values themselves are A's
    assert M.cast(np.array([2.0, 0.0, NAN]), np.bool_).tolist() == [True, False, True]
