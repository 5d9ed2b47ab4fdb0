"""A numpy model of GxB_eWiseUnion (test infrastructure), independent of the library, beside tests/matrix_model.py and tests/vector_model.py whose containers,
operators and typecasts it uses:

    T(i,j) = op(A(i,j), B(i,j))    both operands hold an entry
             op(A(i,j), beta)      only A does
             op(alpha,  B(i,j))    only B does

on the union of the two patterns, in the operator's type `typ`: operand values, alpha and beta are cast into it first (`astype`: 2.75 into INT32 is 2).  The
operator is called on three index sets and on nothing else, so a value behind a hole (a zero divisor, say) is never looked at.  `op` is an operator name of
matrix_model.binop, or a Python function of two arrays of the operator's type (a user-defined operator).

tests/test_union_model.py pins it to a dictionary transcription of the three cases and to matrix_model.ewise / vector_model.ewise over padded operands;
tests/test_ewise_union_gpu.py compares the library with it."""
import numpy as np

import matrix_model as MM
import vector_model as VM

NP = MM.NP


def _call(op, typ, x, y):
    x, y = MM.cast(x, typ), MM.cast(y, typ)
    if callable(op):
        with np.errstate(all="ignore"):
            return np.asarray(op(x, y)).astype(NP[typ])
    return MM.binop(op, typ, x, y)


def _three_sets(op, typ, ka, va, alpha, kb, vb, beta):
    """(keys, values) of the union of two ascending key lists."""
    keys = np.union1d(ka, kb)
    vals = np.zeros(len(keys), NP[typ])
    both, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    only_a = ~np.isin(ka, kb, assume_unique=True); only_b = ~np.isin(kb, ka, assume_unique=True)
    fill = lambda s, n: np.full(n, MM.cast(np.asarray(s), typ), NP[typ])
    vals[np.searchsorted(keys, both)] = _call(op, typ, va[ia], vb[ib])
    vals[np.searchsorted(keys, ka[only_a])] = _call(op, typ, va[only_a], fill(beta, int(only_a.sum())))
    vals[np.searchsorted(keys, kb[only_b])] = _call(op, typ, fill(alpha, int(only_b.sum())), vb[only_b])
    return keys, vals


def union(op, typ, a, alpha, b, beta):
    """T of GxB_eWiseUnion for two MM.Mat of one shape, or two VM.Vec of one size."""
    if isinstance(a, VM.Vec):
        assert a.n == b.n
        ka, kb = np.flatnonzero(a.pres), np.flatnonzero(b.pres)
        keys, vals = _three_sets(op, typ, ka, a.val[ka], alpha, kb, b.val[kb], beta)
        val = np.zeros(a.n, NP[typ]); val[keys] = vals
        return VM.Vec(val, a.pres | b.pres)
    assert (a.nrows, a.ncols) == (b.nrows, b.ncols)
    keys, vals = _three_sets(op, typ, a.keys, a.vals, alpha, b.keys, b.vals, beta)
    return MM.Mat(a.nrows, a.ncols, keys, vals)
