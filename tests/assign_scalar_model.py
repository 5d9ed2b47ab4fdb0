"""A model of the matrix scalar assign `C<M, replace>(I, J) = accum(C(I, J), s)` (test infrastructure), numpy only and independent of the library, built on
tests/matrix_model.py::write_back.  Two formulations of the operand T:

  * `assign_scalar`             T is the full block: s (cast to C's type) at every position of I x J — the C API's own statement;
  * `assign_scalar_restricted`  T is the part of the mask's pattern that lies inside I x J and that the mask counts as true.  Only for a mask that is not
                                complemented: the write-back reads T only where the mask allows a write, so both give the same C.  It never forms the
                                block, so a 70 000 x 70 000 region costs what the mask's entries cost.

Both end in write_back with the accumulator, or SECOND in C's type when there is none: assign keeps the entries of C outside the region and replaces those
inside it, which is SECOND on the union of the two patterns.  `rows` / `cols` are the positions the index arguments name (any order; a repeat changes nothing).
"""
import numpy as np

import matrix_model as mm


def _scalar(s, typ, n):
    return np.full(n, mm.cast(np.asarray(s), typ)[()], mm.NP[typ])


def full_block(C, s, rows, cols):
    r = np.unique(np.asarray(rows, np.int64)); c = np.unique(np.asarray(cols, np.int64))
    keys = (r[:, None] * np.int64(C.ncols) + c[None, :]).ravel()
    return mm.Mat(C.nrows, C.ncols, keys, _scalar(s, C.typ, len(keys)))


def mask_block(C, s, rows, cols, mask, struct):
    truth = np.ones(mask.nvals, bool) if struct else (mask.vals != 0)
    inside = np.isin(mask.rows, np.asarray(rows, np.int64)) & np.isin(mask.cols, np.asarray(cols, np.int64))
    keys = mask.keys[truth & inside]
    return mm.Mat(C.nrows, C.ncols, keys, _scalar(s, C.typ, len(keys)))


def assign_scalar(C, s, rows, cols, mask=None, struct=False, comp=False, replace=False, accum=None):
    """accum: (operator, type) or None."""
    return mm.write_back(C, full_block(C, s, rows, cols), mask, struct, comp, replace, accum or ("SECOND", C.typ))


def assign_scalar_restricted(C, s, rows, cols, mask, struct=False, replace=False, accum=None):
    assert mask is not None
    return mm.write_back(C, mask_block(C, s, rows, cols, mask, struct), mask, struct, False, replace, accum or ("SECOND", C.typ))
