// grb_sddmm.hpp — host interface of the masked product of two FULL matrices (grb_sddmm.hip; the integer geometry is grb_sddmm_geom.hpp): T<M> = X (+).(x) Y' for
// X (m x k) and Y (n x k) full — nnz == rows k, so each value array IS the row-major dense array — and M any CSR mask (m x n).  The pattern of T is the mask's own
// pattern and every entry is the dot product of two contiguous rows, so there is no hashing, no symbolic pass and no sort: a copy of the mask's row pointer and
// columns, and one value kernel over tiles of mask entries.  One more producer of T for GrB_mxm's write-back (grb_matrix_ops.cpp, the `sddmm` route).
#pragma once
#include "grb_matops.hpp"
#include "grb_sddmm_geom.hpp"

namespace grb {

// what the route reports in the plan string
struct SddmmPlan { uint32_t k = 0, group = 0; uint64_t entries = 0; };

// T(i, j) = (+)_l X(i, l) (x) Y(j, l) for EVERY entry (i, j) of M's pattern (the mask's values are not read: a valued mask is applied by the write-back).
// xval / yval: the row-major m x k / n x k values already in the semiring's type, nullptr when the multiplier ignores that side — nothing is loaded from it (the
// SpgemmCall contract).  k >= 1.  Fold order, a function of k alone: with G = sddmm_group(k), lane g of an entry's group folds the products l = g, g + G, ... left
// to right starting from the first one; then for s = G / 2 ... 1, p_g = p_g (+) p_{g + s} where g + s < min(k, G).  No atomics, no LDS: the same bits on every
// run, wherever the entry lies in the mask.
void sddmm_full(const DevCSR& M, const void* xval, const void* yval, uint32_t k, const SemiringDesc& d, DevCSR& out, SddmmPlan& plan);

// ---- between the driver (grb_sddmm.hip) and the value kernel (grb_sddmm_kernels.hpp, one instantiation per value type: grb_sddmm_inst.hip) ----
struct SddmmValuesCall {
  const uint32_t* mrp; const uint32_t* mcol; uint32_t m; uint64_t entries;      // the mask's pattern (= T's)
  const void* xval; const void* yval; uint32_t k; void* tval;
};
template <class T> void run_sddmm_values(const SddmmValuesCall& c, const SemiringDesc& d);

}  // namespace grb
