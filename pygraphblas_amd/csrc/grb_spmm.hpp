// grb_spmm.hpp — host interface of the product with a FULL right operand (grb_spmm.hip; the integer geometry is grb_spmm_geom.hpp): T = A (+).(x) B for A any
// CSR (m x n) and B full (n x k: nnz == n k, so its value array IS the row-major dense array).  The pattern of T is known in advance — row i holds all k
// columns when A(i, :) holds an entry and none otherwise — so there is no symbolic pass, no hashing and no sort: one scan for the row pointer, one fill for the
// columns, and the value kernels.  One more producer of T for GrB_mxm's write-back (grb_matrix_ops.cpp, the `spmm_full` route).
#pragma once
#include "grb_matops.hpp"
#include "grb_spmm_geom.hpp"

namespace grb {

// what the route reports in the plan string
struct SpmmPlan { uint32_t k = 0, group = 0, slabs = 0; uint64_t nlong = 0; };

// T = A (+).(x) B.  c.A any CSR, c.B full (the caller has tested spmm_is_full); c.aval / c.bval as in SpgemmCall: values already in the semiring's type, nullptr
// when the multiplier ignores that side — nothing is loaded from it.  Every entry of T is the fold of its products in ascending column of A (rows of at most
// SPMM_L entries: left to right; longer rows: left to right inside a chunk, then the chunks in ascending order) — no atomics, the same bits on every run.
// false: T would not fit the 32-bit layout; nothing was written and the caller takes another route.
bool spmm_full(const SpgemmCall& c, const SemiringDesc& d, DevCSR& out, SpmmPlan& plan);

// The pattern of a matrix whose non-empty rows are full, written in HBM by one kernel: rowptr[i] = k before[i] for i in [0, nrows] (before == nullptr: k i, every
// row is non-empty), col[e] = e mod k for e < nnz.  `before`: the number of non-empty rows in front of each row, nrows + 1 words.
void full_pattern_fill(uint32_t nrows, uint32_t k, uint64_t nnz, const uint32_t* before, uint32_t* rowptr, uint32_t* col);

// ---- between the driver (grb_spmm.hip) and the value kernels (grb_spmm_kernels.hpp, one instantiation per value type: grb_spmm_inst.hip) ----
struct SpmmValuesCall {
  const DevCSR* A; const void* aval; const void* bval; uint32_t k;
  const uint32_t* trp; void* tval;                                       // T's row pointer and value array
  uint64_t nlong, nslots; const uint32_t* task; const uint32_t* lrank; const uint32_t* lrow; void* part;      // the long rows (nlong == 0: none of these is read)
};
template <class T> void run_spmm_values(const SpmmValuesCall& c, const SemiringDesc& d);

}  // namespace grb
