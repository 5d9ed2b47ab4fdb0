// grb_gemm.hpp — host interface of the product of two FULL matrices (grb_gemm.hip; the integer geometry is grb_gemm_geom.hpp): T = op(A) (+).(x) op(B) for op(A)
// (m x k) and op(B) (k x n) full — nnz == rows cols, so each value array IS the row-major dense array of the matrix as it is stored.  T is full as well: its
// pattern is closed form (full_pattern_fill, no scan, no count to fetch) and its values come from one register-tiled kernel that stages pieces of both operands in
// LDS.  A transposed operand is read where it lies, through the staging loader's address arithmetic: no transpose of a dense matrix is ever built.  One more
// producer of T for GrB_mxm's write-back (grb_matrix_ops.cpp, the `gemm_full` route).
//
// THE ORDER GUARANTEE: every thread owns its outputs for the whole of k, so T(i, j) is the plain left-to-right fold of its products in ascending l, starting from
// the product l = 0, for EVERY k — the oracle's order.  It does not depend on the tile an entry lies in, on the tile shape, on the layout flags, on the grid or
// on the run: no chunks, no butterfly, no atomics, no scratch memory; every output word has one writer.
#pragma once
#include "grb_matops.hpp"
#include "grb_gemm_geom.hpp"

namespace grb {

// what the route reports in the plan string
struct GemmPlan { uint32_t m = 0, n = 0, k = 0, tm = 0, tn = 0; bool ta = false, tb = false; };

// T(i, j) = (+)_l op(A)(i, l) (x) op(B)(l, j), m x n, k >= 1, m n within the 32-bit layout (the caller has tested spmm_overflows(m, n)).  aval: A's values as stored —
// m x k row-major, or k x m row-major when `ta` — already in the semiring's type; bval: B's, k x n row-major, or n x k when `tb`.  nullptr when the multiplier
// ignores that side: nothing is loaded or staged from it (the SpgemmCall contract).
void gemm_full(uint32_t m, uint32_t n, uint32_t k, const void* aval, bool ta, const void* bval, bool tb, const SemiringDesc& d, DevCSR& out, GemmPlan& plan);

// ---- between the driver (grb_gemm.hip) and the value kernel (grb_gemm_kernels.hpp, one instantiation per value type: grb_gemm_inst.hip) ----
struct GemmValuesCall { const void* aval; const void* bval; void* tval; uint32_t m, n, k; bool ta, tb; };
template <class T> void run_gemm_values(const GemmValuesCall& c, const SemiringDesc& d);

}  // namespace grb
