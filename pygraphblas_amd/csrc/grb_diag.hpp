// grb_diag.hpp — host interface of the diagonal kernels (grb_diag.hip): a vector onto the k-th diagonal of a square CSR, and the k-th diagonal of a CSR as a bitmap;
// and the geometry of a diagonal (host arithmetic only, shared by both routes of GxB_Matrix_diag / GxB_Vector_diag in grb_diag_ops.cpp).
#pragma once
#include "grb_internal.hpp"

namespace grb {

// ---- where diagonal k lies: unsigned arithmetic throughout (k = INT64_MIN has no int64 negative) ---------------------------------------------
inline uint64_t diag_abs(int64_t k) { return k < 0 ? 0ull - (uint64_t)k : (uint64_t)k; }
// position r of the diagonal is entry (r + diag_row0(k), r + diag_col0(k))
inline uint64_t diag_row0(int64_t k) { return k < 0 ? diag_abs(k) : 0; }
inline uint64_t diag_col0(int64_t k) { return k < 0 ? 0 : diag_abs(k); }
// positions of diagonal k in an nrows x ncols matrix (0: k lies outside it)
inline uint64_t diag_len(uint64_t nrows, uint64_t ncols, int64_t k) {
  const uint64_t r0 = diag_row0(k), c0 = diag_col0(k);
  if (r0 >= nrows || c0 >= ncols) return 0;
  const uint64_t a = nrows - r0, b = ncols - c0;
  return a < b ? a : b;
}
// dimension of the square matrix that holds a vector of n_v positions on its k-th diagonal; false when it wraps 64 bits
inline bool diag_dim(uint64_t n_v, int64_t k, uint64_t* n) { const uint64_t ak = diag_abs(k); *n = n_v + ak; return *n >= n_v; }
// the row pointer of that matrix when every position of the vector holds an entry (`total` = n_v) or in general (`scan[r]` = entries before position r):
// rows before the diagonal (k < 0) repeat 0, rows after it (k >= 0) repeat the total
inline uint64_t diag_rowptr_at(uint64_t row, uint64_t n_v, int64_t k, uint64_t total, const uint32_t* scan /* nullptr: all present */) {
  const uint64_t r0 = diag_row0(k);
  if (row < r0) return 0;
  const uint64_t r = row - r0;
  if (r >= n_v) return total;
  return scan ? scan[r] : r;
}

// T = the square CSR of dimension n_v + |k| with v(r) at (r, r + k) (k >= 0) or (r + |k|, r) (k < 0); one entry per row at most.  `vval` / `vpres`: the bitmap of a
// vector of n_v positions whose values have type `tcode` (moved by their size, untouched); vpres == nullptr or `all_present`: every position holds an entry
// — then there is no scan and no read-back.  Requires n_v + |k| <= GRB_DIM_DEVICE_MAX (checked by the caller).  Returns whether the all-present path ran.
bool diag_to_csr(int tcode, uint64_t n_v, const void* vval, const uint8_t* vpres, int64_t k, DevCSR& T, bool all_present = false);

// t(r) = A(r, r + k) (k >= 0) or A(r + |k|, r) (k < 0) for r < len, as a bitmap (value 0 where absent); `ts` bytes per value, moved untouched.  A's rows are
// sorted.  len == diag_len(A.nrows, A.ncols, k) (the caller computed it); nothing is launched for len == 0.  No read-back.
void csr_diag_to_bitmap(size_t ts, const DevCSR& A, int64_t k, uint64_t len, void* tval, uint8_t* tpres);

}  // namespace grb
