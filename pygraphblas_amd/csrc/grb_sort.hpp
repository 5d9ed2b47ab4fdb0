// grb_sort.hpp — host interface of the sort kernels (grb_sort.hip): the rows of a CSR ordered by value, a bitmap vector ordered by value, and the flags of a
// top-k selection.  The order is grb_sort_keys.hpp's; the routes (which operand, which transpose, the write-back) are in grb_sort_ops.cpp.
#pragma once
#include "grb_internal.hpp"
#include "grb_sort_keys.hpp"

namespace grb {

// what a row sort did: rows per bin and the kernels launched (the tail of the plan string)
struct SortPlan { uint64_t wave = 0, lds = 0, prim = 0; int key_bits = 32; std::string kernels; };

// For every entry place e of R, in row r = the row of e with i = e - rowptr[r]: perm[e] = the place in R of the i-th entry of row r in sorted order, ocol[e] = i.
// `kcode` / `kval`: the type the comparison runs in and R's values in that type (R.val itself when it is R's type).  `prim_only`: every row goes through the
// segmented radix sort (GRB_MI355X_SORT=prim).  perm and ocol are allocated here (nnz words each, + slack).
void csr_sort_positions(const DevCSR& R, int kcode, const void* kval, bool gt, bool prim_only, DevBuf& perm, DevBuf& ocol, SortPlan& plan);

// The sorted matrices from perm / ocol: T (values of `ts` bytes moved untouched through perm) unless nullptr, Tp (INT64: the column each value came from)
// unless nullptr; both get R's row pointer and ocol as their columns.
void csr_sort_fill(const DevCSR& R, size_t ts, const DevBuf& perm, const DevBuf& ocol, DevCSR* T, DevCSR* Tp);

// keep[perm[e]] = ocol[e] < k: one byte per entry of R, 1 for the first min(k, len) entries of each row in sorted order
void topk_flags(uint64_t nnz, const DevBuf& perm, const DevBuf& ocol, uint64_t k, uint8_t* keep);

// A bitmap vector of n positions: the indices of its present entries in sorted order (sidx, allocated here); returns nvals (one read-back).
uint64_t vec_sort_positions(int kcode, const void* kval, const uint8_t* pres, uint64_t n, bool gt, DevBuf& sidx, SortPlan& plan);
// The sorted vectors: position i < nvals holds the value at sidx[i] (tval, `ts` bytes, untouched) / sidx[i] itself as INT64 (pval); positions beyond hold 0 and
// are absent.  Either pair may be nullptr.
void vec_sort_fill(size_t ts, const void* uval, const DevBuf& sidx, uint64_t nvals, uint64_t n, void* tval, uint8_t* tpres, void* pval, uint8_t* ppres);
// tpres (n bytes) = 1 exactly at the first `keep` sorted indices
void vec_topk_flags(const DevBuf& sidx, uint64_t keep, uint64_t n, uint8_t* tpres);

}  // namespace grb
