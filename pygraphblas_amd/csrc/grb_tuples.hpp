// grb_tuples.hpp — host interface of extractTuples in HBM (grb_tuples.hip); the entry points are GrBX_Matrix_extractTuples_at / GrBX_Vector_extractTuples_at in
// grb_tuples_ops.cpp, the tile arithmetic is in grb_tuples_geom.hpp.
#pragma once
#include "grb_internal.hpp"
#include "grb_tuples_geom.hpp"

namespace grb {

// The entries of a device CSR as lists in stored order — row-major, and inside a row the order the columns are stored in (ascending for every producer of the
// library): I[k] = the row of entry k, J[k] = col[k] zero-extended, X[k] = val[k] untouched.  All pointers are device pointers; any of I / J / X may be nullptr and
// that stream is then neither computed nor written.  Requires A.nnz > 0 and room for A.nnz elements behind every non-null pointer (checked by the caller).
// One launch of k_tuples_csr on the library's stream, not synchronised.
void tuples_from_csr(const DevCSR& A, size_t ts, uint64_t* I, uint64_t* J, void* X);

// The present positions of a bitmap vector (pres[p] != 0) in ascending order.  tuples_count_bitmap: one count word per TUPLES_VEC_WAVE positions, their exclusive
// scan into `offs` (nwords + 1 words, the last one the total) and the total read back (one synchronisation).  tuples_from_bitmap: I[rank] = p and
// X[rank] = val[p] for every present p, rank = offs[its wave's word] + the present positions before it in that word's range.  n > 0; I or X may be nullptr.
uint64_t tuples_count_bitmap(const uint8_t* pres, uint64_t n, DevBuf& offs);
void tuples_from_bitmap(const uint8_t* pres, const void* val, size_t ts, uint64_t n, const DevBuf& offs, uint64_t* I, void* X);
// ... and of a vector known to be full: I[p] = p, X = a copy of val.  n > 0.
void tuples_from_full(const void* val, size_t ts, uint64_t n, uint64_t* I, void* X);

}  // namespace grb
