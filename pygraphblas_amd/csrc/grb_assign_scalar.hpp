// grb_assign_scalar.hpp — host interface of the matrix scalar assign kernels (grb_assign_scalar.hip): the operand T of C<M>(I, J) = accum(C(I, J), s) built in HBM.
// The region arithmetic is in grb_assign_scalar_geom.hpp (plain integers, checked on the host).
#pragma once
#include "grb_assign.hpp"
#include "grb_assign_scalar_geom.hpp"

namespace grb {

// Index arguments are ExIdx that passed assign_inverse (no index named twice); `inv_i` / `inv_j` are its tables (unused for GrB_ALL and ranges).
// `scalar`: the value in T's type, `ts` bytes (1, 2, 4, 8).  T gets C's shape, sorted rows, every value = the scalar.

// Mask-driven: T = the entries of M inside I x J that count as true (`mstruct`: every stored entry; else a non-zero value in M's own type `mcode`).
// O(nnz(M)) whatever |I| |J| is; one read-back, nnz(T).  M may be the output's own CSR: T shares nothing with it.
void scalar_from_mask(const DevCSR& M, int mcode, bool mstruct, const ExIdx& I, const DevBuf& inv_i, const ExIdx& J, const DevBuf& inv_j, const void* scalar, size_t ts, DevCSR& T);

// Closed form: T = all of I x J in an nrows x ncols matrix.  Requires scalar_region_fits(I.n, J.n) (the caller raised the error otherwise).  No read-back.
void scalar_block(uint32_t nrows, uint32_t ncols, const ExIdx& I, const DevBuf& inv_i, const ExIdx& J, const DevBuf& inv_j, const void* scalar, size_t ts, DevCSR& T);

}  // namespace grb
