// grb_kron.hpp — host interface of the Kronecker product kernels (grb_kron.hip): T = A (x)_op B, CSR in, CSR out.
#pragma once
#include "grb_internal.hpp"

namespace grb {

// Entries the product may hold on the device: T's row pointer and its entry positions are 32-bit (the bound of GrBX_Matrix_import_CSR).
constexpr uint64_t KRON_MAX_ENTRIES = 0xFFFFFFF0ull;

// T[(ia br + ib, ja bc + jb)] = op(A[ia, ja], B[ib, jb]) for every pair of entries, in the type `code` (the operator's domain, comparisons included: 0 / 1 in that
// type, as apply_binop gives them).  `aval` / `bval`: the operands' values already in that type, or nullptr when the operator does not read that side
// (FIRST / SECOND / PAIR / ANY) — it is then never touched.  A and B have sorted rows; so has T.
// Requires (checked by the caller, grb_kron_ops.cpp): A.nrows B.nrows and A.ncols B.ncols <= GRB_DIM_DEVICE_MAX, A.nnz B.nnz <= KRON_MAX_ENTRIES.
// `fill_ms`: when given, the device time of the fill kernel alone (HIP events around its launch; 0 for an empty product) — tools/kron_probe.py.
void kron_csr(int code, int opcode, const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T, float* fill_ms = nullptr);

}  // namespace grb
