// grb_edit.hpp — host interface of the in-place edit kernels (grb_edit.hip): a normalised list of element edits applied to a CSR or a vector bitmap in HBM,
// and the pieces of a resize that stays in HBM.  The list arithmetic is in grb_edit_list.hpp; the queue and its flushes are in grb_edit_ops.cpp.
#pragma once
#include "grb_internal.hpp"

namespace grb {

struct EditCounts { uint32_t set = 0, ins = 0, del = 0; };      // overwrites of stored entries, new entries, removed entries (the delete of an absent entry counts nowhere)

// k >= 1 edits in (row, column) order, one per coordinate, all inside A: ei / ej / del (1 = remove) / x (k values of `ts` bytes), host arrays.
// No insert and no delete among them: the values are stored into A.val in place and *structural = false (`out` untouched).  Otherwise `out` is the edited
// matrix in new buffers (A untouched) and *structural = true.
EditCounts csr_apply_edits(const DevCSR& A, size_t ts, uint32_t k, const uint32_t* ei, const uint32_t* ej, const uint8_t* del, const uint8_t* x, DevCSR& out, bool* structural);

// the same on a vector bitmap of n positions: val[idx[e]] = x[e], pres[idx[e]] = 1, or pres[idx[e]] = 0 for a remove; idx strictly increasing, all < n
void vec_apply_edits(size_t ts, uint64_t n, uint32_t k, const uint32_t* idx, const uint8_t* del, const uint8_t* x, void* val, uint8_t* pres);

// ---- resize ---------------------------------------------------------------------------------------------------------------------------------
void csr_keep_cols_below(const DevCSR& A, uint32_t ncols, uint8_t* keep);      // keep[p] = col[p] < ncols (the flags csr_compact takes)
// the row pointer of A for nrows_new rows: its first words, then (more rows) its last word repeated.  Returns the entry count of the new row range — read back
// (4 bytes) when rows go, A.nnz otherwise.
uint64_t csr_resize_rowptr(const DevCSR& A, uint32_t nrows_new, DevBuf& rowptr_new);

}  // namespace grb
