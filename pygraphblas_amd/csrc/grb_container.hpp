// grb_container.hpp — what the files of the object model share beyond grb_internal.hpp's "containers" block (which every operation includes):
//   grb_container.cpp   the extern "C" object surface and the typed families
//   grb_mirror.cpp      host assemble, the image transitions, upload / download of both images
//   grb_edit_ops.cpp    the HBM edit queue, its flushes, element set / get / remove
//   grb_build_ops.cpp   build from tuples        grb_tuples_ops.cpp   extractTuples
#pragma once
#include "grb_api.hpp"
#include "grb_device.hpp"
#include <utility>

#define CHECK_MAT(A) do { if (!(A)) return GrB_NULL_POINTER; if (!check_obj(A)) return GrB_UNINITIALIZED_OBJECT; } while (0)
#define CHECK_VEC(v) CHECK_MAT(v)

namespace grb {

inline constexpr const char* ISO_MSG = "a full one-valued container of this dimension can be read element-wise only";

// ---- grb_mirror.cpp ----------------------------------------------------------------------------------------------------------------------------------
void mat_structure_changed(GrB_Matrix A);   // rows, columns or the entry set of the device CSR changed (the structural flush, resize)
void mat_values_changed(GrB_Matrix A);      // values of the device CSR were overwritten in place (mat_set, the values-only flush)
// a device CSR filled from / copied out to three arrays on either side (`kind`).  Copies only: `valid` and the synchronisation are the caller's.
void csr_upload(DevCSR& c, uint64_t nrows, uint64_t ncols, uint64_t nnz, const uint32_t* rowptr, const uint32_t* col, const void* val, size_t ts, hipMemcpyKind kind);
void csr_download(const DevCSR& c, uint32_t* rowptr, uint32_t* col, void* val, size_t ts, hipMemcpyKind kind);      // (a null array is skipped)
void bitmap_copy(DevBitmap& d, const DevBitmap& s, size_t np, size_t ts);      // the bitmap form of a batch matrix (np positions), device to device, no wait
std::pair<DevBuf, DevBuf> vec_alloc_image(uint64_t n, size_t ts, bool zero);      // the (val, pres) buffers of an n-vector's bitmap, zeroed on request
// one element between an image and the thread's pinned scratch (past the first 64 bytes, where the counters' read-backs land): the copy and the wait for it
inline uint8_t* elem_scratch() { return (uint8_t*)pinned_scratch() + 64; }
void elem_peek(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);

// ---- grb_edit_ops.cpp --------------------------------------------------------------------------------------------------------------------------------
bool mat_edit_route(GrB_Matrix A);          // element edits of A are queued for the device
bool vec_edit_route(GrB_Vector v);
GrB_Info mat_set(GrB_Matrix C, const void* x, int xcode, GrB_Index i, GrB_Index j);
GrB_Info mat_get(void* x, int xcode, GrB_Matrix A, GrB_Index i, GrB_Index j);
GrB_Info vec_set(GrB_Vector w, const void* x, int xcode, GrB_Index i);
GrB_Info vec_get(void* x, int xcode, GrB_Vector v, GrB_Index i);
// The plan string of a flush goes IN FRONT of what the plan holds: most flushes run inside an operation (mat_to_device / mat_nvals / vec_gate of its operands and
// output), whose own plan stays behind it.  The entry points that are flush points of their own (nvals, wait, dup, extractElement, extractTuples) start from an
// empty plan when edits are queued.  True: they were.
inline bool flush_point(GrB_Matrix A) { const bool queued = mat_edits_queued(A); if (queued) g_last_plan.clear(); return queued; }
inline bool flush_point(GrB_Vector v) { const bool queued = vec_edits_queued(v); if (queued) g_last_plan.clear(); return queued; }

// ---- grb_build_ops.cpp, grb_tuples_ops.cpp -----------------------------------------------------------------------------------------------------------
GrB_Info mat_build(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const void* X, int xcode, GrB_Index n, GrB_BinaryOp dup, int location = 0);
GrB_Info vec_build(GrB_Vector w, const GrB_Index* I, const void* X, int xcode, GrB_Index n, GrB_BinaryOp dup, int location = 0);
GrB_Info mat_tuples(GrB_Index* I, GrB_Index* J, void* X, int xcode, GrB_Index* n, GrB_Matrix A);
GrB_Info vec_tuples(GrB_Index* I, void* X, int xcode, GrB_Index* n, GrB_Vector v);

}  // namespace grb
