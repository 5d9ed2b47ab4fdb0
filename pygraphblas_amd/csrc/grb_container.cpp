// grb_container.cpp — GrB_Matrix / GrB_Vector / GxB_Scalar objects: the extern "C" object surface.
//
// Replaces the object-model half of the `lib.` surface that pygraphblas calls:
//   GrB_Matrix_new/free/dup/clear/nrows/ncols/nvals/wait/error/resize/removeElement
//        (reference call sites: pygraphblas/matrix.py:99-117, 171-175, 627-760, 3353)
//   GrB_Matrix_build_<T> / setElement_<T> / extractElement_<T> / extractTuples_<T>
//        (pygraphblas/matrix.py:325-330, 1503-1529, 3180-3308; types.py:87-110)
//   the Vector and Scalar equivalents (pygraphblas/vector.py:60-95, scalar.py:20-92).
// Ownership: the library allocates in *_new and frees in *_free(&h); free of NULL / already freed
// handles is a successful no-op (reference __del__ checks the return code).
// What is behind the surface: the two images and the way between them (grb_mirror.cpp), element edits (grb_edit_ops.cpp), build (grb_build_ops.cpp),
// extractTuples (grb_tuples_ops.cpp); grb_container.hpp declares what these files share.
#include "grb_container.hpp"
#include "grb_matops.hpp"
#include "grb_edit.hpp"
#include <algorithm>
#include <tuple>
#include <string.h>
#include <stdarg.h>

using namespace grb;

extern "C" {

// =================================== Matrix ========================================================
GrB_Info GrB_Matrix_new(GrB_Matrix* A, GrB_Type type, GrB_Index nrows, GrB_Index ncols) {
  if (!A) return GrB_NULL_POINTER; *A = nullptr;
  if (!check_obj(type)) return GrB_UNINITIALIZED_OBJECT;
  if (type->code >= T_UDT) return GrB_DOMAIN_MISMATCH;    // user types: out of scope; complex: host-side containers only
  if (nrows > GXB_INDEX_MAX || ncols > GXB_INDEX_MAX) return GrB_INVALID_VALUE;
  auto* m = new (std::nothrow) GrB_Matrix_opaque(); if (!m) return GrB_OUT_OF_MEMORY;
  m->type = type; m->nrows = nrows; m->ncols = ncols; *A = m; return GrB_SUCCESS;
}
GrB_Info GrB_Matrix_free(GrB_Matrix* A) {
  if (!A || !*A) return GrB_SUCCESS;
  if (check_obj(*A)) { (*A)->magic = GRB_FREED; delete *A; }
  *A = nullptr; return GrB_SUCCESS;
}
GrB_Info GrB_Matrix_dup(GrB_Matrix* C, const GrB_Matrix A) {
  if (!C) return GrB_NULL_POINTER; CHECK_MAT(A);
  GrB_Matrix m = nullptr; GrB_Info info = GrB_Matrix_new(&m, A->type, A->nrows, A->ncols); if (info) return info;
  info = guarded(A, [&] {
    flush_point(A);
    m->format = A->format; m->sparsity_control = A->sparsity_control; m->hyper_switch = A->hyper_switch;
    if (A->iso_full) { m->iso_full = true; memcpy(m->iso_val, A->iso_val, 16); }
    else if (A->host_valid) { mat_host_assemble(A); m->hi = A->hi; m->hj = A->hj; m->hx = A->hx; m->host_valid = true; }
    else if (mat_bitmap_only(A)) {                             // a batch matrix that lives as a bitmap: so does its copy
      bitmap_copy(m->bm, A->bm, (size_t)A->nrows * A->ncols, A->type->size);
      m->host_valid = false; m->dev_valid = false;
    } else {
      mat_edit_flush(A);
      const DevCSR& s = A->csr;
      csr_upload(m->csr, s.nrows, s.ncols, s.nnz, s.rowptr.as<uint32_t>(), s.col.as<uint32_t>(), s.val.p, A->type->size, hipMemcpyDeviceToDevice);      // (stream order is enough: no wait)
      m->csr.valid = true; m->dev_valid = true; m->host_valid = false;
    }
  });
  if (info) { GrB_Matrix_free(&m); return info; }
  *C = m; return GrB_SUCCESS;
}
GrB_Info GrB_Matrix_clear(GrB_Matrix A) {
  CHECK_MAT(A); A->hi.clear(); A->hj.clear(); A->hx.clear(); A->pending.clear(); A->host_valid = true; A->iso_full = false; mat_invalidate_device(A); return GrB_SUCCESS;
}
GrB_Info GrB_Matrix_nrows(GrB_Index* n, const GrB_Matrix A) { if (!n) return GrB_NULL_POINTER; CHECK_MAT(A); *n = A->nrows; return GrB_SUCCESS; }
GrB_Info GrB_Matrix_ncols(GrB_Index* n, const GrB_Matrix A) { if (!n) return GrB_NULL_POINTER; CHECK_MAT(A); *n = A->ncols; return GrB_SUCCESS; }
GrB_Info GrB_Matrix_nvals(GrB_Index* n, const GrB_Matrix A) {
  if (!n) return GrB_NULL_POINTER; CHECK_MAT(A); return guarded(A, [&] { flush_point(A); *n = mat_nvals(A); });
}
GrB_Info GrB_Matrix_wait(GrB_Matrix* A) {
  if (!A) return GrB_NULL_POINTER; CHECK_MAT(*A);
  return guarded(*A, [&] { if ((*A)->host_valid && !(*A)->iso_full) mat_host_assemble(*A); flush_point(*A); mat_edit_flush(*A); if (device_ok()) GRB_HIP(hipStreamSynchronize(stream())); });
}
// the reference asks `self` for the message even when the failing object was the output (pygraphblas/matrix.py:43-51)
GrB_Info GrB_Matrix_error(const char** s, const GrB_Matrix A) { if (!s) return GrB_NULL_POINTER; CHECK_MAT(A); *s = A->err.empty() ? g_last_error.c_str() : A->err.c_str(); return GrB_SUCCESS; }
GrB_Info GxB_Matrix_type(GrB_Type* t, const GrB_Matrix A) { if (!t) return GrB_NULL_POINTER; CHECK_MAT(A); *t = A->type; return GrB_SUCCESS; }
GrB_Info GrB_Matrix_resize(GrB_Matrix A, GrB_Index nr, GrB_Index nc) {
  CHECK_MAT(A); if (nr > GXB_INDEX_MAX || nc > GXB_INDEX_MAX) return GrB_INVALID_VALUE;
  return guarded(A, [&] {
    if (mat_edit_route(A) && nr <= GRB_DIM_DEVICE_MAX && nc <= GRB_DIM_DEVICE_MAX) {      // it lives in HBM and stays there (a dimension beyond the device range: the host route below)
      mat_edit_flush(A);
      const size_t ts = A->type->size; const uint32_t nr32 = (uint32_t)nr, nc32 = (uint32_t)nc;
      const bool changed = nr32 != A->csr.nrows || nc32 != A->csr.ncols;
      if (nr32 != A->csr.nrows) {                            // fewer rows: the row pointer truncated; more: extended with its last word.  The entries stay where they are.
        DevCSR t; t.nrows = nr32; t.ncols = A->csr.ncols;
        t.nnz = csr_resize_rowptr(A->csr, nr32, t.rowptr);
        t.col = std::move(A->csr.col); t.val = std::move(A->csr.val); t.valid = true;
        A->csr = std::move(t);
      }
      if (nc32 < A->csr.ncols && A->csr.nnz) {               // fewer columns: keep bytes, then the compaction every select uses
        DevBuf keep(A->csr.nnz + 16); DevCSR t;
        csr_keep_cols_below(A->csr, nc32, keep.as<uint8_t>());
        csr_compact(A->csr, A->csr.val.p, ts, keep.as<uint8_t>(), t);
        A->csr = std::move(t);
      }
      A->csr.ncols = nc32;
      if (changed) mat_structure_changed(A);
      A->nrows = nr; A->ncols = nc;
      g_last_plan = "resize<on=matrix,rows=" + std::to_string(nr) + ",cols=" + std::to_string(nc) + "> ";
      return;
    }
    mat_to_host(A); const size_t ts = A->type->size; size_t w = 0;
    for (size_t k = 0; k < A->hi.size(); k++) if (A->hi[k] < nr && A->hj[k] < nc) {
      if (w != k) { A->hi[w] = A->hi[k]; A->hj[w] = A->hj[k]; memmove(&A->hx[w * ts], &A->hx[k * ts], ts); } w++; }
    A->hi.resize(w); A->hj.resize(w); A->hx.resize(w * ts); A->nrows = nr; A->ncols = nc; mat_invalidate_device(A);
  });
}
double GxB_ALWAYS_HYPER = 1.0, GxB_NEVER_HYPER = -1.0, GxB_HYPER_DEFAULT = 0.0625;      // hyper_switch settings (stored options only)
GrB_Info GxB_Matrix_Option_set(GrB_Matrix A, int field, ...) {
  CHECK_MAT(A); va_list ap; va_start(ap, field); GrB_Info info = GrB_SUCCESS;
  switch (field) {
    case 1: A->format = va_arg(ap, int); break;
    case 0: A->hyper_switch = va_arg(ap, double); break;
    case 32: A->sparsity_control = va_arg(ap, int); break;
    case 34: (void)va_arg(ap, double); break;
    default: info = GrB_INVALID_VALUE;
  }
  va_end(ap); return info;
}
GrB_Info GxB_Matrix_Option_get(GrB_Matrix A, int field, ...) {
  CHECK_MAT(A); va_list ap; va_start(ap, field); GrB_Info info = GrB_SUCCESS;
  switch (field) {
    case 1: { int* p = va_arg(ap, int*); if (p) *p = A->format; break; }
    case 0: { double* p = va_arg(ap, double*); if (p) *p = A->hyper_switch; break; }
    case 32: { int* p = va_arg(ap, int*); if (p) *p = A->sparsity_control; break; }
    case 33: { int* p = va_arg(ap, int*); uint64_t nv = 1; if (!A->iso_full) info = guarded(A, [&] { nv = mat_nvals(A); }); if (p) *p = A->iso_full ? 8 : (A->nrows > GRB_DIM_DEVICE_MAX || A->hyper_switch >= 1.0 || nv == 0) ? 1 : 2; break; }  // what SuiteSparse would report: hypersparse for huge or empty matrices and under hyper_switch = GxB_ALWAYS_HYPER (a stored option here), else sparse
    case 34: { double* p = va_arg(ap, double*); if (p) *p = 0.04; break; }
    default: info = GrB_INVALID_VALUE;
  }
  va_end(ap); return info;
}
GrB_Info GxB_Matrix_memoryUsage(size_t* size, const GrB_Matrix A) {
  if (!size) return GrB_NULL_POINTER; CHECK_MAT(A);
  *size = sizeof(*A) + A->hi.capacity() * 16 + A->hx.capacity() + A->csr.rowptr.bytes + A->csr.col.bytes + A->csr.val.bytes +
          A->csc.rowptr.bytes + A->csc.col.bytes + A->csc.val.bytes; return GrB_SUCCESS;
}

// =================================== Vector ========================================================
GrB_Info GrB_Vector_new(GrB_Vector* v, GrB_Type type, GrB_Index n) {
  if (!v) return GrB_NULL_POINTER; *v = nullptr;
  if (!check_obj(type)) return GrB_UNINITIALIZED_OBJECT;
  if (type->code >= T_UDT) return GrB_DOMAIN_MISMATCH;
  if (n > GXB_INDEX_MAX) return GrB_INVALID_VALUE;
  auto* w = new (std::nothrow) GrB_Vector_opaque(); if (!w) return GrB_OUT_OF_MEMORY;
  w->type = type; w->n = n; *v = w; return GrB_SUCCESS;
}
GrB_Info GrB_Vector_free(GrB_Vector* v) {
  if (!v || !*v) return GrB_SUCCESS;
  if (check_obj(*v)) {
    if ((*v)->lazy | (*v)->q_reads) { GrB_Vector x = *v; (void)guarded(x, [&] { vec_overwritten(x); }); }   // deferred work that reads it runs first; work that only wrote it is dropped
    (*v)->magic = GRB_FREED; delete *v; }
  *v = nullptr; return GrB_SUCCESS;
}
GrB_Info GrB_Vector_dup(GrB_Vector* w, const GrB_Vector u) {
  if (!w) return GrB_NULL_POINTER; CHECK_VEC(u);
  GrB_Vector r = nullptr; GrB_Info info = GrB_Vector_new(&r, u->type, u->n); if (info) return info;
  info = guarded(u, [&] {
    flush_point(u);
    vec_gate(u);
    if (u->iso_full) { r->iso_full = true; memcpy(r->iso_val, u->iso_val, 16); }
    else if (u->host_valid) { vec_host_assemble(u); r->hi = u->hi; r->hx = u->hx; }
    else {
      const size_t ts = u->type->size;
      std::tie(r->dval, r->dpres) = vec_alloc_image(u->n, ts, false);
      if (u->n) dev_copy2(r->dval.p, u->dval.p, u->n * ts, r->dpres.p, u->dpres.p, u->n);
      r->facts.image_replaced(u->facts.dnvals, u->facts.dnvals_known); r->dev_valid = true; r->host_valid = false;
    }
  });
  if (info) { GrB_Vector_free(&r); return info; }
  *w = r; return GrB_SUCCESS;
}
GrB_Info GrB_Vector_clear(GrB_Vector v) { CHECK_VEC(v); if (v->lazy | v->q_reads) { GrB_Info e = guarded(v, [&] { vec_overwritten(v); }); if (e) return e; } v->hi.clear(); v->hx.clear(); v->pending.clear(); v->host_valid = true; v->iso_full = false; vec_invalidate_device(v); return GrB_SUCCESS; }
GrB_Info GrB_Vector_size(GrB_Index* n, const GrB_Vector v) { if (!n) return GrB_NULL_POINTER; CHECK_VEC(v); *n = v->n; return GrB_SUCCESS; }
GrB_Info GrB_Vector_nvals(GrB_Index* n, const GrB_Vector v) { if (!n) return GrB_NULL_POINTER; CHECK_VEC(v); return guarded(v, [&] { flush_point(v); *n = vec_nvals(v); }); }
GrB_Info GrB_Vector_wait(GrB_Vector* v) {
  if (!v) return GrB_NULL_POINTER; CHECK_VEC(*v);
  return guarded(*v, [&] { flush_point(*v); vec_gate(*v); if ((*v)->host_valid) vec_host_assemble(*v); if (device_ok()) GRB_HIP(hipStreamSynchronize(stream())); });
}
GrB_Info GrB_Vector_error(const char** s, const GrB_Vector v) { if (!s) return GrB_NULL_POINTER; CHECK_VEC(v); *s = v->err.empty() ? g_last_error.c_str() : v->err.c_str(); return GrB_SUCCESS; }
GrB_Info GxB_Vector_type(GrB_Type* t, const GrB_Vector v) { if (!t) return GrB_NULL_POINTER; CHECK_VEC(v); *t = v->type; return GrB_SUCCESS; }
GrB_Info GrB_Vector_resize(GrB_Vector v, GrB_Index n) {
  CHECK_VEC(v); if (n > GXB_INDEX_MAX) return GrB_INVALID_VALUE;
  return guarded(v, [&] {
    if (!v->host_valid) vec_gate(v);
    if (vec_edit_route(v) && n <= GRB_DIM_DEVICE_MAX) {       // it lives in HBM and stays there: a new bitmap, the common prefix copied, the tail zero
      const size_t ts = v->type->size; const uint64_t keep = std::min<uint64_t>(n, v->n);
      if (n != v->n) {
        auto [nval, npres] = vec_alloc_image(n, ts, false);
        if (keep) dev_copy2(nval.p, v->dval.p, keep * ts, npres.p, v->dpres.p, keep);
        if (n > keep) { GRB_HIP(hipMemsetAsync((uint8_t*)nval.p + keep * ts, 0, (n - keep) * ts, stream())); GRB_HIP(hipMemsetAsync(npres.as<uint8_t>() + keep, 0, n - keep, stream())); }
        v->facts.image_replaced(v->facts.dnvals, v->facts.dnvals_known && n >= v->n);      // (a longer vector holds what it held)
        v->dval = std::move(nval); v->dpres = std::move(npres); v->dcode.reset(); v->n = n;
      }
      g_last_plan = "resize<on=vector,rows=" + std::to_string(n) + ",cols=1> ";
      return;
    }
    vec_to_host(v); const size_t ts = v->type->size; size_t w = 0;
    while (w < v->hi.size() && v->hi[w] < n) w++;
    v->hi.resize(w); v->hx.resize(w * ts); v->n = n; vec_invalidate_device(v); });
}
GrB_Info GxB_Vector_Option_set(GrB_Vector v, int field, ...) {
  CHECK_VEC(v); va_list ap; va_start(ap, field); GrB_Info info = GrB_SUCCESS;
  switch (field) { case 32: v->sparsity_control = va_arg(ap, int); break; case 34: (void)va_arg(ap, double); break;
                   case 1: (void)va_arg(ap, int); break; case 0: (void)va_arg(ap, double); break; default: info = GrB_INVALID_VALUE; }
  va_end(ap); return info;
}
GrB_Info GxB_Vector_Option_get(GrB_Vector v, int field, ...) {
  CHECK_VEC(v); va_list ap; va_start(ap, field); GrB_Info info = GrB_SUCCESS;
  switch (field) {
    case 32: { int* p = va_arg(ap, int*); if (p) *p = v->sparsity_control; break; }
    case 33: { int* p = va_arg(ap, int*); (void)guarded(v, [&] { vec_gate(v); }); if (p) *p = v->dev_valid && !v->host_valid ? (vec_dev_nvals(v) == v->n ? 8 : 4) : 2; break; }
    case 1: { int* p = va_arg(ap, int*); if (p) *p = 1; break; }
    case 34: { double* p = va_arg(ap, double*); if (p) *p = 0.04; break; }
    default: info = GrB_INVALID_VALUE;
  }
  va_end(ap); return info;
}
GrB_Info GxB_Vector_memoryUsage(size_t* size, const GrB_Vector v) {
  if (!size) return GrB_NULL_POINTER; CHECK_VEC(v); *size = sizeof(*v) + v->hi.capacity() * 8 + v->hx.capacity() + v->dval.bytes + v->dpres.bytes; return GrB_SUCCESS;
}

// =================================== Scalar ========================================================
GrB_Info GxB_Scalar_new(GxB_Scalar* s, GrB_Type type) {
  if (!s) return GrB_NULL_POINTER; *s = nullptr; if (!check_obj(type)) return GrB_UNINITIALIZED_OBJECT;
  if (type->code >= T_UDT) return GrB_DOMAIN_MISMATCH;
  auto* r = new (std::nothrow) GxB_Scalar_opaque(); if (!r) return GrB_OUT_OF_MEMORY; r->type = type; *s = r; return GrB_SUCCESS;
}
GrB_Info GxB_Scalar_dup(GxB_Scalar* s, const GxB_Scalar t) {
  if (!s) return GrB_NULL_POINTER; CHECK_MAT(t); auto* r = new (std::nothrow) GxB_Scalar_opaque(); if (!r) return GrB_OUT_OF_MEMORY;
  r->type = t->type; r->has = t->has; memcpy(r->x, t->x, 16); *s = r; return GrB_SUCCESS;
}
GrB_Info GxB_Scalar_clear(GxB_Scalar s) { CHECK_MAT(s); s->has = false; return GrB_SUCCESS; }
GrB_Info GxB_Scalar_free(GxB_Scalar* s) { if (!s || !*s) return GrB_SUCCESS; if (check_obj(*s)) { (*s)->magic = GRB_FREED; delete *s; } *s = nullptr; return GrB_SUCCESS; }
GrB_Info GxB_Scalar_nvals(GrB_Index* n, const GxB_Scalar s) { if (!n) return GrB_NULL_POINTER; CHECK_MAT(s); *n = s->has ? 1 : 0; return GrB_SUCCESS; }
GrB_Info GxB_Scalar_wait(GxB_Scalar* s) { if (!s) return GrB_NULL_POINTER; CHECK_MAT(*s); return GrB_SUCCESS; }
GrB_Info GxB_Scalar_type(GrB_Type* t, const GxB_Scalar s) { if (!t) return GrB_NULL_POINTER; CHECK_MAT(s); *t = s->type; return GrB_SUCCESS; }
static GrB_Info scalar_set(GxB_Scalar s, const void* x, int xcode) { CHECK_MAT(s); cast_scalar(s->type->code, s->x, xcode, x); s->has = true; return GrB_SUCCESS; }
static GrB_Info scalar_get(void* x, int xcode, GxB_Scalar s) { if (!x) return GrB_NULL_POINTER; CHECK_MAT(s); if (!s->has) return GrB_NO_VALUE; cast_scalar(xcode, x, s->type->code, s->x); return GrB_SUCCESS; }

// ---- typed families: PRE is GrB for the 11 real types, GxB for the complex ones (the Scalar is GxB for all) -------------------------
#define GRB_TYPED_CONTAINER(PRE, SUF, CT, CODE) \
  GrB_Info PRE##_Matrix_build_##SUF(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const CT* X, GrB_Index n, const GrB_BinaryOp dup) { return mat_build(C, I, J, X, CODE, n, dup); } \
  GrB_Info PRE##_Matrix_setElement_##SUF(GrB_Matrix C, CT x, GrB_Index i, GrB_Index j) { return mat_set(C, &x, CODE, i, j); } \
  GrB_Info PRE##_Matrix_extractElement_##SUF(CT* x, const GrB_Matrix A, GrB_Index i, GrB_Index j) { return mat_get(x, CODE, A, i, j); } \
  GrB_Info PRE##_Matrix_extractTuples_##SUF(GrB_Index* I, GrB_Index* J, CT* X, GrB_Index* n, const GrB_Matrix A) { return mat_tuples(I, J, X, CODE, n, A); } \
  GrB_Info PRE##_Vector_build_##SUF(GrB_Vector w, const GrB_Index* I, const CT* X, GrB_Index n, const GrB_BinaryOp dup) { return vec_build(w, I, X, CODE, n, dup); } \
  GrB_Info PRE##_Vector_setElement_##SUF(GrB_Vector w, CT x, GrB_Index i) { return vec_set(w, &x, CODE, i); } \
  GrB_Info PRE##_Vector_extractElement_##SUF(CT* x, const GrB_Vector v, GrB_Index i) { return vec_get(x, CODE, v, i); } \
  GrB_Info PRE##_Vector_extractTuples_##SUF(GrB_Index* I, CT* X, GrB_Index* n, const GrB_Vector v) { return vec_tuples(I, X, CODE, n, v); } \
  GrB_Info GxB_Scalar_setElement_##SUF(GxB_Scalar s, CT x) { return scalar_set(s, &x, CODE); } \
  GrB_Info GxB_Scalar_extractElement_##SUF(CT* x, const GxB_Scalar s) { return scalar_get(x, CODE, s); }
GRB_TYPED_CONTAINER(GrB, BOOL, bool, T_BOOL) GRB_TYPED_CONTAINER(GrB, INT8, int8_t, T_INT8) GRB_TYPED_CONTAINER(GrB, UINT8, uint8_t, T_UINT8)
GRB_TYPED_CONTAINER(GrB, INT16, int16_t, T_INT16) GRB_TYPED_CONTAINER(GrB, UINT16, uint16_t, T_UINT16) GRB_TYPED_CONTAINER(GrB, INT32, int32_t, T_INT32)
GRB_TYPED_CONTAINER(GrB, UINT32, uint32_t, T_UINT32) GRB_TYPED_CONTAINER(GrB, INT64, int64_t, T_INT64) GRB_TYPED_CONTAINER(GrB, UINT64, uint64_t, T_UINT64)
GRB_TYPED_CONTAINER(GrB, FP32, float, T_FP32) GRB_TYPED_CONTAINER(GrB, FP64, double, T_FP64)

// complex entries: stored, set, read and listed on the host mirror (the reference's type registry, from_lists with
// complex values and Matrix.dense(FC64) need that much: tests/test_matrix.py:56-57,853); arithmetic on them is not offered
typedef struct { float re, im; } GxB_FC32_t;
typedef struct { double re, im; } GxB_FC64_t;
GRB_TYPED_CONTAINER(GxB, FC32, GxB_FC32_t, T_FC32) GRB_TYPED_CONTAINER(GxB, FC64, GxB_FC64_t, T_FC64)

// =================================== bulk / device import-export ===================================
GrB_Info GrBX_Matrix_import_CSR(GrB_Matrix* A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, GrB_Index nvals,
                                const uint32_t* rowptr, const uint32_t* colidx, const void* values, int location) {
  if (!A || !rowptr || (nvals && (!colidx || !values))) return GrB_NULL_POINTER;
  GrB_Matrix m = nullptr; GrB_Info info = GrB_Matrix_new(&m, type, nrows, ncols); if (info) return info;
  info = guarded(m, [&] {
    need_device();
    if (nrows > GRB_DIM_DEVICE_MAX || ncols > GRB_DIM_DEVICE_MAX || nvals > 0xFFFFFFF0ull) fail(GrB_INSUFFICIENT_SPACE, "import_CSR: 32-bit index range exceeded");
    csr_upload(m->csr, nrows, ncols, nvals, rowptr, colidx, values, type->size, location ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    GRB_HIP(hipStreamSynchronize(stream()));
    m->csr.valid = true; m->dev_valid = true; m->host_valid = false;
  });
  if (info) { GrB_Matrix_free(&m); return info; }
  *A = m; return GrB_SUCCESS;
}
GrB_Info GrBX_Matrix_export_CSR(const GrB_Matrix A, uint32_t* rowptr, uint32_t* colidx, void* values, int location) {
  CHECK_MAT(A);
  return guarded(A, [&] {
    mat_to_device(A);
    csr_download(A->csr, rowptr, colidx, values, A->type->size, location ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    GRB_HIP(hipStreamSynchronize(stream()));
  });
}
GrB_Info GrBX_Vector_import_Bitmap(GrB_Vector* v, GrB_Type type, GrB_Index n, const void* values, const uint8_t* present, int location) {
  if (!v || (n && !values)) return GrB_NULL_POINTER;
  GrB_Vector w = nullptr; GrB_Info info = GrB_Vector_new(&w, type, n); if (info) return info;
  info = guarded(w, [&] {
    need_device(); if (n > GRB_DIM_DEVICE_MAX) fail(GrB_INSUFFICIENT_SPACE, "import: vector too long");
    const size_t ts = type->size; hipMemcpyKind k = location ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    std::tie(w->dval, w->dpres) = vec_alloc_image(n, ts, false);
    if (n) {
      GRB_HIP(hipMemcpyAsync(w->dval.p, values, n * ts, k, stream()));
      if (present) GRB_HIP(hipMemcpyAsync(w->dpres.p, present, n, k, stream()));
      else GRB_HIP(hipMemsetAsync(w->dpres.p, 1, n, stream()));
    }
    w->dev_valid = true; w->host_valid = false;
    w->facts.image_replaced(n, !present);
    GRB_HIP(hipStreamSynchronize(stream()));
  });
  if (info) { GrB_Vector_free(&w); return info; }
  *v = w; return GrB_SUCCESS;
}
GrB_Info GrBX_Vector_import_Full(GrB_Vector* v, GrB_Type type, GrB_Index n, const void* values, int location) {
  return GrBX_Vector_import_Bitmap(v, type, n, values, nullptr, location);
}
GrB_Info GrBX_Vector_export_Bitmap(const GrB_Vector v, void* values, uint8_t* present, int location) {
  CHECK_VEC(v);
  return guarded(v, [&] {
    vec_to_device(v); const size_t ts = v->type->size; hipMemcpyKind k = location ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (values && v->n) GRB_HIP(hipMemcpyAsync(values, v->dval.p, v->n * ts, k, stream()));
    if (present && v->n) GRB_HIP(hipMemcpyAsync(present, v->dpres.p, v->n, k, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  });
}
GrB_Info GrBX_Vector_device_view(GrB_Vector v, void** values, uint8_t** present, GrB_Index* nvals) {
  CHECK_VEC(v);
  return guarded(v, [&] { vec_to_device(v); if (values) *values = v->dval.p; if (present) *present = v->dpres.as<uint8_t>(); if (nvals) *nvals = vec_dev_nvals(v); });
}
GrB_Info GrBX_Vector_device_touch(GrB_Vector v) {
  CHECK_VEC(v);
  return guarded(v, [&] { if (!v->dev_valid) fail(GrB_INVALID_VALUE, "device_touch: vector has no device view");
    vec_device_extended(v); });      // (the caller wrote through the view: the count is void, the edge bound stays — a stale one can only cost speed)
}

}  // extern "C"
