// grb_edit_ops.cpp — one element at a time: setElement / extractElement / removeElement of matrices and vectors, and the edit queue of a container that
// lives in HBM only with its two flushes (the list arithmetic: grb_edit_list.hpp; the kernels: grb_edit.hip).
#include "grb_container.hpp"
#include "grb_matops.hpp"
#include "grb_edit.hpp"
#include "grb_edit_list.hpp"
#include <algorithm>
#include <string.h>

namespace grb {

// ---- the edit queue of a container that lives in HBM only ------------------------------------------------------------------------------
// `A[i, j] = x`, `del A[i, j]`, `v[i] = x` on a container whose only valid image is the HBM one append today's Pending record and nothing else: no download, nothing
// invalidated.  The queue is applied on the device (grb_edit.hip) before anything reads or replaces that image: mat_to_device / mat_to_host / mat_nvals / dup / wait /
// resize for matrices, vec_gate (which every reader of a vector passes) for vectors; extractElement looks in the queue first.  Whoever replaces the image as a whole
// clears `pending` (mat_invalidate_host, GrB_Matrix_clear, the vector drivers).  GRB_MI355X_EDIT=0 forces the host route everywhere.
// (Where the plan string of a flush goes: flush_point, grb_container.hpp.)
bool mat_edit_route(GrB_Matrix A) {
  return A->dev_valid && !A->host_valid && !A->iso_full && A->csr.valid && A->type->code < T_FC32 && A->nrows <= GRB_DIM_DEVICE_MAX && A->ncols <= GRB_DIM_DEVICE_MAX &&
         device_ok() && route_env("GRB_MI355X_EDIT") != 0;
}
bool vec_edit_route(GrB_Vector v) {
  return v->dev_valid && !v->host_valid && !v->iso_full && v->lazy == 0 && v->q_reads == 0 && v->type->code < T_FC32 && v->n <= GRB_DIM_DEVICE_MAX && device_ok() &&
         route_env("GRB_MI355X_EDIT") != 0;
}
void mat_edit_flush(GrB_Matrix A) {
  if (!mat_edits_queued(A)) return;
  if (!A->dev_valid || !A->csr.valid) fail(GrB_PANIC, "edit: queued element edits without a device image");
  const size_t ts = A->type->size; auto& P = A->pending;
  const std::vector<uint32_t> ord = edit_normalise_ij(P);
  const uint32_t k = (uint32_t)ord.size();
  std::vector<uint32_t> ei(k), ej(k); std::vector<uint8_t> del(k), x((size_t)k * ts);
  for (uint32_t e = 0; e < k; e++) { const auto& r = P[ord[e]]; ei[e] = (uint32_t)r.i; ej[e] = (uint32_t)r.j; del[e] = r.del ? 1 : 0; memcpy(&x[(size_t)e * ts], r.x, ts); }
  DevCSR out; bool structural = false;
  const EditCounts n = csr_apply_edits(A->csr, ts, k, ei.data(), ej.data(), del.data(), x.data(), out, &structural);      // (neither csr_apply_edits nor anything it calls comes back here)
  P.clear(); P.shrink_to_fit();                              // only now: a flush that failed (allocation, launch, the entry-count limit) leaves the queue as it was, and the caller its error
  if (structural) { A->csr = std::move(out); mat_structure_changed(A); }
  else if (n.set) mat_values_changed(A);
  g_last_plan = "edit<on=matrix,set=" + std::to_string(n.set) + ",ins=" + std::to_string(n.ins) + ",del=" + std::to_string(n.del) + "> k_edit_locate " +
                (structural ? "k_edit_rowptr k_edit_stream k_edit_place " : n.set ? "k_edit_values " : "") + g_last_plan;
}
void vec_edit_flush(GrB_Vector v) {
  if (!vec_edits_queued(v)) return;
  if (!v->dev_valid) fail(GrB_PANIC, "edit: queued element edits without a device image");
  const size_t ts = v->type->size; auto& P = v->pending;
  const std::vector<uint32_t> ord = edit_normalise_i(P);
  const uint32_t k = (uint32_t)ord.size(); uint32_t nset = 0;
  std::vector<uint32_t> idx(k); std::vector<uint8_t> del(k), x((size_t)k * ts);
  for (uint32_t e = 0; e < k; e++) { const auto& r = P[ord[e]]; idx[e] = (uint32_t)r.i; del[e] = r.del ? 1 : 0; nset += r.del ? 0 : 1; memcpy(&x[(size_t)e * ts], r.x, ts); }
  v->facts.image_replaced(0, false);
  vec_apply_edits(ts, v->n, k, idx.data(), del.data(), x.data(), v->dval.p, v->dpres.as<uint8_t>());
  P.clear(); P.shrink_to_fit();                              // only now: a flush that failed leaves the queue as it was (the scatter stores the same bytes when it runs again)
  // (a bitmap store does not tell an overwrite from an insert: `set` counts both, `ins` is not known)
  g_last_plan = "edit<on=vector,set=" + std::to_string(nset) + ",ins=-,del=" + std::to_string(k - nset) + "> k_edit_vector " + g_last_plan;
}

// ---- matrix elements -------------------------------------------------------------------------------------------------------------------
// a matrix that lives in HBM only and is large (`paths[i, source] = 1` on a dense ns x n batch, gap/bcmark.py:23: bringing 134 MB to
// the host mirror for one value was a third of the algorithm): the entry is looked up on the device; an existing one is read or
// overwritten in place (what changes with the values — the transpose cache, a kernel-X plan's copy — is dropped)
// (a caller that touches many elements one by one is better served by the host mirror: one transfer, then no round trips)
static bool mat_device_only(GrB_Matrix A) { return A->dev_elem_ops++ < 32 && device_ok() && A->dev_valid && !A->host_valid && A->pending.empty() && !A->iso_full && A->csr.valid && A->csr.nnz >= (1u << 16) && A->type->code < T_FC32; }
GrB_Info mat_set(GrB_Matrix C, const void* x, int xcode, GrB_Index i, GrB_Index j) {
  CHECK_MAT(C); if (i >= C->nrows || j >= C->ncols) return GrB_INVALID_INDEX;
  return guarded(C, [&] {
    if (mat_device_only(C)) {
      const uint64_t pos = csr_find_entry(C->csr, (uint32_t)i, (uint32_t)j);
      if (pos != ~0ull) {
        uint8_t* pin = elem_scratch(); cast_scalar(C->type->code, pin, xcode, x);
        elem_peek((uint8_t*)C->csr.val.p + pos * C->type->size, pin, C->type->size, hipMemcpyHostToDevice);
        mat_values_changed(C);
        return;
      }
    }
    if (C->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
    GrB_Matrix_opaque::Pending p{i, j, false, {0}}; cast_scalar(C->type->code, p.x, xcode, x);
    if (mat_edit_route(C)) { C->pending.push_back(p); C->bm.clear(); return; }      // it lives in HBM (a new position, or edits are queued already: order is kept): queued for the device
    if (!C->host_valid) mat_to_host(C);
    C->pending.push_back(p); mat_invalidate_device(C);
  });
}
static size_t mat_find(GrB_Matrix A, GrB_Index i, GrB_Index j) {   // index into host tuples or SIZE_MAX
  const size_t p = tuples_lower_bound(A->hi, &A->hj, i, j);
  return tuples_hold(A->hi, &A->hj, p, i, j) ? p : SIZE_MAX;
}
GrB_Info mat_get(void* x, int xcode, GrB_Matrix A, GrB_Index i, GrB_Index j) {
  if (!x) return GrB_NULL_POINTER; CHECK_MAT(A); if (i >= A->nrows || j >= A->ncols) return GrB_INVALID_INDEX;
  GrB_Info r = GrB_SUCCESS;
  GrB_Info info = guarded(A, [&] {
    if (A->iso_full) { cast_scalar(xcode, x, A->type->code, A->iso_val); return; }
    if (mat_edits_queued(A)) {                                 // the last queued edit of the coordinate answers; else the device image does, edits applied
      if (const auto* e = edit_lookup(A->pending, [&](const GrB_Matrix_opaque::Pending& q) { return q.i == i && q.j == j; })) {
        if (e->del) r = GrB_NO_VALUE; else cast_scalar(xcode, x, A->type->code, e->x); return; }
      flush_point(A); mat_edit_flush(A);
    }
    if (mat_device_only(A)) {
      const uint64_t pos = csr_find_entry(A->csr, (uint32_t)i, (uint32_t)j);
      if (pos == ~0ull) { r = GrB_NO_VALUE; return; }
      uint8_t* pin = elem_scratch();
      elem_peek(pin, (const uint8_t*)A->csr.val.p + pos * A->type->size, A->type->size, hipMemcpyDeviceToHost);
      cast_scalar(xcode, x, A->type->code, pin); return;
    }
    mat_to_host(A); size_t k = mat_find(A, i, j);
    if (k == SIZE_MAX) r = GrB_NO_VALUE; else cast_scalar(xcode, x, A->type->code, &A->hx[k * A->type->size]); });
  return info ? info : r;
}

// ---- vector elements -------------------------------------------------------------------------------------------------------------------
GrB_Info vec_set(GrB_Vector w, const void* x, int xcode, GrB_Index i) {
  CHECK_VEC(w); if (i >= w->n) return GrB_INVALID_INDEX;
  return guarded(w, [&] { if (w->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
    GrB_Vector_opaque::Pending p{i, false, {0}}; cast_scalar(w->type->code, p.x, xcode, x);
    if (!w->host_valid) { if (w->lazy | w->q_reads) vec_resolve(w); if (vec_edit_route(w)) { w->pending.push_back(p); w->facts.image_replaced(0, false); return; } vec_to_host(w); }      // it lives in HBM (a deferred chain completed first): queued for the device
    w->pending.push_back(p); vec_invalidate_device(w); });
}
GrB_Info vec_get(void* x, int xcode, GrB_Vector v, GrB_Index i) {
  if (!x) return GrB_NULL_POINTER; CHECK_VEC(v); if (i >= v->n) return GrB_INVALID_INDEX;
  GrB_Info r = GrB_SUCCESS;
  GrB_Info info = guarded(v, [&] {
    if (v->iso_full) { cast_scalar(xcode, x, v->type->code, v->iso_val); return; }
    if (vec_edits_queued(v)) {                                 // the last queued edit of the position answers; else the device image does, edits applied (vec_gate)
      if (const auto* e = edit_lookup(v->pending, [&](const GrB_Vector_opaque::Pending& q) { return q.i == i; })) {
        if (e->del) r = GrB_NO_VALUE; else cast_scalar(xcode, x, v->type->code, e->x); return; }
      flush_point(v);
    }
    vec_gate(v);
    // a large vector that lives in HBM only (`r[vertex]` after a PageRank): the presence byte and the value come over alone — a few
    // dozen reads in a row, then the host mirror takes over (one transfer, no more round trips)
    if (device_ok() && v->dev_valid && !v->host_valid && v->pending.empty() && v->n >= (1u << 16) && v->type->code < T_FC32 && v->dev_elem_ops++ < 32) {
      uint8_t* pin = elem_scratch(); const size_t ts = v->type->size;
      GRB_HIP(hipMemcpyAsync(pin, v->dpres.as<uint8_t>() + i, 1, hipMemcpyDeviceToHost, stream()));      // (the presence byte rides in front of the value: one wait for both)
      elem_peek(pin + 16, (const uint8_t*)v->dval.p + i * ts, ts, hipMemcpyDeviceToHost);
      if (!pin[0]) r = GrB_NO_VALUE; else cast_scalar(xcode, x, v->type->code, pin + 16);
      return;
    }
    vec_to_host(v);
    auto it = std::lower_bound(v->hi.begin(), v->hi.end(), i);
    if (it == v->hi.end() || *it != i) r = GrB_NO_VALUE;
    else cast_scalar(xcode, x, v->type->code, &v->hx[(it - v->hi.begin()) * v->type->size]); });
  return info ? info : r;
}

}  // namespace grb

using namespace grb;

extern "C" {

GrB_Info GrB_Matrix_removeElement(GrB_Matrix A, GrB_Index i, GrB_Index j) {
  CHECK_MAT(A); if (i >= A->nrows || j >= A->ncols) return GrB_INVALID_INDEX;
  return guarded(A, [&] {
    GrB_Matrix_opaque::Pending p{i, j, true, {0}};
    if (mat_edit_route(A)) { A->pending.push_back(p); A->bm.clear(); return; }      // it lives in HBM: queued for the device (the bitmap cache beside the CSR has its own readers: dropped now)
    mat_to_host(A); A->pending.push_back(p); mat_invalidate_device(A); });
}
GrB_Info GrB_Vector_removeElement(GrB_Vector v, GrB_Index i) {
  CHECK_VEC(v); if (i >= v->n) return GrB_INVALID_INDEX;
  return guarded(v, [&] {
    GrB_Vector_opaque::Pending p{i, true, {0}};
    if (!v->host_valid && !v->iso_full) { if (v->lazy | v->q_reads) vec_resolve(v); if (vec_edit_route(v)) { v->pending.push_back(p); v->facts.image_replaced(0, false); return; } }      // it lives in HBM (a deferred chain completed first): queued for the device
    vec_to_host(v); v->pending.push_back(p); vec_invalidate_device(v); });
}

}  // extern "C"
