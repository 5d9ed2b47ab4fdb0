// grb_mirror.cpp — the two images of a container and the way between them: the host mirror (sorted tuples, assembled from the pending edits), the HBM image
// (CSR / bitmap), what happens to either when the other is written, and the upload / download that makes one from the other.
#include "grb_container.hpp"
#include "grb_edit_list.hpp"
#include <string.h>
#include <tuple>

namespace grb {

// ---- host assemble: apply pending setElement/removeElement in program order (the merge: grb_edit_list.hpp) ---------------------
template <class C> static void host_assemble(C* c, std::vector<GrB_Index>* hj) {
  if (c->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
  if (c->pending.empty()) return;
  const bool rebuilt = c->pending.size() > EDIT_IN_PLACE_MAX;
  edit_merge_host(c->hi, hj, c->hx, c->type->size, c->pending);
  c->pending.clear(); if (rebuilt) c->pending.shrink_to_fit();
}
void mat_host_assemble(GrB_Matrix A) { host_assemble(A, &A->hj); }
void vec_host_assemble(GrB_Vector v) { host_assemble(v, nullptr); }

// ---- what happened to the device image: one function per event, each covers csr, csc and bm (the transitions: grb_devcsr.hpp) ----
// no device image (the host mirror was written)
void mat_invalidate_device(GrB_Matrix A) { A->dev_valid = false; A->csr.clear(); A->csc.clear(); A->bm.clear(); }
// rows, columns or the entry set of the device CSR changed (the structural flush, resize)
void mat_structure_changed(GrB_Matrix A) { A->csc.clear(); A->bm.clear(); A->csr.derived.structure_changed(); }
// the device image was replaced as a whole: the host mirror and the edit queue go, and whatever was derived from the old image.  The caller installs the new one.
void mat_invalidate_host(GrB_Matrix A) {
  A->host_valid = false; A->hi.clear(); A->hj.clear(); A->hx.clear(); A->pending.clear(); A->dev_elem_ops = 0;
  A->hi.shrink_to_fit(); A->hj.shrink_to_fit(); A->hx.shrink_to_fit();
  mat_structure_changed(A);
}
// values of the device CSR were overwritten in place (mat_set, the values-only flush): the transpose and the bitmap hold copies of them
void mat_values_changed(GrB_Matrix A) { A->csc.clear(); A->bm.clear(); A->csr.derived.values_changed(); }

void vec_invalidate_device(GrB_Vector v) { vec_overwritten(v); v->dev_valid = false; v->dval.reset(); v->dpres.reset(); v->facts.image_dropped(); }
// the device image was written: deferred work on v is settled and the host mirror goes
static void vec_host_dropped(GrB_Vector v) {
  vec_overwritten(v); v->dev_elem_ops = 0;
  v->host_valid = false; v->hi.clear(); v->hx.clear(); v->pending.clear(); v->hi.shrink_to_fit(); v->hx.shrink_to_fit();
}
void vec_invalidate_host(GrB_Vector v, uint64_t nvals, bool known) { vec_host_dropped(v); v->facts.image_replaced(nvals, known); }
void vec_device_extended(GrB_Vector v) { vec_host_dropped(v); v->facts.image_extended(); }

// ---- one way in and out of a device image ---------------------------------------------------------------------------------------
void csr_upload(DevCSR& c, uint64_t nrows, uint64_t ncols, uint64_t nnz, const uint32_t* rowptr, const uint32_t* col, const void* val, size_t ts, hipMemcpyKind kind) {
  c.nrows = (uint32_t)nrows; c.ncols = (uint32_t)ncols; c.nnz = nnz;
  c.rowptr.alloc(((size_t)nrows + 1) * 4); c.col.alloc(nnz * 4); c.val.alloc(nnz * ts);
  GRB_HIP(hipMemcpyAsync(c.rowptr.p, rowptr, ((size_t)nrows + 1) * 4, kind, stream()));
  if (nnz) {
    GRB_HIP(hipMemcpyAsync(c.col.p, col, nnz * 4, kind, stream()));
    GRB_HIP(hipMemcpyAsync(c.val.p, val, nnz * ts, kind, stream()));
  }
}
void csr_download(const DevCSR& c, uint32_t* rowptr, uint32_t* col, void* val, size_t ts, hipMemcpyKind kind) {
  if (rowptr) GRB_HIP(hipMemcpyAsync(rowptr, c.rowptr.p, ((size_t)c.nrows + 1) * 4, kind, stream()));
  if (col && c.nnz) GRB_HIP(hipMemcpyAsync(col, c.col.p, c.nnz * 4, kind, stream()));
  if (val && c.nnz) GRB_HIP(hipMemcpyAsync(val, c.val.p, c.nnz * ts, kind, stream()));
}
void bitmap_copy(DevBitmap& d, const DevBitmap& s, size_t np, size_t ts) {
  d.val.alloc(np * ts + 64); d.pres.alloc(np + 64);
  GRB_HIP(hipMemcpyAsync(d.val.p, s.val.p, np * ts, hipMemcpyDeviceToDevice, stream()));
  GRB_HIP(hipMemcpyAsync(d.pres.p, s.pres.p, np, hipMemcpyDeviceToDevice, stream()));
  d.valid = true; d.nvals = s.nvals; d.nvals_known = s.nvals_known;
}
std::pair<DevBuf, DevBuf> vec_alloc_image(uint64_t n, size_t ts, bool zero) {
  std::pair<DevBuf, DevBuf> m;
  m.first.alloc(n * ts ? n * ts : 1); m.second.alloc(n ? n : 1);
  if (zero && n) { GRB_HIP(hipMemsetAsync(m.first.p, 0, n * ts, stream())); GRB_HIP(hipMemsetAsync(m.second.p, 0, n, stream())); }
  return m;
}
void elem_peek(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  GRB_HIP(hipMemcpyAsync(dst, src, bytes, kind, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));
}

// ---- matrices ---------------------------------------------------------------------------------------------------------------------
void mat_to_host(GrB_Matrix A) {
  if (A->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
  if (A->host_valid) { mat_host_assemble(A); return; }
  if (mat_bitmap_only(A)) mat_to_device(A);                  // a batch matrix that lives as a bitmap: its CSR first
  mat_edit_flush(A);                                         // queued element edits reach the device image first
  // download the device CSR and expand to sorted tuples
  const DevCSR& c = A->csr; const size_t ts = A->type->size;
  std::vector<uint32_t> rp(c.nrows + 1), col(c.nnz);
  A->hx.resize(c.nnz * ts);
  csr_download(c, rp.data(), col.data(), A->hx.data(), ts, hipMemcpyDeviceToHost);
  GRB_HIP(hipStreamSynchronize(stream()));
  A->hi.resize(c.nnz); A->hj.resize(c.nnz);
  for (uint32_t r = 0; r < c.nrows; r++)
    for (uint32_t p = rp[r]; p < rp[r + 1]; p++) { A->hi[p] = r; A->hj[p] = col[p]; }
  A->host_valid = true;
}

void mat_to_device(GrB_Matrix A) {
  if (A->dev_valid) { mat_edit_flush(A); return; }
  if (mat_bitmap_only(A)) { mat_bitmap_to_csr(A); return; }
  if (A->type->code >= T_FC32) fail(GrB_DOMAIN_MISMATCH, "complex matrices are host-side containers here: no device arithmetic on them");
  need_device();
  mat_host_assemble(A);
  if (A->nrows > GRB_DIM_DEVICE_MAX || A->ncols > GRB_DIM_DEVICE_MAX)
    fail(GrB_INSUFFICIENT_SPACE, "matrix dimension exceeds the 32-bit index range of the HBM CSR layout");
  const uint64_t nnz = A->hi.size();
  if (nnz > 0xFFFFFFF0ull) fail(GrB_INSUFFICIENT_SPACE, "more than 2^32 entries in one device matrix");
  DevCSR& c = A->csr; c.clear();
  std::vector<uint32_t> rp((size_t)A->nrows + 1, 0), col(nnz);
  for (uint64_t p = 0; p < nnz; p++) { rp[A->hi[p] + 1]++; col[p] = (uint32_t)A->hj[p]; }
  for (uint64_t r = 0; r < A->nrows; r++) rp[r + 1] += rp[r];
  csr_upload(c, A->nrows, A->ncols, nnz, rp.data(), col.data(), A->hx.data(), A->type->size, hipMemcpyHostToDevice);
  GRB_HIP(hipStreamSynchronize(stream()));
  c.valid = true; A->dev_valid = true;
}

uint64_t mat_nvals(GrB_Matrix A) {
  if (A->iso_full) { const unsigned __int128 t = (unsigned __int128)A->nrows * A->ncols; return t > UINT64_MAX ? UINT64_MAX : (uint64_t)t; }
  if (A->host_valid) { mat_host_assemble(A); return A->hi.size(); }
  if (mat_bitmap_only(A)) return mat_bitmap_nvals(A);
  mat_edit_flush(A);
  return A->csr.nnz;
}

const DevCSR& mat_csc(GrB_Matrix A) {
  mat_to_device(A);
  if (!A->csc.valid) csr_transpose(A->csr, A->type->size, A->csc);
  return A->csc;
}

// ---- vectors ---------------------------------------------------------------------------------------
void vec_to_host(GrB_Vector v) {
  vec_gate(v);
  if (v->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
  if (v->host_valid) { vec_host_assemble(v); return; }
  const size_t ts = v->type->size; const uint64_t n = v->n;
  std::vector<uint8_t> val(n * ts), pres(n);
  if (n) {
    GRB_HIP(hipMemcpyAsync(val.data(), v->dval.p, n * ts, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipMemcpyAsync(pres.data(), v->dpres.p, n, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  }
  v->hi.clear(); v->hx.clear();
  for (uint64_t i = 0; i < n; i++) if (pres[i]) { v->hi.push_back(i); v->hx.insert(v->hx.end(), &val[i * ts], &val[i * ts] + ts); }
  v->host_valid = true;
}
void vec_to_device(GrB_Vector v) {
  vec_gate(v);
  if (v->dev_valid) return;
  if (v->type->code >= T_FC32) fail(GrB_DOMAIN_MISMATCH, "complex vectors are host-side containers here: no device arithmetic on them");
  need_device();
  vec_host_assemble(v);
  if (v->n > GRB_DIM_DEVICE_MAX) fail(GrB_INSUFFICIENT_SPACE, "vector length exceeds the 32-bit index range of the HBM bitmap layout");
  const size_t ts = v->type->size; const uint64_t n = v->n;
  std::tie(v->dval, v->dpres) = vec_alloc_image(n, ts, false);
  if (n && v->hi.size() * 16 <= n) {
    // few entries (an empty output vector, the one-entry frontier of a BFS): zero the bitmap in HBM and scatter the entries —
    // staging n zero bytes on the host and copying them cost 2 x 15 ms per PageRank run at R-MAT-25 and half of a BFS at R-MAT-22
    const uint32_t k = (uint32_t)v->hi.size();
    if (k <= 16 && ts <= 8) init_entries_small(k, v->hi.data(), v->hx.data(), ts, v->dval.p, v->dpres.as<uint8_t>(), n);      // zeros + the entries, one launch
    else { GRB_HIP(hipMemsetAsync(v->dval.p, 0, n * ts, stream())); GRB_HIP(hipMemsetAsync(v->dpres.p, 0, n, stream())); }
    if (k <= 16 && ts <= 8) {}
    else if (k) {
      std::vector<uint32_t> i32(k); for (uint32_t e = 0; e < k; e++) i32[e] = (uint32_t)v->hi[e];
      DevBuf di((size_t)k * 4), dx((size_t)k * ts);
      GRB_HIP(hipMemcpyAsync(di.p, i32.data(), (size_t)k * 4, hipMemcpyHostToDevice, stream()));
      GRB_HIP(hipMemcpyAsync(dx.p, v->hx.data(), (size_t)k * ts, hipMemcpyHostToDevice, stream()));
      scatter_entries(k, di.as<uint32_t>(), dx.p, ts, v->dval.p, v->dpres.as<uint8_t>());
      GRB_HIP(hipStreamSynchronize(stream()));                          // the host staging vectors go out of scope
    }
    v->facts.image_replaced(k, true); v->dev_valid = true;
    if (k <= 64) {                                                       // the entries as a list (see small_idx)
      v->facts.small_idx.assign(k, 0); bool truthy = true;
      for (uint32_t e = 0; e < k; e++) {
        v->facts.small_idx[e] = (uint32_t)v->hi[e];
        // truth as the mask kernels test it — value != 0 in the vector's type: the bytes of an FP -0.0 are not all zero, the value is false
        bool nz = false;
        const uint8_t* px = &v->hx[(size_t)e * ts];
        if (v->type->code == T_FP32) { float f; memcpy(&f, px, 4); nz = f != 0.0f; }
        else if (v->type->code == T_FP64) { double f; memcpy(&f, px, 8); nz = f != 0.0; }
        else for (size_t b = 0; b < ts; b++) nz = nz || px[b] != 0;
        truthy = truthy && nz;
      }
      v->facts.small_valid = true; v->facts.small_truthy = truthy;
    }
    return;
  }
  std::vector<uint8_t> val(n * ts, 0), pres(n, 0);
  for (size_t k = 0; k < v->hi.size(); k++) { pres[v->hi[k]] = 1; memcpy(&val[v->hi[k] * ts], &v->hx[k * ts], ts); }
  if (n) {
    GRB_HIP(hipMemcpyAsync(v->dval.p, val.data(), n * ts, hipMemcpyHostToDevice, stream()));
    GRB_HIP(hipMemcpyAsync(v->dpres.p, pres.data(), n, hipMemcpyHostToDevice, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  }
  v->facts.image_replaced(v->hi.size(), true); v->dev_valid = true;
}
uint64_t vec_dev_nvals(GrB_Vector v) {
  vec_gate(v);
  if (!v->facts.dnvals_known) { v->facts.dnvals = count_present(v->dpres.as<uint8_t>(), v->n); v->facts.dnvals_known = true; }
  return v->facts.dnvals;
}
uint64_t vec_nvals(GrB_Vector v) {
  vec_gate(v);
  if (v->iso_full) return v->n;
  if (v->host_valid) { vec_host_assemble(v); return v->hi.size(); }
  return vec_dev_nvals(v);
}

}  // namespace grb
