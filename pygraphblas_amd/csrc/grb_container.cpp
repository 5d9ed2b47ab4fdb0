// grb_container.cpp — GrB_Matrix / GrB_Vector / GxB_Scalar objects and their host<->HBM mirrors.
//
// Replaces the object-model half of the `lib.` surface that pygraphblas calls:
//   GrB_Matrix_new/free/dup/clear/nrows/ncols/nvals/wait/error/resize/removeElement
//        (reference call sites: pygraphblas/matrix.py:99-117, 171-175, 627-760, 3353)
//   GrB_Matrix_build_<T> / setElement_<T> / extractElement_<T> / extractTuples_<T>
//        (pygraphblas/matrix.py:325-330, 1503-1529, 3180-3308; types.py:87-110)
//   the Vector and Scalar equivalents (pygraphblas/vector.py:60-95, scalar.py:20-92).
// Ownership: the library allocates in *_new and frees in *_free(&h); free of NULL / already freed
// handles is a successful no-op (reference __del__ checks the return code).
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_matops.hpp"
#include "grb_userop.hpp"
#include "grb_edit.hpp"
#include "grb_edit_list.hpp"
#include "grb_build.hpp"
#include "grb_tuples.hpp"
#include <algorithm>
#include <numeric>
#include <string.h>
#include <stdarg.h>
#include <stdio.h>

namespace grb {

// ---- host assemble: apply pending setElement/removeElement in program order ---------------------
static const char* const ISO_MSG = "a full one-valued container of this dimension can be read element-wise only";
void mat_host_assemble(GrB_Matrix A) {
  if (A->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
  if (A->pending.empty()) return;
  const size_t ts = A->type->size;
  auto& P = A->pending;
  if (P.size() <= 8) {            // a few edits (`M[i, j] = x` then a read): in place, one memmove each, instead of rebuilding the tuple arrays
    for (const auto& e : P) {
      size_t lo = 0, hi = A->hi.size();
      while (lo < hi) { const size_t m = (lo + hi) / 2; if (A->hi[m] < e.i || (A->hi[m] == e.i && A->hj[m] < e.j)) lo = m + 1; else hi = m; }
      const bool found = lo < A->hi.size() && A->hi[lo] == e.i && A->hj[lo] == e.j;
      if (e.del) { if (found) { A->hi.erase(A->hi.begin() + lo); A->hj.erase(A->hj.begin() + lo); A->hx.erase(A->hx.begin() + lo * ts, A->hx.begin() + (lo + 1) * ts); } }
      else if (found) memcpy(&A->hx[lo * ts], e.x, ts);
      else { A->hi.insert(A->hi.begin() + lo, e.i); A->hj.insert(A->hj.begin() + lo, e.j); A->hx.insert(A->hx.begin() + lo * ts, e.x, e.x + ts); }
    }
    P.clear(); return;
  }
  std::vector<uint32_t> ord(P.size());
  std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
    return P[a].i != P[b].i ? P[a].i < P[b].i : P[a].j < P[b].j; });
  std::vector<GrB_Index> ni, nj; std::vector<uint8_t> nx;
  ni.reserve(A->hi.size() + P.size()); nj.reserve(A->hi.size() + P.size()); nx.reserve((A->hi.size() + P.size()) * ts);
  size_t b = 0, nb = A->hi.size(), k = 0;
  auto push_base = [&](size_t q) { ni.push_back(A->hi[q]); nj.push_back(A->hj[q]); nx.insert(nx.end(), &A->hx[q * ts], &A->hx[q * ts] + ts); };
  while (k < ord.size()) {
    size_t e = k;   // [k, e] = run of edits to the same coordinate; the last one wins
    while (e + 1 < ord.size() && P[ord[e + 1]].i == P[ord[k]].i && P[ord[e + 1]].j == P[ord[k]].j) e++;
    const auto& last = P[ord[e]];
    while (b < nb && (A->hi[b] < last.i || (A->hi[b] == last.i && A->hj[b] < last.j))) push_base(b++);
    if (b < nb && A->hi[b] == last.i && A->hj[b] == last.j) b++;   // replaced or deleted
    if (!last.del) { ni.push_back(last.i); nj.push_back(last.j); nx.insert(nx.end(), last.x, last.x + ts); }
    k = e + 1;
  }
  while (b < nb) push_base(b++);
  A->hi.swap(ni); A->hj.swap(nj); A->hx.swap(nx); P.clear(); P.shrink_to_fit();
}

// ---- what happened to the device image: one function per event, each covers csr, csc and bm (the transitions: grb_devcsr.hpp) ----
// no device image (the host mirror was written)
void mat_invalidate_device(GrB_Matrix A) { A->dev_valid = false; A->csr.clear(); A->csc.clear(); A->bm.clear(); }
// rows, columns or the entry set of the device CSR changed (the structural flush, resize)
static void mat_structure_changed(GrB_Matrix A) { A->csc.clear(); A->bm.clear(); A->csr.derived.structure_changed(); }
// the device image was replaced as a whole: the host mirror and the edit queue go, and whatever was derived from the old image.  The caller installs the new one.
void mat_invalidate_host(GrB_Matrix A) {
  A->host_valid = false; A->hi.clear(); A->hj.clear(); A->hx.clear(); A->pending.clear(); A->dev_elem_ops = 0;
  A->hi.shrink_to_fit(); A->hj.shrink_to_fit(); A->hx.shrink_to_fit();
  mat_structure_changed(A);
}
// values of the device CSR were overwritten in place (mat_set, the values-only flush): the transpose and the bitmap hold copies of them
static void mat_values_changed(GrB_Matrix A) { A->csc.clear(); A->bm.clear(); A->csr.derived.values_changed(); }

// ---- the edit queue of a container that lives in HBM only ------------------------------------------------------------------------------
// `A[i, j] = x`, `del A[i, j]`, `v[i] = x` on a container whose only valid image is the HBM one append today's Pending record and nothing else: no download, nothing
// invalidated.  The queue is applied on the device (grb_edit.hip) before anything reads or replaces that image: mat_to_device / mat_to_host / mat_nvals / dup / wait /
// resize for matrices, vec_gate (which every reader of a vector passes) for vectors; extractElement looks in the queue first.  Whoever replaces the image as a whole
// clears `pending` (mat_invalidate_host, GrB_Matrix_clear, the vector drivers).  GRB_MI355X_EDIT=0 forces the host route everywhere.
// The plan string of a flush goes IN FRONT of what the plan holds: most flushes run inside an operation (mat_to_device / mat_nvals / vec_gate of its operands and
// output), whose own plan stays behind it.  The entry points that are flush points of their own (nvals, wait, dup, extractElement, extractTuples) start from an
// empty plan when edits are queued.
static bool edit_env_off() { const char* e = getenv("GRB_MI355X_EDIT"); return e && *e && atoi(e) == 0; }
static bool mat_edit_route(GrB_Matrix A) {
  return A->dev_valid && !A->host_valid && !A->iso_full && A->csr.valid && A->type->code < T_FC32 && A->nrows <= GRB_DIM_DEVICE_MAX && A->ncols <= GRB_DIM_DEVICE_MAX &&
         device_ok() && !edit_env_off();
}
static bool vec_edit_route(GrB_Vector v) {
  return v->dev_valid && !v->host_valid && !v->iso_full && v->lazy == 0 && v->q_reads == 0 && v->type->code < T_FC32 && v->n <= GRB_DIM_DEVICE_MAX && device_ok() && !edit_env_off();
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

void mat_to_host(GrB_Matrix A) {
  if (A->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
  if (A->host_valid) { mat_host_assemble(A); return; }
  if (mat_bitmap_only(A)) mat_to_device(A);                  // a batch matrix that lives as a bitmap: its CSR first
  mat_edit_flush(A);                                         // queued element edits reach the device image first
  // download the device CSR and expand to sorted tuples
  const DevCSR& c = A->csr; const size_t ts = A->type->size;
  std::vector<uint32_t> rp(c.nrows + 1), col(c.nnz);
  A->hx.resize(c.nnz * ts);
  GRB_HIP(hipMemcpyAsync(rp.data(), c.rowptr.p, (c.nrows + 1) * 4ull, hipMemcpyDeviceToHost, stream()));
  if (c.nnz) {
    GRB_HIP(hipMemcpyAsync(col.data(), c.col.p, c.nnz * 4ull, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipMemcpyAsync(A->hx.data(), c.val.p, c.nnz * ts, hipMemcpyDeviceToHost, stream()));
  }
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
  const uint64_t nnz = A->hi.size(); const size_t ts = A->type->size;
  if (nnz > 0xFFFFFFF0ull) fail(GrB_INSUFFICIENT_SPACE, "more than 2^32 entries in one device matrix");
  DevCSR& c = A->csr; c.clear();
  c.nrows = (uint32_t)A->nrows; c.ncols = (uint32_t)A->ncols; c.nnz = nnz;
  std::vector<uint32_t> rp((size_t)c.nrows + 1, 0), col(nnz);
  for (uint64_t p = 0; p < nnz; p++) { rp[A->hi[p] + 1]++; col[p] = (uint32_t)A->hj[p]; }
  for (uint32_t r = 0; r < c.nrows; r++) rp[r + 1] += rp[r];
  c.rowptr.alloc(((size_t)c.nrows + 1) * 4); c.col.alloc(nnz * 4); c.val.alloc(nnz * ts);
  GRB_HIP(hipMemcpyAsync(c.rowptr.p, rp.data(), rp.size() * 4, hipMemcpyHostToDevice, stream()));
  if (nnz) {
    GRB_HIP(hipMemcpyAsync(c.col.p, col.data(), nnz * 4, hipMemcpyHostToDevice, stream()));
    GRB_HIP(hipMemcpyAsync(c.val.p, A->hx.data(), nnz * ts, hipMemcpyHostToDevice, stream()));
  }
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
void vec_host_assemble(GrB_Vector v) {
  if (v->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
  if (v->pending.empty()) return;
  const size_t ts = v->type->size; auto& P = v->pending;
  std::vector<uint32_t> ord(P.size()); std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return P[a].i < P[b].i; });
  std::vector<GrB_Index> ni; std::vector<uint8_t> nx;
  size_t b = 0, nb = v->hi.size(), k = 0;
  auto push_base = [&](size_t q) { ni.push_back(v->hi[q]); nx.insert(nx.end(), &v->hx[q * ts], &v->hx[q * ts] + ts); };
  while (k < ord.size()) {
    size_t e = k; while (e + 1 < ord.size() && P[ord[e + 1]].i == P[ord[k]].i) e++;
    const auto& last = P[ord[e]];
    while (b < nb && v->hi[b] < last.i) push_base(b++);
    if (b < nb && v->hi[b] == last.i) b++;
    if (!last.del) { ni.push_back(last.i); nx.insert(nx.end(), last.x, last.x + ts); }
    k = e + 1;
  }
  while (b < nb) push_base(b++);
  v->hi.swap(ni); v->hx.swap(nx); P.clear(); P.shrink_to_fit();
}
// ---- "any stored value true" of a BOOL product result (grb_spmv.hpp: SpmvCall::any_true) -----------------------------------
// One device word per thread.  Every product brings a fresh non-zero tag and its kernels store that tag, so the word never has
// to be cleared: it answers "true" for the vector that holds the tag it currently shows, and only the latest product's vector
// may ask (GrB_Vector_reduce_BOOL with LOR then reads four bytes instead of launching a kernel over the vector).
// Round 5: the summary of a BOOL result's true entries (SpmvCall::fe_host) — every workgroup of the product stores its (edge sum, entry count),
// tagged, into its own pair of page-locked HOST words, and the lookup spins until all pairs carry the product's tag: no copy, no stream
// synchronisation.
namespace {
constexpr size_t FE_HOST_PAIRS = 2048;      // (grb_spmv_kernels.hpp: FE_MAX_BLOCKS)
struct AnyTrue { DevBuf word; GrB_Vector owner = nullptr; uint32_t tag = 0; bool fe_has = false; uint64_t fe_key = 0; uint32_t fe_nblocks = 0; unsigned long long* host = nullptr; unsigned long long* host_dev = nullptr; };
thread_local AnyTrue t_any;
}
uint32_t* any_true_acquire(uint32_t* tag) {
  AnyTrue& s = t_any;
  if (!s.word.p) {
    s.word.alloc(64); GRB_HIP(hipMemsetAsync(s.word.p, 0, 64, stream()));
    void* h = nullptr; GRB_HIP(hipHostMalloc(&h, FE_HOST_PAIRS * 8, hipHostMallocMapped | hipHostMallocCoherent)); memset(h, 0, FE_HOST_PAIRS * 8); s.host = (unsigned long long*)h;      // (lives as long as the thread's pinned scratch: never freed)
    void* dp = nullptr; if (hipHostGetDevicePointer(&dp, h, 0) != hipSuccess) { (void)hipGetLastError(); dp = h; }
    s.host_dev = (unsigned long long*)dp;
    if (const char* e = getenv("GRB_MI355X_SUMMARY_TAG0")) s.tag = (uint32_t)strtoul(e, nullptr, 0);      // test hook: start the tags just below the 24-bit wrap
  }
  if ((++s.tag & 0xFFFFFFu) == 0) {                   // (the low 24 bits travel in the host words of the summary: never zero)
    s.tag++;
    // the 24-bit tags start over: a word that a product 2^24 calls ago left unread (its summary was never asked for, and no product since had as many
    // workgroups) must not pass for the coming product's — once per 16.7 million products, wait for the stream and wipe the words
    GRB_HIP(hipStreamSynchronize(stream())); memset(s.host, 0, FE_HOST_PAIRS * 8);
  }
  s.owner = nullptr; s.fe_has = false; *tag = s.tag;
  return s.word.as<uint32_t>();
}
unsigned long long* fe_summary_host() { return t_any.host_dev; }      // (after any_true_acquire)
void any_true_written(GrB_Vector w, const void* key, uint32_t tag, uint64_t fe_key, uint32_t fe_nblocks) {
  AnyTrue& s = t_any;
  s.owner = w; s.fe_has = fe_key != 0 && w != nullptr && fe_nblocks > 0 && fe_nblocks <= FE_HOST_PAIRS; s.fe_key = fe_key; s.fe_nblocks = fe_nblocks;
  if (w) { w->facts.lor_state = 1; w->facts.lor_key = key; w->facts.lor_tag = tag; }
}
bool any_true_lookup(GrB_Vector u, bool* value) {
  if (!u->facts.lor_state || u->lazy || u->q_reads || !u->dev_valid || u->dval.p != u->facts.lor_key) return false;
  if (u->facts.lor_state == 1) {
    AnyTrue& s = t_any;
    if (s.owner != u || s.tag != u->facts.lor_tag) { u->facts.lor_state = 0; return false; }
    if (s.fe_has) {
      // every workgroup stores  tag (24 bits) | true entries, saturating (8) | edge sum, saturating (32)  into its host word: wait for all of them,
      // and clear what was read (a word is never mistaken for a later product's with the same 24-bit tag)
      volatile unsigned long long* h = s.host; const unsigned long long want = (unsigned long long)(u->facts.lor_tag & 0xFFFFFFu);
      unsigned long long fe = 0, cnt = 0; uint32_t i = 0; const uint32_t nb = s.fe_nblocks;
      for (int round = 0; round < 2 && i < nb; round++) {
        for (uint64_t spin = 0; spin < (1ull << 22) && i < nb;) {
          const unsigned long long a = h[i];
          if ((a >> 40) == want && a != 0) { fe += a & 0xFFFFFFFFull; cnt += (a >> 32) & 0xFFull; h[i] = 0; i++; } else { spin++; __builtin_ia32_pause(); }
        }
        if (i < nb) GRB_HIP(hipStreamSynchronize(stream()));      // (far beyond any product's time: let a failed launch report itself, then look once more)
      }
      s.owner = nullptr; s.fe_has = false;
      if (i < nb) { u->facts.lor_state = 0; return false; }
      u->facts.lor_state = cnt ? 3 : 2;
      u->facts.fe_lb = fe; u->facts.fe_lb_key = s.fe_key; u->facts.fe_lb_true = true;      // the edges leaving u's true entries (exact when the kernel counted: a lower bound is all the direction choice asks for)
    } else {
      uint32_t* pin = (uint32_t*)pinned_scratch();
      GRB_HIP(hipMemcpyAsync(pin, s.word.p, 4, hipMemcpyDeviceToHost, stream()));
      GRB_HIP(hipStreamSynchronize(stream()));
      u->facts.lor_state = pin[0] == u->facts.lor_tag ? 3 : 2; s.owner = nullptr;
    }
  }
  *value = u->facts.lor_state == 3; return true;
}

void vec_invalidate_device(GrB_Vector v) { vec_overwritten(v); v->dev_valid = false; v->dval.reset(); v->dpres.reset(); v->facts.image_dropped(); }
// the device image was written: deferred work on v is settled and the host mirror goes
static void vec_host_dropped(GrB_Vector v) {
  vec_overwritten(v); v->dev_elem_ops = 0;
  v->host_valid = false; v->hi.clear(); v->hx.clear(); v->pending.clear(); v->hi.shrink_to_fit(); v->hx.shrink_to_fit();
}
void vec_invalidate_host(GrB_Vector v, uint64_t nvals, bool known) { vec_host_dropped(v); v->facts.image_replaced(nvals, known); }
void vec_device_extended(GrB_Vector v) { vec_host_dropped(v); v->facts.image_extended(); }
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
  v->dval.alloc(n * ts ? n * ts : 1); v->dpres.alloc(n ? n : 1);
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

// sort + combine duplicates for build(); keys are (i,j) pairs (j == 0 for vectors)
static void build_tuples(GrB_Type type, const GrB_Index* I, const GrB_Index* J, const void* X, int xcode, GrB_Index n,
                         GrB_Index nrows, GrB_Index ncols, GrB_BinaryOp dup, std::vector<GrB_Index>& hi,
                         std::vector<GrB_Index>* hj, std::vector<uint8_t>& hx) {
  const size_t ts = type->size; const size_t xs = type_size(xcode);
  if (dup && check_obj(dup) && is_user(dup)) userop_refuse(dup->name, "the dup operator of build");
  if (dup && check_obj(dup) && binop_is_positional(dup->opcode)) fail(GrB_DOMAIN_MISMATCH, std::string("positional operator ") + dup->name + " cannot be used as the dup operator of build: it is the multiplier of the positional semirings, which run in mxm, mxv and vxm only");
  for (GrB_Index k = 0; k < n; k++) {
    if (I[k] >= nrows || (J && J[k] >= ncols)) fail(GrB_INDEX_OUT_OF_BOUNDS, "build: index out of bounds");
  }
  std::vector<uint64_t> ord(n); std::iota(ord.begin(), ord.end(), 0ull);
  std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
    if (I[a] != I[b]) return I[a] < I[b]; return J ? J[a] < J[b] : false; });
  hi.clear(); if (hj) hj->clear(); hx.clear();
  hi.reserve(n); if (hj) hj->reserve(n); hx.reserve(n * ts);
  uint8_t cur[16], nxt[16];
  for (GrB_Index k = 0; k < n;) {
    GrB_Index e = k; const uint64_t o = ord[k];
    cast_scalar(type->code, cur, xcode, (const uint8_t*)X + o * xs);
    while (e + 1 < n && I[ord[e + 1]] == I[o] && (!J || J[ord[e + 1]] == J[o])) {
      e++;
      cast_scalar(type->code, nxt, xcode, (const uint8_t*)X + ord[e] * xs);
      if (!dup) fail(GrB_INVALID_VALUE, "build: duplicate index and no dup operator");
      if (type->code >= T_FC32) fail(GrB_DOMAIN_MISMATCH, "build: combining duplicate complex entries is out of scope");
      dispatch_type(type->code, [&]<class T>() { T a, b; memcpy(&a, cur, sizeof(T)); memcpy(&b, nxt, sizeof(T));
        T z = apply_binop<T>(dup->opcode, a, b); memcpy(cur, &z, sizeof(T)); });
    }
    hi.push_back(I[o]); if (hj) hj->push_back(J[o]); hx.insert(hx.end(), cur, cur + ts);
    k = e + 1;
  }
}

// ---- build on the device (kernels: grb_build.hip; key arithmetic, thresholds and the route predicate: grb_build_keys.hpp) ------------------------------------------
// The device route is taken when a HIP device is present, the container has one of the 11 real types and the tuples have that type too (a build that casts keeps
// the host route), dup is NULL or a built-in, non-positional operator whose three domains are that type and whose device evaluation gives the host's bits (not the
// operators of binop_needs_math: ATAN2 ... LDEXP and POW — POW on every type, integer and BOOL included, although those are exact: the fold kernel is compiled
// without the math switch), the dimensions and the tuple count fit the 32-bit layout, and the call has at least BUILD_DEVICE_MIN_TUPLES tuples.
// GRB_MI355X_BUILD=0 forces the host route, =1 the device route wherever it is legal (read per call: a test hook).  Outcomes come in the host route's order —
// OUTPUT_NOT_EMPTY (before the choice), INDEX_OUT_OF_BOUNDS, INVALID_VALUE — and the container is written only after the last of them is excluded: a refused
// build leaves it as it was.  A run of duplicates beyond BUILD_RUN_SERIAL_MAX of an operator that is not exactly associative sends the whole call to the host route.
static bool build_dup_on_device(GrB_BinaryOp dup, int code) {
  if (!dup) return true;
  return dup->opcode < B_FIRSTI && !binop_needs_math(dup->opcode) && dup->xtype && dup->ytype && dup->ztype &&
         dup->xtype->code == code && dup->ytype->code == code && dup->ztype->code == code;
}
static bool build_takes_device(GrB_Type type, bool iso, int xcode, GrB_Index n, GrB_Index nrows, GrB_Index ncols, GrB_BinaryOp dup) {
  const bool legal = build_route_legal(device_ok() && !iso, type->code <= T_FP64, xcode == type->code, build_dup_on_device(dup, type->code), nrows, ncols, n);
  return build_route_taken(legal, route_env("GRB_MI355X_BUILD"), n);
}
// "GrB_PLUS_FP64" of type "GrB_FP64" -> "PLUS"
static std::string build_plan(GrB_Type type, GrB_BinaryOp dup, const BuildResult& r) {
  const std::string tn = strlen(type->name) > 4 ? type->name + 4 : type->name;
  std::string dn = "none";
  if (dup) { dn = strlen(dup->name) > 4 ? dup->name + 4 : dup->name; if (dn.size() > tn.size() + 1 && dn.compare(dn.size() - tn.size() - 1, std::string::npos, "_" + tn) == 0) dn.resize(dn.size() - tn.size() - 1); }
  std::string p = "build<type=" + tn + ",dup=" + dn + ",key=" + (r.key64 ? "u64" : "u32") + ",sorted=" + (r.sorted ? "1" : "0") + ",fold=" + r.fold + ",rows=" + (r.search ? "search" : "heads") + "> ";
  if (r.sorted && !r.nvals) return p;                          // no tuples: nothing was launched
  p += r.sorted ? "k_build_keys k_build_unpack " : "k_build_keys k_build_heads k_build_starts k_build_runmax k_build_fold ";
  return p;
}
// the tuples where the kernels read them: device pointers as they are, host arrays uploaded once
struct BuildStage {
  DevBuf bi, bj, bx; const uint64_t* I; const uint64_t* J; const void* X;
  BuildStage(const GrB_Index* I_, const GrB_Index* J_, const void* X_, GrB_Index n, size_t ts, int location) : I(I_), J(J_), X(X_) {
    if (location || !n) return;
    bi.alloc(n * 8); GRB_HIP(hipMemcpyAsync(bi.p, I_, n * 8, hipMemcpyHostToDevice, stream())); I = bi.as<uint64_t>();
    if (J_) { bj.alloc(n * 8); GRB_HIP(hipMemcpyAsync(bj.p, J_, n * 8, hipMemcpyHostToDevice, stream())); J = bj.as<uint64_t>(); }
    bx.alloc(n * ts); GRB_HIP(hipMemcpyAsync(bx.p, X_, n * ts, hipMemcpyHostToDevice, stream())); X = bx.p;
  }
};
static void build_refusals(const BuildResult& r) {
  if (r.status == BUILD_OUT_OF_BOUNDS) fail(GrB_INDEX_OUT_OF_BOUNDS, "build: index out of bounds");
  if (r.status == BUILD_DUPLICATE) fail(GrB_INVALID_VALUE, "build: duplicate index and no dup operator");
}
// false: the longest run is beyond the device fold (nothing was written: the host route takes the call)
static bool mat_build_device(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const void* X, GrB_Index n, GrB_BinaryOp dup, int location) {
  BuildStage st(I, J, X, n, C->type->size, location);
  DevBuf rows, col, val;
  const BuildResult r0 = build_from_tuples(C->type->code, st.I, st.J, st.X, n, C->nrows, C->ncols, dup ? dup->opcode : -1, rows, &col, val);
  build_refusals(r0);
  if (r0.status == BUILD_RUN_TOO_LONG) return false;
  BuildResult r = r0;
  DevCSR T; T.nrows = (uint32_t)C->nrows; T.ncols = (uint32_t)C->ncols; T.nnz = r.nvals;
  T.rowptr.alloc(((size_t)T.nrows + 1) * 4);
  r.search = build_rowptr(rows.as<uint32_t>(), r.nvals, T.nrows, T.rowptr.as<uint32_t>());
  T.col = std::move(col); T.val = std::move(val); T.valid = true;
  GRB_HIP(hipStreamSynchronize(stream()));                     // the staged tuples and the row list go out of scope
  mat_invalidate_host(C);                                      // the image is replaced as a whole: mirror, edit queue, csc, bm and everything derived go (CsrDerived::structure_changed)
  C->csr = std::move(T); C->dev_valid = true;
  g_last_plan = build_plan(C->type, dup, r);
  return true;
}
static bool vec_build_device(GrB_Vector w, const GrB_Index* I, const void* X, GrB_Index n, GrB_BinaryOp dup, int location) {
  const size_t ts = w->type->size; const uint64_t len = w->n;
  BuildStage st(I, nullptr, X, n, ts, location);
  DevBuf idx, val;
  const BuildResult r = build_from_tuples(w->type->code, st.I, nullptr, st.X, n, len, 1, dup ? dup->opcode : -1, idx, nullptr, val);
  build_refusals(r);
  if (r.status == BUILD_RUN_TOO_LONG) return false;
  DevBuf nval(len * ts ? len * ts : 1), npres(len ? len : 1);
  if (len) { GRB_HIP(hipMemsetAsync(nval.p, 0, len * ts, stream())); GRB_HIP(hipMemsetAsync(npres.p, 0, len, stream())); }
  if (r.nvals) scatter_entries((uint32_t)r.nvals, idx.as<uint32_t>(), val.p, ts, nval.p, npres.as<uint8_t>());
  GRB_HIP(hipStreamSynchronize(stream()));
  vec_invalidate_host(w, r.nvals, true);                       // facts.image_replaced(nvals, known): the count is the fold's, no count kernel
  w->dval = std::move(nval); w->dpres = std::move(npres); w->dev_valid = true;
  g_last_plan = build_plan(w->type, dup, r) + (r.nvals ? "k_scatter_entries " : "");
  return true;
}
// the host route of a call whose tuples are device arrays: downloaded once
struct BuildHostCopy {
  std::vector<GrB_Index> I, J; std::vector<uint8_t> X;
  BuildHostCopy(const GrB_Index* dI, const GrB_Index* dJ, const void* dX, GrB_Index n, size_t xs) {
    need_device(); I.resize(n); if (dJ) J.resize(n); X.resize(n * xs);
    if (!n) return;
    GRB_HIP(hipMemcpyAsync(I.data(), dI, n * 8, hipMemcpyDeviceToHost, stream()));
    if (dJ) GRB_HIP(hipMemcpyAsync(J.data(), dJ, n * 8, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipMemcpyAsync(X.data(), dX, n * xs, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  }
};
static void build_plan_host() { if (g_last_plan.compare(0, 6, "build<") == 0) g_last_plan.clear(); }      // (a host-route build launches nothing: an earlier build's word must not pass for its own)

}  // namespace grb

using namespace grb;

#define CHECK_MAT(A) do { if (!(A)) return GrB_NULL_POINTER; if (!check_obj(A)) return GrB_UNINITIALIZED_OBJECT; } while (0)
#define CHECK_VEC(v) CHECK_MAT(v)

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
    if (mat_edits_queued(A)) g_last_plan.clear();
    m->format = A->format; m->sparsity_control = A->sparsity_control; m->hyper_switch = A->hyper_switch;
    if (A->iso_full) { m->iso_full = true; memcpy(m->iso_val, A->iso_val, 16); }
    else if (A->host_valid) { mat_host_assemble(A); m->hi = A->hi; m->hj = A->hj; m->hx = A->hx; m->host_valid = true; }
    else if (mat_bitmap_only(A)) {                             // a batch matrix that lives as a bitmap: so does its copy
      const size_t np = (size_t)A->nrows * A->ncols, ts = A->type->size;
      m->bm.val.alloc(np * ts + 64); m->bm.pres.alloc(np + 64);
      GRB_HIP(hipMemcpyAsync(m->bm.val.p, A->bm.val.p, np * ts, hipMemcpyDeviceToDevice, stream()));
      GRB_HIP(hipMemcpyAsync(m->bm.pres.p, A->bm.pres.p, np, hipMemcpyDeviceToDevice, stream()));
      m->bm.valid = true; m->bm.nvals = A->bm.nvals; m->bm.nvals_known = A->bm.nvals_known; m->host_valid = false; m->dev_valid = false;
    } else {
      mat_edit_flush(A);
      const DevCSR& s = A->csr; DevCSR& d = m->csr; const size_t ts = A->type->size;
      d.nrows = s.nrows; d.ncols = s.ncols; d.nnz = s.nnz;
      d.rowptr.alloc(((size_t)s.nrows + 1) * 4); d.col.alloc(s.nnz * 4); d.val.alloc(s.nnz * ts);
      GRB_HIP(hipMemcpyAsync(d.rowptr.p, s.rowptr.p, ((size_t)s.nrows + 1) * 4, hipMemcpyDeviceToDevice, stream()));
      if (s.nnz) { GRB_HIP(hipMemcpyAsync(d.col.p, s.col.p, s.nnz * 4, hipMemcpyDeviceToDevice, stream()));
                   GRB_HIP(hipMemcpyAsync(d.val.p, s.val.p, s.nnz * ts, hipMemcpyDeviceToDevice, stream())); }
      d.valid = true; m->dev_valid = true; m->host_valid = false;
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
  if (!n) return GrB_NULL_POINTER; CHECK_MAT(A); return guarded(A, [&] { if (mat_edits_queued(A)) g_last_plan.clear(); *n = mat_nvals(A); });
}
GrB_Info GrB_Matrix_wait(GrB_Matrix* A) {
  if (!A) return GrB_NULL_POINTER; CHECK_MAT(*A);
  return guarded(*A, [&] { if ((*A)->host_valid && !(*A)->iso_full) mat_host_assemble(*A); if (mat_edits_queued(*A)) g_last_plan.clear(); mat_edit_flush(*A); if (device_ok()) GRB_HIP(hipStreamSynchronize(stream())); });
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
GrB_Info GrB_Matrix_removeElement(GrB_Matrix A, GrB_Index i, GrB_Index j) {
  CHECK_MAT(A); if (i >= A->nrows || j >= A->ncols) return GrB_INVALID_INDEX;
  return guarded(A, [&] {
    GrB_Matrix_opaque::Pending p{i, j, true, {0}};
    if (mat_edit_route(A)) { A->pending.push_back(p); A->bm.clear(); return; }      // it lives in HBM: queued for the device (the bitmap cache beside the CSR has its own readers: dropped now)
    mat_to_host(A); A->pending.push_back(p); mat_invalidate_device(A); });
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

static GrB_Info mat_build(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const void* X, int xcode, GrB_Index n, GrB_BinaryOp dup, int location = 0) {
  CHECK_MAT(C); if (n && (!I || !J || !X)) return GrB_NULL_POINTER;
  if (dup && !check_obj(dup)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    if (mat_nvals(C) != 0) fail(GrB_OUTPUT_NOT_EMPTY, "build: output already has entries");
    if (build_takes_device(C->type, C->iso_full, xcode, n, C->nrows, C->ncols, dup) && mat_build_device(C, I, J, X, n, dup, location)) return;
    build_plan_host();
    if (location) { const BuildHostCopy h(I, J, X, n, type_size(xcode)); build_tuples(C->type, h.I.data(), h.J.data(), h.X.data(), xcode, n, C->nrows, C->ncols, dup, C->hi, &C->hj, C->hx); }
    else build_tuples(C->type, I, J, X, xcode, n, C->nrows, C->ncols, dup, C->hi, &C->hj, C->hx);
    C->host_valid = true; mat_invalidate_device(C);
  });
}
// a matrix that lives in HBM only and is large (`paths[i, source] = 1` on a dense ns x n batch, gap/bcmark.py:23: bringing 134 MB to
// the host mirror for one value was a third of the algorithm): the entry is looked up on the device; an existing one is read or
// overwritten in place (what changes with the values — the transpose cache, a kernel-X plan's copy — is dropped)
// (a caller that touches many elements one by one is better served by the host mirror: one transfer, then no round trips)
static bool mat_device_only(GrB_Matrix A) { return A->dev_elem_ops++ < 32 && device_ok() && A->dev_valid && !A->host_valid && A->pending.empty() && !A->iso_full && A->csr.valid && A->csr.nnz >= (1u << 16) && A->type->code < T_FC32; }
static GrB_Info mat_set(GrB_Matrix C, const void* x, int xcode, GrB_Index i, GrB_Index j) {
  CHECK_MAT(C); if (i >= C->nrows || j >= C->ncols) return GrB_INVALID_INDEX;
  return guarded(C, [&] {
    if (mat_device_only(C)) {
      const uint64_t pos = csr_find_entry(C->csr, (uint32_t)i, (uint32_t)j);
      if (pos != ~0ull) {
        uint8_t* pin = (uint8_t*)pinned_scratch() + 64; cast_scalar(C->type->code, pin, xcode, x);
        GRB_HIP(hipMemcpyAsync((uint8_t*)C->csr.val.p + pos * C->type->size, pin, C->type->size, hipMemcpyHostToDevice, stream()));
        GRB_HIP(hipStreamSynchronize(stream()));
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
  size_t lo = 0, hi = A->hi.size();
  while (lo < hi) { size_t m = (lo + hi) / 2; if (A->hi[m] < i || (A->hi[m] == i && A->hj[m] < j)) lo = m + 1; else hi = m; }
  return (lo < A->hi.size() && A->hi[lo] == i && A->hj[lo] == j) ? lo : SIZE_MAX;
}
static GrB_Info mat_get(void* x, int xcode, GrB_Matrix A, GrB_Index i, GrB_Index j) {
  if (!x) return GrB_NULL_POINTER; CHECK_MAT(A); if (i >= A->nrows || j >= A->ncols) return GrB_INVALID_INDEX;
  GrB_Info r = GrB_SUCCESS;
  GrB_Info info = guarded(A, [&] {
    if (A->iso_full) { cast_scalar(xcode, x, A->type->code, A->iso_val); return; }
    if (mat_edits_queued(A)) {                                 // the last queued edit of the coordinate answers; else the device image does, edits applied
      if (const auto* e = edit_lookup(A->pending, [&](const GrB_Matrix_opaque::Pending& q) { return q.i == i && q.j == j; })) {
        if (e->del) r = GrB_NO_VALUE; else cast_scalar(xcode, x, A->type->code, e->x); return; }
      g_last_plan.clear(); mat_edit_flush(A);
    }
    if (mat_device_only(A)) {
      const uint64_t pos = csr_find_entry(A->csr, (uint32_t)i, (uint32_t)j);
      if (pos == ~0ull) { r = GrB_NO_VALUE; return; }
      uint8_t* pin = (uint8_t*)pinned_scratch() + 64;
      GRB_HIP(hipMemcpyAsync(pin, (const uint8_t*)A->csr.val.p + pos * A->type->size, A->type->size, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
      cast_scalar(xcode, x, A->type->code, pin); return;
    }
    mat_to_host(A); size_t k = mat_find(A, i, j);
    if (k == SIZE_MAX) r = GrB_NO_VALUE; else cast_scalar(xcode, x, A->type->code, &A->hx[k * A->type->size]); });
  return info ? info : r;
}
static GrB_Info mat_tuples(GrB_Index* I, GrB_Index* J, void* X, int xcode, GrB_Index* n, GrB_Matrix A) {
  if (!n) return GrB_NULL_POINTER; CHECK_MAT(A);
  return guarded(A, [&] {
    if (mat_edits_queued(A)) g_last_plan.clear();
    mat_to_host(A); const GrB_Index nv = A->hi.size();
    if ((I || J || X) && *n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
    const size_t ts = A->type->size, xs = type_size(xcode);
    for (GrB_Index k = 0; k < nv; k++) {
      if (I) I[k] = A->hi[k]; if (J) J[k] = A->hj[k];
      if (X) cast_scalar(xcode, (uint8_t*)X + k * xs, A->type->code, &A->hx[k * ts]);
    }
    *n = nv;
  });
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
    if (vec_edits_queued(u)) g_last_plan.clear();
    vec_gate(u);
    if (u->iso_full) { r->iso_full = true; memcpy(r->iso_val, u->iso_val, 16); }
    else if (u->host_valid) { vec_host_assemble(u); r->hi = u->hi; r->hx = u->hx; }
    else {
      const size_t ts = u->type->size;
      r->dval.alloc(u->n * ts ? u->n * ts : 1); r->dpres.alloc(u->n ? u->n : 1);
      if (u->n) dev_copy2(r->dval.p, u->dval.p, u->n * ts, r->dpres.p, u->dpres.p, u->n);
      r->facts.image_replaced(u->facts.dnvals, u->facts.dnvals_known); r->dev_valid = true; r->host_valid = false;
    }
  });
  if (info) { GrB_Vector_free(&r); return info; }
  *w = r; return GrB_SUCCESS;
}
GrB_Info GrB_Vector_clear(GrB_Vector v) { CHECK_VEC(v); if (v->lazy | v->q_reads) { GrB_Info e = guarded(v, [&] { vec_overwritten(v); }); if (e) return e; } v->hi.clear(); v->hx.clear(); v->pending.clear(); v->host_valid = true; v->iso_full = false; vec_invalidate_device(v); return GrB_SUCCESS; }
GrB_Info GrB_Vector_size(GrB_Index* n, const GrB_Vector v) { if (!n) return GrB_NULL_POINTER; CHECK_VEC(v); *n = v->n; return GrB_SUCCESS; }
GrB_Info GrB_Vector_nvals(GrB_Index* n, const GrB_Vector v) { if (!n) return GrB_NULL_POINTER; CHECK_VEC(v); return guarded(v, [&] { if (vec_edits_queued(v)) g_last_plan.clear(); *n = vec_nvals(v); }); }
GrB_Info GrB_Vector_wait(GrB_Vector* v) {
  if (!v) return GrB_NULL_POINTER; CHECK_VEC(*v);
  return guarded(*v, [&] { if (vec_edits_queued(*v)) g_last_plan.clear(); vec_gate(*v); if ((*v)->host_valid) vec_host_assemble(*v); if (device_ok()) GRB_HIP(hipStreamSynchronize(stream())); });
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
        DevBuf nval(n * ts ? n * ts : 1), npres(n ? n : 1);
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
GrB_Info GrB_Vector_removeElement(GrB_Vector v, GrB_Index i) {
  CHECK_VEC(v); if (i >= v->n) return GrB_INVALID_INDEX;
  return guarded(v, [&] {
    GrB_Vector_opaque::Pending p{i, true, {0}};
    if (!v->host_valid && !v->iso_full) { if (v->lazy | v->q_reads) vec_resolve(v); if (vec_edit_route(v)) { v->pending.push_back(p); v->facts.image_replaced(0, false); return; } }      // it lives in HBM (a deferred chain completed first): queued for the device
    vec_to_host(v); v->pending.push_back(p); vec_invalidate_device(v); });
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
static GrB_Info vec_build(GrB_Vector w, const GrB_Index* I, const void* X, int xcode, GrB_Index n, GrB_BinaryOp dup, int location = 0) {
  CHECK_VEC(w); if (n && (!I || !X)) return GrB_NULL_POINTER; if (dup && !check_obj(dup)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] {
    if (vec_nvals(w) != 0) fail(GrB_OUTPUT_NOT_EMPTY, "build: output already has entries");
    if (build_takes_device(w->type, w->iso_full, xcode, n, w->n, 1, dup) && vec_build_device(w, I, X, n, dup, location)) return;
    build_plan_host();
    if (location) { const BuildHostCopy h(I, nullptr, X, n, type_size(xcode)); build_tuples(w->type, h.I.data(), nullptr, h.X.data(), xcode, n, w->n, 1, dup, w->hi, nullptr, w->hx); }
    else build_tuples(w->type, I, nullptr, X, xcode, n, w->n, 1, dup, w->hi, nullptr, w->hx);
    w->host_valid = true; vec_invalidate_device(w);
  });
}
static GrB_Info vec_set(GrB_Vector w, const void* x, int xcode, GrB_Index i) {
  CHECK_VEC(w); if (i >= w->n) return GrB_INVALID_INDEX;
  return guarded(w, [&] { if (w->iso_full) fail(GrB_INSUFFICIENT_SPACE, ISO_MSG);
    GrB_Vector_opaque::Pending p{i, false, {0}}; cast_scalar(w->type->code, p.x, xcode, x);
    if (!w->host_valid) { if (w->lazy | w->q_reads) vec_resolve(w); if (vec_edit_route(w)) { w->pending.push_back(p); w->facts.image_replaced(0, false); return; } vec_to_host(w); }      // it lives in HBM (a deferred chain completed first): queued for the device
    w->pending.push_back(p); vec_invalidate_device(w); });
}
static GrB_Info vec_get(void* x, int xcode, GrB_Vector v, GrB_Index i) {
  if (!x) return GrB_NULL_POINTER; CHECK_VEC(v); if (i >= v->n) return GrB_INVALID_INDEX;
  GrB_Info r = GrB_SUCCESS;
  GrB_Info info = guarded(v, [&] {
    if (v->iso_full) { cast_scalar(xcode, x, v->type->code, v->iso_val); return; }
    if (vec_edits_queued(v)) {                                 // the last queued edit of the position answers; else the device image does, edits applied (vec_gate)
      if (const auto* e = edit_lookup(v->pending, [&](const GrB_Vector_opaque::Pending& q) { return q.i == i; })) {
        if (e->del) r = GrB_NO_VALUE; else cast_scalar(xcode, x, v->type->code, e->x); return; }
      g_last_plan.clear();
    }
    vec_gate(v);
    // a large vector that lives in HBM only (`r[vertex]` after a PageRank): the presence byte and the value come over alone — a few
    // dozen reads in a row, then the host mirror takes over (one transfer, no more round trips)
    if (device_ok() && v->dev_valid && !v->host_valid && v->pending.empty() && v->n >= (1u << 16) && v->type->code < T_FC32 && v->dev_elem_ops++ < 32) {
      uint8_t* pin = (uint8_t*)pinned_scratch() + 64; const size_t ts = v->type->size;
      GRB_HIP(hipMemcpyAsync(pin, v->dpres.as<uint8_t>() + i, 1, hipMemcpyDeviceToHost, stream()));
      GRB_HIP(hipMemcpyAsync(pin + 16, (const uint8_t*)v->dval.p + i * ts, ts, hipMemcpyDeviceToHost, stream()));
      GRB_HIP(hipStreamSynchronize(stream()));
      if (!pin[0]) r = GrB_NO_VALUE; else cast_scalar(xcode, x, v->type->code, pin + 16);
      return;
    }
    vec_to_host(v);
    auto it = std::lower_bound(v->hi.begin(), v->hi.end(), i);
    if (it == v->hi.end() || *it != i) r = GrB_NO_VALUE;
    else cast_scalar(xcode, x, v->type->code, &v->hx[(it - v->hi.begin()) * v->type->size]); });
  return info ? info : r;
}
static GrB_Info vec_tuples(GrB_Index* I, void* X, int xcode, GrB_Index* n, GrB_Vector v) {
  if (!n) return GrB_NULL_POINTER; CHECK_VEC(v);
  return guarded(v, [&] {
    if (vec_edits_queued(v)) g_last_plan.clear();
    vec_to_host(v); const GrB_Index nv = v->hi.size();
    if ((I || X) && *n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
    const size_t ts = v->type->size, xs = type_size(xcode);
    for (GrB_Index k = 0; k < nv; k++) { if (I) I[k] = v->hi[k]; if (X) cast_scalar(xcode, (uint8_t*)X + k * xs, v->type->code, &v->hx[k * ts]); }
    *n = nv;
  });
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

// ---- typed families ---------------------------------------------------------------------------------
#define GRB_TYPED_CONTAINER(SUF, CT, CODE) \
  GrB_Info GrB_Matrix_build_##SUF(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const CT* X, GrB_Index n, const GrB_BinaryOp dup) { return mat_build(C, I, J, X, CODE, n, dup); } \
  GrB_Info GrB_Matrix_setElement_##SUF(GrB_Matrix C, CT x, GrB_Index i, GrB_Index j) { return mat_set(C, &x, CODE, i, j); } \
  GrB_Info GrB_Matrix_extractElement_##SUF(CT* x, const GrB_Matrix A, GrB_Index i, GrB_Index j) { return mat_get(x, CODE, A, i, j); } \
  GrB_Info GrB_Matrix_extractTuples_##SUF(GrB_Index* I, GrB_Index* J, CT* X, GrB_Index* n, const GrB_Matrix A) { return mat_tuples(I, J, X, CODE, n, A); } \
  GrB_Info GrB_Vector_build_##SUF(GrB_Vector w, const GrB_Index* I, const CT* X, GrB_Index n, const GrB_BinaryOp dup) { return vec_build(w, I, X, CODE, n, dup); } \
  GrB_Info GrB_Vector_setElement_##SUF(GrB_Vector w, CT x, GrB_Index i) { return vec_set(w, &x, CODE, i); } \
  GrB_Info GrB_Vector_extractElement_##SUF(CT* x, const GrB_Vector v, GrB_Index i) { return vec_get(x, CODE, v, i); } \
  GrB_Info GrB_Vector_extractTuples_##SUF(GrB_Index* I, CT* X, GrB_Index* n, const GrB_Vector v) { return vec_tuples(I, X, CODE, n, v); } \
  GrB_Info GxB_Scalar_setElement_##SUF(GxB_Scalar s, CT x) { return scalar_set(s, &x, CODE); } \
  GrB_Info GxB_Scalar_extractElement_##SUF(CT* x, const GxB_Scalar s) { return scalar_get(x, CODE, s); }
GRB_TYPED_CONTAINER(BOOL, bool, T_BOOL) GRB_TYPED_CONTAINER(INT8, int8_t, T_INT8) GRB_TYPED_CONTAINER(UINT8, uint8_t, T_UINT8)
GRB_TYPED_CONTAINER(INT16, int16_t, T_INT16) GRB_TYPED_CONTAINER(UINT16, uint16_t, T_UINT16) GRB_TYPED_CONTAINER(INT32, int32_t, T_INT32)
GRB_TYPED_CONTAINER(UINT32, uint32_t, T_UINT32) GRB_TYPED_CONTAINER(INT64, int64_t, T_INT64) GRB_TYPED_CONTAINER(UINT64, uint64_t, T_UINT64)
GRB_TYPED_CONTAINER(FP32, float, T_FP32) GRB_TYPED_CONTAINER(FP64, double, T_FP64)

// complex entries: stored, set, read and listed on the host mirror (the reference's type registry, from_lists with
// complex values and Matrix.dense(FC64) need that much: tests/test_matrix.py:56-57,853); arithmetic on them is not offered
typedef struct { float re, im; } GxB_FC32_t;
typedef struct { double re, im; } GxB_FC64_t;
#define GRB_COMPLEX_CONTAINER(SUF, CT, CODE) \
  GrB_Info GxB_Matrix_build_##SUF(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const CT* X, GrB_Index n, const GrB_BinaryOp dup) { return mat_build(C, I, J, X, CODE, n, dup); } \
  GrB_Info GxB_Matrix_setElement_##SUF(GrB_Matrix C, CT x, GrB_Index i, GrB_Index j) { return mat_set(C, &x, CODE, i, j); } \
  GrB_Info GxB_Matrix_extractElement_##SUF(CT* x, const GrB_Matrix A, GrB_Index i, GrB_Index j) { return mat_get(x, CODE, A, i, j); } \
  GrB_Info GxB_Matrix_extractTuples_##SUF(GrB_Index* I, GrB_Index* J, CT* X, GrB_Index* n, const GrB_Matrix A) { return mat_tuples(I, J, X, CODE, n, A); } \
  GrB_Info GxB_Vector_build_##SUF(GrB_Vector w, const GrB_Index* I, const CT* X, GrB_Index n, const GrB_BinaryOp dup) { return vec_build(w, I, X, CODE, n, dup); } \
  GrB_Info GxB_Vector_setElement_##SUF(GrB_Vector w, CT x, GrB_Index i) { return vec_set(w, &x, CODE, i); } \
  GrB_Info GxB_Vector_extractElement_##SUF(CT* x, const GrB_Vector v, GrB_Index i) { return vec_get(x, CODE, v, i); } \
  GrB_Info GxB_Vector_extractTuples_##SUF(GrB_Index* I, CT* X, GrB_Index* n, const GrB_Vector v) { return vec_tuples(I, X, CODE, n, v); } \
  GrB_Info GxB_Scalar_setElement_##SUF(GxB_Scalar s, CT x) { return scalar_set(s, &x, CODE); } \
  GrB_Info GxB_Scalar_extractElement_##SUF(CT* x, const GxB_Scalar s) { return scalar_get(x, CODE, s); }
GRB_COMPLEX_CONTAINER(FC32, GxB_FC32_t, T_FC32) GRB_COMPLEX_CONTAINER(FC64, GxB_FC64_t, T_FC64)

// build from tuples that may live in HBM: I / J are 64-bit indices, X holds values of the container's own type; location 0 = host arrays, 1 = device arrays, which the
// device route reads where they are (the host route downloads them once, so that the call is total)
GrB_Info GrBX_Matrix_build_at(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const void* X, GrB_Index n, const GrB_BinaryOp dup, int location) {
  CHECK_MAT(C); if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  return mat_build(C, I, J, X, C->type->code, n, dup, location);
}
GrB_Info GrBX_Vector_build_at(GrB_Vector w, const GrB_Index* I, const void* X, GrB_Index n, const GrB_BinaryOp dup, int location) {
  CHECK_VEC(w); if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  return vec_build(w, I, X, w->type->code, n, dup, location);
}
GrB_Info GrBX_build_thresholds(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = BUILD_DEVICE_MIN_TUPLES; out[1] = BUILD_RUN_SERIAL; out[2] = BUILD_RUN_SERIAL_MAX; return GrB_SUCCESS;
}

// extractTuples into arrays that may live in HBM (kernels: grb_tuples.hip).  location 0 IS GrB_*_extractTuples_<own type>; location 1: I / J / X are device arrays,
// the call is the same flush point (queued edits, deferred element-wise work), and a container that has an HBM layout is expanded where it lives — uploaded first
// when it is host-resident only, its CSR made first when it is a bitmap-only batch matrix — without a host mirror being built: what lived in HBM only still does.
// A container without an HBM layout (complex, a dimension beyond GRB_DIM_DEVICE_MAX, a full one-valued one) takes the host route and its mirror is copied up once.
static void tuples_plan_host() { if (g_last_plan.compare(0, 7, "tuples<") == 0) g_last_plan.clear(); }      // (the host route launches nothing: an earlier call's word must not pass for its own)
static std::string tuples_plan(const char* on, bool i, bool j, bool x, const char* kernels) {
  return std::string("tuples<on=") + on + ",i=" + (i ? "1" : "0") + ",j=" + (j ? "1" : "0") + ",x=" + (x ? "1" : "0") + "> " + kernels;
}
static void tuples_copy_up(void* dst, const void* src, size_t bytes) { if (dst && bytes) GRB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream())); }
GrB_Info GrBX_Matrix_extractTuples_at(GrB_Index* I, GrB_Index* J, void* X, GrB_Index* n, const GrB_Matrix A, int location) {
  if (!n) return GrB_NULL_POINTER; CHECK_MAT(A); if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  if (location == 0) { tuples_plan_host(); return mat_tuples(I, J, X, A->type->code, n, A); }
  return guarded(A, [&] {
    need_device();
    const bool any = I || J || X; const size_t ts = A->type->size;
    if (A->iso_full || A->type->code >= T_FC32 || A->nrows > GRB_DIM_DEVICE_MAX || A->ncols > GRB_DIM_DEVICE_MAX) {
      tuples_plan_host();
      mat_to_host(A); const GrB_Index nv = A->hi.size();
      if (any && *n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
      tuples_copy_up(I, A->hi.data(), nv * 8); tuples_copy_up(J, A->hj.data(), nv * 8); tuples_copy_up(X, A->hx.data(), nv * ts);
      GRB_HIP(hipStreamSynchronize(stream()));
      *n = nv; return;
    }
    const bool queued = mat_edits_queued(A);
    if (queued) g_last_plan.clear();                           // a flush point of its own: the flush's word goes in front of this call's
    mat_to_device(A);                                          // the flush, the CSR of a bitmap-only batch matrix, the upload of a host-resident matrix
    const GrB_Index nv = A->csr.nnz;
    if (any && *n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
    const bool launch = any && nv;
    if (launch) tuples_from_csr(A->csr, ts, I, J, X);
    g_last_plan = (queued ? g_last_plan : std::string()) + tuples_plan("matrix", I, J, X, launch ? "k_tuples_csr " : "");
    GRB_HIP(hipStreamSynchronize(stream()));
    *n = nv;
  });
}
GrB_Info GrBX_Vector_extractTuples_at(GrB_Index* I, void* X, GrB_Index* n, const GrB_Vector v, int location) {
  if (!n) return GrB_NULL_POINTER; CHECK_VEC(v); if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  if (location == 0) { tuples_plan_host(); return vec_tuples(I, X, v->type->code, n, v); }
  return guarded(v, [&] {
    need_device();
    const bool any = I || X; const size_t ts = v->type->size;
    if (v->iso_full || v->type->code >= T_FC32 || v->n > GRB_DIM_DEVICE_MAX) {
      tuples_plan_host();
      vec_to_host(v); const GrB_Index nv = v->hi.size();
      if (any && *n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
      tuples_copy_up(I, v->hi.data(), nv * 8); tuples_copy_up(X, v->hx.data(), nv * ts);
      GRB_HIP(hipStreamSynchronize(stream()));
      *n = nv; return;
    }
    const bool queued = vec_edits_queued(v);
    if (queued) g_last_plan.clear();
    vec_to_device(v);                                          // vec_gate: the deferred chain that writes v completes, queued edits are applied; then the upload of a host-resident vector
    const uint64_t len = v->n; const char* kernels = "";
    GrB_Index nv = 0;
    if (!any) nv = vec_dev_nvals(v);
    else if (v->facts.dnvals_known && (v->facts.dnvals == len || v->facts.dnvals == 0)) {      // the facts record already says "all present" (or "none"): no count pass
      nv = v->facts.dnvals;
      if (*n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
      if (nv) { tuples_from_full(v->dval.p, ts, len, I, X); kernels = "k_tuples_iota "; }
    } else {
      DevBuf offs;
      nv = tuples_count_bitmap(v->dpres.as<uint8_t>(), len, offs);
      v->facts.dnvals = nv; v->facts.dnvals_known = true;        // (learnt by reading the image: recorded without a transition, as vec_dev_nvals does)
      if (*n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small");
      kernels = "k_tuples_count ";
      if (nv) { tuples_from_bitmap(v->dpres.as<uint8_t>(), v->dval.p, ts, len, offs, I, X); kernels = "k_tuples_count k_tuples_scatter "; }
      GRB_HIP(hipStreamSynchronize(stream()));                   // `offs` goes out of scope
    }
    g_last_plan = (queued ? g_last_plan : std::string()) + tuples_plan("vector", I, false, X, kernels);
    GRB_HIP(hipStreamSynchronize(stream()));
    *n = nv;
  });
}
GrB_Info GrBX_tuples_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = TUPLES_TILE; out[1] = TUPLES_VEC_TILE; out[2] = TUPLES_GRID_CAP; return GrB_SUCCESS;
}

// =================================== bulk / device import-export ===================================
GrB_Info GrBX_Matrix_import_CSR(GrB_Matrix* A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, GrB_Index nvals,
                                const uint32_t* rowptr, const uint32_t* colidx, const void* values, int location) {
  if (!A || !rowptr || (nvals && (!colidx || !values))) return GrB_NULL_POINTER;
  GrB_Matrix m = nullptr; GrB_Info info = GrB_Matrix_new(&m, type, nrows, ncols); if (info) return info;
  info = guarded(m, [&] {
    need_device();
    if (nrows > GRB_DIM_DEVICE_MAX || ncols > GRB_DIM_DEVICE_MAX || nvals > 0xFFFFFFF0ull) fail(GrB_INSUFFICIENT_SPACE, "import_CSR: 32-bit index range exceeded");
    DevCSR& c = m->csr; const size_t ts = type->size;
    c.nrows = (uint32_t)nrows; c.ncols = (uint32_t)ncols; c.nnz = nvals;
    c.rowptr.alloc((nrows + 1) * 4); c.col.alloc(nvals * 4); c.val.alloc(nvals * ts);
    hipMemcpyKind k = location ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    GRB_HIP(hipMemcpyAsync(c.rowptr.p, rowptr, (nrows + 1) * 4, k, stream()));
    if (nvals) { GRB_HIP(hipMemcpyAsync(c.col.p, colidx, nvals * 4, k, stream())); GRB_HIP(hipMemcpyAsync(c.val.p, values, nvals * ts, k, stream())); }
    GRB_HIP(hipStreamSynchronize(stream()));
    c.valid = true; m->dev_valid = true; m->host_valid = false;
  });
  if (info) { GrB_Matrix_free(&m); return info; }
  *A = m; return GrB_SUCCESS;
}
GrB_Info GrBX_Matrix_export_CSR(const GrB_Matrix A, uint32_t* rowptr, uint32_t* colidx, void* values, int location) {
  CHECK_MAT(A);
  return guarded(A, [&] {
    mat_to_device(A); const DevCSR& c = A->csr; const size_t ts = A->type->size;
    hipMemcpyKind k = location ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (rowptr) GRB_HIP(hipMemcpyAsync(rowptr, c.rowptr.p, ((size_t)c.nrows + 1) * 4, k, stream()));
    if (colidx && c.nnz) GRB_HIP(hipMemcpyAsync(colidx, c.col.p, c.nnz * 4, k, stream()));
    if (values && c.nnz) GRB_HIP(hipMemcpyAsync(values, c.val.p, c.nnz * ts, k, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  });
}
GrB_Info GrBX_Vector_import_Bitmap(GrB_Vector* v, GrB_Type type, GrB_Index n, const void* values, const uint8_t* present, int location) {
  if (!v || (n && !values)) return GrB_NULL_POINTER;
  GrB_Vector w = nullptr; GrB_Info info = GrB_Vector_new(&w, type, n); if (info) return info;
  info = guarded(w, [&] {
    need_device(); if (n > GRB_DIM_DEVICE_MAX) fail(GrB_INSUFFICIENT_SPACE, "import: vector too long");
    const size_t ts = type->size; hipMemcpyKind k = location ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    w->dval.alloc(n * ts ? n * ts : 1); w->dpres.alloc(n ? n : 1);
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
