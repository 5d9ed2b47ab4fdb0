// grb_tuples_ops.cpp — extractTuples: GrB_*_extractTuples_<T> (through mat_tuples / vec_tuples, the host mirror), GrBX_*_extractTuples_at (arrays that may
// live in HBM: the kernels of grb_tuples.hip).
#include "grb_container.hpp"
#include "grb_tuples.hpp"

namespace grb {

static void tuples_capacity(bool any, GrB_Index n, GrB_Index nv) { if (any && n < nv) fail(GrB_INSUFFICIENT_SPACE, "extractTuples: output arrays too small"); }

GrB_Info mat_tuples(GrB_Index* I, GrB_Index* J, void* X, int xcode, GrB_Index* n, GrB_Matrix A) {
  if (!n) return GrB_NULL_POINTER; CHECK_MAT(A);
  return guarded(A, [&] {
    flush_point(A);
    mat_to_host(A); const GrB_Index nv = A->hi.size();
    tuples_capacity(I || J || X, *n, nv);
    const size_t ts = A->type->size, xs = type_size(xcode);
    for (GrB_Index k = 0; k < nv; k++) {
      if (I) I[k] = A->hi[k]; if (J) J[k] = A->hj[k];
      if (X) cast_scalar(xcode, (uint8_t*)X + k * xs, A->type->code, &A->hx[k * ts]);
    }
    *n = nv;
  });
}
GrB_Info vec_tuples(GrB_Index* I, void* X, int xcode, GrB_Index* n, GrB_Vector v) {
  if (!n) return GrB_NULL_POINTER; CHECK_VEC(v);
  return guarded(v, [&] {
    flush_point(v);
    vec_to_host(v); const GrB_Index nv = v->hi.size();
    tuples_capacity(I || X, *n, nv);
    const size_t ts = v->type->size, xs = type_size(xcode);
    for (GrB_Index k = 0; k < nv; k++) { if (I) I[k] = v->hi[k]; if (X) cast_scalar(xcode, (uint8_t*)X + k * xs, v->type->code, &v->hx[k * ts]); }
    *n = nv;
  });
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

}  // namespace grb

using namespace grb;

extern "C" {

GrB_Info GrBX_Matrix_extractTuples_at(GrB_Index* I, GrB_Index* J, void* X, GrB_Index* n, const GrB_Matrix A, int location) {
  if (!n) return GrB_NULL_POINTER; CHECK_MAT(A); if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  if (location == 0) { tuples_plan_host(); return mat_tuples(I, J, X, A->type->code, n, A); }
  return guarded(A, [&] {
    need_device();
    const bool any = I || J || X; const size_t ts = A->type->size;
    if (A->iso_full || A->type->code >= T_FC32 || A->nrows > GRB_DIM_DEVICE_MAX || A->ncols > GRB_DIM_DEVICE_MAX) {
      tuples_plan_host();
      mat_to_host(A); const GrB_Index nv = A->hi.size();
      tuples_capacity(any, *n, nv);
      tuples_copy_up(I, A->hi.data(), nv * 8); tuples_copy_up(J, A->hj.data(), nv * 8); tuples_copy_up(X, A->hx.data(), nv * ts);
      GRB_HIP(hipStreamSynchronize(stream()));
      *n = nv; return;
    }
    const bool queued = flush_point(A);                        // a flush point of its own: the flush's word goes in front of this call's
    mat_to_device(A);                                          // the flush, the CSR of a bitmap-only batch matrix, the upload of a host-resident matrix
    const GrB_Index nv = A->csr.nnz;
    tuples_capacity(any, *n, nv);
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
      tuples_capacity(any, *n, nv);
      tuples_copy_up(I, v->hi.data(), nv * 8); tuples_copy_up(X, v->hx.data(), nv * ts);
      GRB_HIP(hipStreamSynchronize(stream()));
      *n = nv; return;
    }
    const bool queued = flush_point(v);
    vec_to_device(v);                                          // vec_gate: the deferred chain that writes v completes, queued edits are applied; then the upload of a host-resident vector
    const uint64_t len = v->n; const char* kernels = "";
    GrB_Index nv = 0;
    if (!any) nv = vec_dev_nvals(v);
    else if (v->facts.dnvals_known && (v->facts.dnvals == len || v->facts.dnvals == 0)) {      // the facts record already says "all present" (or "none"): no count pass
      nv = v->facts.dnvals;
      tuples_capacity(true, *n, nv);
      if (nv) { tuples_from_full(v->dval.p, ts, len, I, X); kernels = "k_tuples_iota "; }
    } else {
      DevBuf offs;
      nv = tuples_count_bitmap(v->dpres.as<uint8_t>(), len, offs);
      v->facts.dnvals = nv; v->facts.dnvals_known = true;        // (learnt by reading the image: recorded without a transition, as vec_dev_nvals does)
      tuples_capacity(true, *n, nv);
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

}  // extern "C"
