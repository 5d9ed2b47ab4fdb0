// grb_build_ops.cpp — build from tuples: GrB_*_build_<T> (through mat_build / vec_build), GrBX_*_build_at.  The host route sorts and folds on the host mirror;
// the device route runs the kernels of grb_build.hip.
#include "grb_container.hpp"
#include "grb_userop.hpp"
#include "grb_build.hpp"
#include <algorithm>
#include <numeric>
#include <string.h>

namespace grb {

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
  auto [nval, npres] = vec_alloc_image(len, ts, true);
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

GrB_Info mat_build(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const void* X, int xcode, GrB_Index n, GrB_BinaryOp dup, int location) {
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
GrB_Info vec_build(GrB_Vector w, const GrB_Index* I, const void* X, int xcode, GrB_Index n, GrB_BinaryOp dup, int location) {
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

}  // namespace grb

using namespace grb;

extern "C" {

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

}  // extern "C"
