// grb_host_ops.cpp — index-list extract / assign and kronecker (host mirror, or HBM for device-resident and large containers).
//
//   GrB_Vector_extract, GrB_Col_extract, GrB_Matrix_extract     <- Vector / Matrix slicing  (pygraphblas/vector.py:1526-1573, matrix.py:2807-2990)
//   GrB_Vector_assign, GrB_Row_assign, GrB_Col_assign, GrB_Matrix_assign <- slice assignment (vector.py:1447-1492, matrix.py:2992-3130)
//   GrB_Matrix_kronecker_BinaryOp / _Monoid / _Semiring, GxB_kron <- Matrix.kronecker, Matrix.kronpow (matrix.py:2739-2805, 1732-1757)
//   GxB_{Matrix,Vector}_apply_BinaryOp1st/2nd                   <- apply_first / apply_second with a Scalar (matrix.py:1999-2004, 2034-2039)
//   GxB_Matrix_diag, GxB_Vector_diag                            <- Matrix.from_diag, Matrix.vector_diag (matrix.py:333-375, 2225-2277)
//
// None of these is on the hot path (mxm / mxv / vxm and the O(n) / O(nnz) operations of the BFS, PageRank and
// triangle-count loops, all HIP): they are the element-wise container surface — notebook slicing `M[2]`, `v[1:3]`,
// `M[1, :] = v` — beside setElement / extractElement, and like those they edit the host mirror of the container (sorted
// tuples); the HBM image is rebuilt lazily the next time a kernel needs it.  Semantics: C API 1.3: T is
// formed, then C<M,replace> = accum(C, T); for assign the mask spans all of C (GrB_assign), for row / column assign only that
// row / column.
//
// The three extract entry points have a second route: when the operand lives in HBM (or is large) they run the kernels of
// grb_extract.hip and the device write-back instead — see `extract_on_device` below.  The four container forms of assign have one too
// (grb_assign.hip, `assign_on_device`), and so has Kronecker (grb_kron.hip, `kron_on_device`): a product of two 8 000-entry matrices is
// 6.4e7 entries — one streaming store pass in HBM, out of reach for the map-based host route.
// The two diagonal entry points have one as well (grb_diag.hip, `diag_matrix_on_device` / `diag_vector_on_device`), and so have GxB_Matrix_sort / GxB_Vector_sort /
// GrBX_*_select_topk at the end of this file (grb_sort.hip, `sort_route`): no reference counterpart, the SuiteSparse 6.1 entry points.
#include "grb_opcommon.hpp"
#include "grb_extract.hpp"
#include "grb_assign.hpp"
#include "grb_kron.hpp"
#include "grb_diag.hpp"
#include "grb_matops.hpp"
#include "grb_tuples.hpp"
#include "grb_sort.hpp"
#include <algorithm>
#include <array>
#include <map>

// the typed apply entry points (grb_matrix_ops.cpp / grb_vector_ops.cpp) that the GxB_Scalar forms forward to
#define GRB_FOR_TYPES(X) X(BOOL, bool, T_BOOL) X(INT8, int8_t, T_INT8) X(UINT8, uint8_t, T_UINT8) X(INT16, int16_t, T_INT16) X(UINT16, uint16_t, T_UINT16) X(INT32, int32_t, T_INT32) \
  X(UINT32, uint32_t, T_UINT32) X(INT64, int64_t, T_INT64) X(UINT64, uint64_t, T_UINT64) X(FP32, float, T_FP32) X(FP64, double, T_FP64)
extern "C" {
#define GRB_DECL(SUF, CT, CODE) \
  GrB_Info GxB_Matrix_apply_BinaryOp1st_##SUF(GrB_Matrix, const GrB_Matrix, const GrB_BinaryOp, const GrB_BinaryOp, CT, const GrB_Matrix, const GrB_Descriptor); \
  GrB_Info GxB_Matrix_apply_BinaryOp2nd_##SUF(GrB_Matrix, const GrB_Matrix, const GrB_BinaryOp, const GrB_BinaryOp, const GrB_Matrix, CT, const GrB_Descriptor); \
  GrB_Info GxB_Vector_apply_BinaryOp1st_##SUF(GrB_Vector, const GrB_Vector, const GrB_BinaryOp, const GrB_BinaryOp, CT, const GrB_Vector, const GrB_Descriptor); \
  GrB_Info GxB_Vector_apply_BinaryOp2nd_##SUF(GrB_Vector, const GrB_Vector, const GrB_BinaryOp, const GrB_BinaryOp, const GrB_Vector, CT, const GrB_Descriptor);
GRB_FOR_TYPES(GRB_DECL)
#undef GRB_DECL
GrB_Info GrB_Matrix_eWiseAdd_BinaryOp(GrB_Matrix, const GrB_Matrix, const GrB_BinaryOp, const GrB_BinaryOp, const GrB_Matrix, const GrB_Matrix, const GrB_Descriptor);
GrB_Info GrB_Vector_eWiseAdd_BinaryOp(GrB_Vector, const GrB_Vector, const GrB_BinaryOp, const GrB_BinaryOp, const GrB_Vector, const GrB_Vector, const GrB_Descriptor);
}

using namespace grb;

namespace {

typedef std::array<uint8_t, 16> Val;
typedef std::map<std::pair<uint64_t, uint64_t>, Val> Map;     // (row, column) -> value bytes in some type

Map load(GrB_Matrix A, bool transpose) {
  mat_to_host(A); Map m; const size_t ts = A->type->size;
  for (size_t p = 0; p < A->hi.size(); p++) { Val v{}; memcpy(v.data(), &A->hx[p * ts], ts); m[transpose ? std::make_pair(A->hj[p], A->hi[p]) : std::make_pair(A->hi[p], A->hj[p])] = v; }
  return m;
}
Map load(GrB_Vector u) {
  vec_to_host(u); Map m; const size_t ts = u->type->size;
  for (size_t p = 0; p < u->hi.size(); p++) { Val v{}; memcpy(v.data(), &u->hx[p * ts], ts); m[{u->hi[p], 0}] = v; }
  return m;
}
void store(GrB_Matrix C, const Map& m) {
  const size_t ts = C->type->size;
  C->hi.clear(); C->hj.clear(); C->hx.clear(); C->pending.clear();
  for (auto& kv : m) { C->hi.push_back(kv.first.first); C->hj.push_back(kv.first.second); C->hx.insert(C->hx.end(), kv.second.data(), kv.second.data() + ts); }
  C->host_valid = true; mat_invalidate_device(C);
}
void store(GrB_Vector w, const Map& m) {
  const size_t ts = w->type->size;
  w->hi.clear(); w->hx.clear(); w->pending.clear();
  for (auto& kv : m) { w->hi.push_back(kv.first.first); w->hx.insert(w->hx.end(), kv.second.data(), kv.second.data() + ts); }
  w->host_valid = true; vec_invalidate_device(w);
}
Val cast(int dst, int src, const Val& v) { Val o{}; cast_scalar(dst, o.data(), src, v.data()); return o; }
bool truth(int code, const Val& v) { Val b = cast(T_BOOL, code, v); return b[0] != 0; }
Val combine(GrB_BinaryOp op, int ccode, const Val& c, int tcode, const Val& t) {          // accum(c, t) in the operator's domain, result in C's type
  const int ac = op->xtype->code; if (ac >= T_FC32) fail(GrB_DOMAIN_MISMATCH, "operators on complex values are out of scope");
  Val a = cast(ac, ccode, c), b = cast(ac, tcode, t), z{};
  dispatch_type(ac, [&]<class T>() { T x, y; memcpy(&x, a.data(), sizeof(T)); memcpy(&y, b.data(), sizeof(T)); T r = apply_binop<T>(op->opcode, x, y); memcpy(z.data(), &r, sizeof(T)); });
  return cast(ccode, op->ztype->code, z);
}
struct MaskView { const Map* m; int code; bool structural, comp, present;
  bool allows(const std::pair<uint64_t, uint64_t>& p) const {
    if (!present) return !comp;
    auto it = m->find(p); const bool t = it != m->end() && (structural || truth(code, it->second));
    return t != comp;
  } };

// C<M,replace> = accum(C, T) on maps.  `in_scope(p)`: positions the mask / replace step may touch (all of C, or one row / column)
template <class Scope> void write_back(Map& C, int ccode, const Map& T, int tcode, const MaskView& mk, bool replace, GrB_BinaryOp accum, Scope in_scope) {
  if (accum) check_binop(accum, "accum");
  Map Z;
  if (accum) {
    Z = C;
    for (auto& kv : T) { auto it = Z.find(kv.first); if (it == Z.end()) Z[kv.first] = cast(ccode, tcode, kv.second); else it->second = combine(accum, ccode, it->second, tcode, kv.second); }
  } else for (auto& kv : T) Z[kv.first] = cast(ccode, tcode, kv.second);
  Map out;
  for (auto& kv : C) { const bool scope = in_scope(kv.first); if (!scope || (!mk.allows(kv.first) && !replace)) out[kv.first] = kv.second; }   // what survives untouched
  for (auto& kv : Z) if (in_scope(kv.first) && mk.allows(kv.first)) out[kv.first] = kv.second;
  if (accum) { /* outside the scope Z == C: already kept */ }
  C.swap(out);
}
auto everywhere = [](const std::pair<uint64_t, uint64_t>&) { return true; };

std::vector<uint64_t> indices(const GrB_Index* I, GrB_Index ni, uint64_t dim, const char* what) { return expand_index_list(I, ni, dim, what); }
// an index list that is never materialised when it is GrB_ALL (the identity map): the default-dimension (2^60) hypersparse
// containers are sliced with it (`H[1]`, `H[:, 2]`), and a vector of `dim` indices cannot exist there
struct Sel {
  bool all = false; uint64_t dim = 0; std::vector<uint64_t> v;
  Sel(const GrB_Index* I, GrB_Index ni, uint64_t d, const char* what) : all(I == GrB_ALL), dim(d) { if (!all) v = expand_index_list(I, ni, d, what); }
  uint64_t size() const { return all ? dim : v.size(); }
  bool increasing() const { if (all) return true; for (size_t k = 1; k < v.size(); k++) if (v[k] <= v[k - 1]) return false; return true; }
  // position of source index x in an increasing list, or ~0
  uint64_t find_sorted(uint64_t x) const { if (all) return x < dim ? x : ~0ull; const auto a = std::lower_bound(v.begin(), v.end(), x); return (a == v.end() || *a != x) ? ~0ull : (uint64_t)(a - v.begin()); }
};
void check_m(GrB_Matrix A, const char* w) { if (!check_obj(A)) fail(GrB_UNINITIALIZED_OBJECT, std::string(w) + ": uninitialised matrix"); }
void check_v(GrB_Vector A, const char* w) { if (!check_obj(A)) fail(GrB_UNINITIALIZED_OBJECT, std::string(w) + ": uninitialised vector"); }

// ---- the common slices on the sorted tuples themselves (no map of the whole matrix): `M[i]`, `M[:, j]`, `M[i] = v`, `M[a:b, c:d]` ----
typedef std::vector<std::pair<uint64_t, Val>> Line;                     // (index, value bytes), sorted by index
Val val_at(const GrB_Matrix A, size_t p) { Val v{}; memcpy(v.data(), &A->hx[p * A->type->size], A->type->size); return v; }
std::pair<size_t, size_t> row_range(const GrB_Matrix A, uint64_t i) {
  const auto lo = std::lower_bound(A->hi.begin(), A->hi.end(), i), hi = std::upper_bound(lo, A->hi.end(), i);
  return {(size_t)(lo - A->hi.begin()), (size_t)(hi - A->hi.begin())};
}
// column j of op(A): a row of A is a contiguous run of its tuples, a column is picked out in one pass
Line line_of(GrB_Matrix A, bool transposed, uint64_t j) {
  mat_to_host(A); Line out;
  if (transposed) { const auto r = row_range(A, j); out.reserve(r.second - r.first); for (size_t p = r.first; p < r.second; p++) out.push_back({A->hj[p], val_at(A, p)}); }
  else for (size_t p = 0; p < A->hj.size(); p++) if (A->hj[p] == j) out.push_back({A->hi[p], val_at(A, p)});
  return out;
}
// row i (or column i) of C := `line` (values already in C's type)
void replace_line(GrB_Matrix C, bool is_row, uint64_t i, const Line& line) {
  const size_t ts = C->type->size;
  if (is_row) {
    const auto r = row_range(C, i);
    std::vector<GrB_Index> nj; std::vector<uint8_t> nx; nj.reserve(line.size()); nx.reserve(line.size() * ts);
    for (auto& e : line) { nj.push_back(e.first); nx.insert(nx.end(), e.second.data(), e.second.data() + ts); }
    C->hi.erase(C->hi.begin() + r.first, C->hi.begin() + r.second); C->hi.insert(C->hi.begin() + r.first, line.size(), i);
    C->hj.erase(C->hj.begin() + r.first, C->hj.begin() + r.second); C->hj.insert(C->hj.begin() + r.first, nj.begin(), nj.end());
    C->hx.erase(C->hx.begin() + r.first * ts, C->hx.begin() + r.second * ts); C->hx.insert(C->hx.begin() + r.first * ts, nx.begin(), nx.end());
  } else {
    const size_t n = C->hi.size();
    std::vector<GrB_Index> ni, nj; std::vector<uint8_t> nx; ni.reserve(n + line.size()); nj.reserve(n + line.size()); nx.reserve((n + line.size()) * ts);
    size_t q = 0;
    auto emit = [&](const std::pair<uint64_t, Val>& e) { ni.push_back(e.first); nj.push_back(i); nx.insert(nx.end(), e.second.data(), e.second.data() + ts); };
    for (size_t p = 0; p < n; p++) {
      while (q < line.size() && (line[q].first < C->hi[p] || (line[q].first == C->hi[p] && i < C->hj[p]))) emit(line[q++]);
      if (C->hj[p] == i) continue;                                      // the column's old entry
      ni.push_back(C->hi[p]); nj.push_back(C->hj[p]); nx.insert(nx.end(), &C->hx[p * ts], &C->hx[p * ts] + ts);
    }
    while (q < line.size()) emit(line[q++]);
    C->hi.swap(ni); C->hj.swap(nj); C->hx.swap(nx);
  }
  C->host_valid = true; mat_invalidate_device(C);
}
// the line C gets from `C(line) = accum(C(line), u)` over ALL positions, no mask: u's entries (cast), united with C's under accum
Line assigned_line(const Line& cur, int ccode, GrB_Vector u, GrB_BinaryOp accum) {
  if (accum) check_binop(accum, "accum");
  vec_to_host(u); const size_t us = u->type->size; const int ucode = u->type->code;
  Line out; out.reserve(cur.size() + u->hi.size());
  size_t a = 0, b = 0;
  auto uval = [&](size_t k) { Val v{}; memcpy(v.data(), &u->hx[k * us], us); return v; };
  while (a < cur.size() || b < u->hi.size()) {
    if (b >= u->hi.size() || (a < cur.size() && cur[a].first < u->hi[b])) { if (accum) out.push_back(cur[a]); a++; }          // C only: kept under accum, deleted without
    else if (a >= cur.size() || u->hi[b] < cur[a].first) { out.push_back({u->hi[b], cast(ccode, ucode, uval(b))}); b++; }
    else { out.push_back({u->hi[b], accum ? combine(accum, ccode, cur[a].second, ucode, uval(b)) : cast(ccode, ucode, uval(b))}); a++; b++; }
  }
  return out;
}
bool strictly_increasing(const std::vector<uint64_t>& v) { for (size_t k = 1; k < v.size(); k++) if (v[k] <= v[k - 1]) return false; return true; }

// ---- extract: which route ---------------------------------------------------------------------------------------------------------
// The device route (grb_extract.hip) is taken when a HIP device is present, every container of the call has an HBM layout (not hypersparse,
// not complex; the operand not a bitmap-only batch matrix) and the operand either lives in HBM only or holds at least
// EXTRACT_DEVICE_MIN_ENTRIES entries (the measured crossover against this file's host route, upload included: DESIGN.md §8).  Small
// host-resident containers — notebook slices — keep the host route.  GRB_MI355X_EXTRACT=0 forces the host route, =1 the device route
// wherever it is legal; GRB_MI355X_EXTRACT_BISECT=1 makes a column list bisect instead of using its table (both read per call: test hooks).
constexpr uint64_t EXTRACT_DEVICE_MIN_ENTRIES = 10000;
int route_env(const char* name) { const char* e = getenv(name); return (e && *e) ? (atoi(e) != 0 ? 1 : 0) : -1; }      // a route's test hook: 0 host, 1 device, -1 not set
bool extract_bisect_env() { const char* e = getenv("GRB_MI355X_EXTRACT_BISECT"); return e && atoi(e) != 0; }
bool dev_capable(GrB_Matrix A) { return !A || (!is_hyper(A) && A->type->code < T_FC32 && !A->iso_full); }
bool dev_capable(GrB_Vector v) { return !v || (!is_hyper(v) && v->type->code < T_FC32 && !v->iso_full); }
// `list_in_hbm`: an index list of the call lies in HBM (IdxArg) — the device route wherever it is legal, whatever the entry counts: the list is not downloaded to pick a route
bool extract_on_device(GrB_Matrix A, bool others_capable, bool list_in_hbm) {
  const int env = route_env("GRB_MI355X_EXTRACT");
  if (env == 0 || !device_ok() || !others_capable || !dev_capable(A) || mat_bitmap_only(A)) return false;
  if (env == 1 || list_in_hbm) return true;
  if (A->dev_valid && !A->host_valid) return true;                      // it lives in HBM: it is not downloaded for this
  return A->host_valid && mat_nvals(A) >= EXTRACT_DEVICE_MIN_ENTRIES;   // (the count of a valid host mirror: no device work)
}
bool extract_on_device(GrB_Vector u, bool others_capable, bool list_in_hbm) {
  const int env = route_env("GRB_MI355X_EXTRACT");
  if (env == 0 || !device_ok() || !others_capable || !dev_capable(u)) return false;
  if (env == 1 || list_in_hbm) return true;
  vec_gate(u);                                                          // deferred work that involves u is completed first, as every reader does
  if (u->dev_valid && !u->host_valid) return true;
  return u->host_valid && vec_nvals(u) >= EXTRACT_DEVICE_MIN_ENTRIES;
}
const char* kind_name(const ExIdx& x) { return x.kind == EX_ALL ? "all" : x.kind == EX_LIST ? (x.hbm ? "list@hbm" : "list") : "range"; }
// the plan's word for a list that was parsed in HBM (grb_index.hip); nothing for every other index argument, so that host-list calls keep their strings
std::string parse_name(const ExIdx& x) { return (x.hbm && x.n) ? std::string("k_index_parse<increasing=") + (x.increasing ? "1" : "0") + "> " : std::string(); }
// The host route of a call whose list lies in HBM: the list is copied down once, and the route's own parse reports what it always reports.
struct HostList {
  std::vector<GrB_Index> v;
  const GrB_Index* get(const IdxArg& a) {
    if (!a.in_hbm() || !a.I) return a.I;
    need_device(); v.resize(a.n ? a.n : 1);
    if (a.n) { GRB_HIP(hipMemcpyAsync(v.data(), a.I, a.n * 8, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream())); }
    return v.data();
  }
};

// The prelude of the two vector-valued extracts (vector_prelude with the index argument parsed first and the accumulator checked before the mask is touched):
// `idx` over `dim` positions, the checks in the host route's order, the mask as `allow`.  True: nothing may be written — w has been cleared under replace, and
// the caller returns.
bool extract_vector_prelude(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, const IdxArg& ia, uint64_t dim, const DescView& dv, ExIdx& idx, DevBuf& allow_buf, const uint8_t*& allow) {
  extract_parse(idx, ia, dim, "extract");
  if (w->n != idx.n || (mask && mask->n != w->n)) fail(GrB_DIMENSION_MISMATCH, "extract: output size must equal the number of indices");
  if (accum) check_binop(accum, "accum");
  bool nothing = false;
  allow = vector_allow(mask, dv, w->n, allow_buf, &nothing);
  if (nothing && dv.replace) GrB_Vector_clear(w);
  return nothing;
}

void extract_vector_device(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Vector u, const IdxArg& ia, const DescView& dv) {
  ExIdx idx; DevBuf allow_buf; const uint8_t* allow;
  if (extract_vector_prelude(w, mask, accum, ia, u->n, dv, idx, allow_buf, allow)) return;
  vec_to_device(u);
  const uint64_t n = idx.n; const size_t ts = u->type->size;
  DevBuf keep, tval(n * ts + 8), tpres(n + 1);
  extract_upload(idx, keep);
  extract_vector(ts, u->dval.p, u->dpres.as<uint8_t>(), idx, tval.p, tpres.as<uint8_t>());
  if (keep.p) GRB_HIP(hipStreamSynchronize(stream()));                  // (the uploaded list returns to the pool)
  g_last_plan = std::string("extract_vector<index=") + kind_name(idx) + "> " + parse_name(idx) + "k_extract_vector ";
  vector_write_back(w, u->type->code, tval, tpres, allow, accum, dv.replace, false);
}

void extract_col_device(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Matrix A, const IdxArg& ia, GrB_Index j, const DescView& dv, uint64_t ar) {
  ExIdx idx; DevBuf allow_buf; const uint8_t* allow;
  if (extract_vector_prelude(w, mask, accum, ia, ar, dv, idx, allow_buf, allow)) return;
  mat_to_device(A);
  const uint64_t n = idx.n; const size_t ts = A->type->size;
  DevBuf keep, tval(n * ts + 8), tpres(n + 1);
  extract_upload(idx, keep);
  extract_line(A->csr, ts, dv.tran0, (uint32_t)j, idx, tval.p, tpres.as<uint8_t>());
  if (keep.p) GRB_HIP(hipStreamSynchronize(stream()));
  const bool scatter = dv.tran0 && idx.kind == EX_ALL;
  g_last_plan = std::string("extract_col<") + (dv.tran0 ? "row of the CSR" : "column of the CSR") + ",index=" + kind_name(idx) + "> " +
                parse_name(idx) + (scatter ? "k_extract_row_scatter " : "k_extract_lookup ");
  vector_write_back(w, A->type->code, tval, tpres, allow, accum, dv.replace, false);
}

void extract_matrix_device(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const DescView& dv, uint64_t ar, uint64_t ac) {
  ExIdx ri, ci; extract_parse(ri, ia, ar, "extract"); extract_parse(ci, ja, ac, "extract");
  if (C->nrows != ri.n || C->ncols != ci.n || (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols))) fail(GrB_DIMENSION_MISMATCH, "extract: output shape must be |I| x |J|");
  if (accum) check_binop(accum, "accum");
  if (!Mask && dv.mask_comp) { if (dv.replace) GrB_Matrix_clear(C); return; }      // no mask + complement: nothing may be written
  mat_to_device(A);
  const size_t ts = A->type->size;
  DevBuf keep_i, keep_j; extract_upload(ri, keep_i); extract_upload(ci, keep_j);
  // op(A)(I, J) = (A(J, I))^T under GrB_DESC_T0: the (smaller) result is transposed, never A
  ExtractPlan plan; DevCSR T, Tt;
  extract_csr(A->csr, ts, dv.tran0 ? ci : ri, dv.tran0 ? ri : ci, extract_bisect_env(), T, plan);
  if (dv.tran0) { csr_transpose(T, ts, Tt); T.clear(); }
  g_last_plan = std::string("extract_matrix<cols=") + plan.cols + ",rowsort=" + (plan.rowsort ? "1" : "0") + ",transpose=" + (dv.tran0 ? "1" : "0") + (ri.hbm ? ",rows=list@hbm" : "") + (ci.hbm ? ",columns=list@hbm" : "") + "> " +
                parse_name(ri) + parse_name(ci) + "k_extract_rows<count> k_extract_rows<fill> ";
  matrix_write_back(C, dv.tran0 ? Tt : T, A->type->code, Mask, dv, accum, false);
}

}  // namespace

// The seven index-list operations, each once for both kinds of list: GrB_<name> passes a host list (or GrB_ALL, or a range triple), GrBX_<name>_at with
// location 1 and the GrBX_*_Vector entry points pass a list that lies in HBM (IdxArg).
static GrB_Info vector_extract_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, const GrB_Descriptor desc) {
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] {
    check_v(u, "extract"); if (mask) check_v(mask, "extract");
    const DescView dv(desc);
    if (extract_on_device(u, dev_capable(w) && dev_capable(mask), ia.in_hbm())) { extract_vector_device(w, mask, accum, u, ia, dv); return; }
    HostList hl; const GrB_Index* I = hl.get(ia); const GrB_Index ni = ia.n;
    const Sel idx(I, ni, u->n, "extract");
    if (w->n != idx.size() || (mask && mask->n != w->n)) fail(GrB_DIMENSION_MISMATCH, "extract: output size must equal the number of indices");
    Map U = load(u), T, C = load(w), Mm; if (mask) Mm = load(mask);
    if (idx.all) T = U;
    else for (size_t k = 0; k < idx.v.size(); k++) { auto it = U.find({idx.v[k], 0}); if (it != U.end()) T[{k, 0}] = it->second; }
    write_back(C, w->type->code, T, u->type->code, MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}, dv.replace, accum, everywhere);
    store(w, C);
  });
}

static GrB_Info col_extract_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, GrB_Index j, const GrB_Descriptor desc) {
  if (!w || !A) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] {
    check_m(A, "extract"); if (mask) check_v(mask, "extract");
    const DescView dv(desc);
    const uint64_t ar = dv.tran0 ? A->ncols : A->nrows, ac = dv.tran0 ? A->nrows : A->ncols;
    if (j >= ac) fail(GrB_INVALID_INDEX, "extract: column index out of range");
    if (extract_on_device(A, dev_capable(w) && dev_capable(mask), ia.in_hbm())) { extract_col_device(w, mask, accum, A, ia, j, dv, ar); return; }
    HostList hl; const GrB_Index* I = hl.get(ia); const GrB_Index ni = ia.n;
    const Sel idx(I, ni, ar, "extract");
    if (w->n != idx.size() || (mask && mask->n != w->n)) fail(GrB_DIMENSION_MISMATCH, "extract: output size must equal the number of indices");
    const Line col = line_of(A, dv.tran0, j);                             // (index in op(A)'s column j, value), sorted
    Map T, C = load(w), Mm; if (mask) Mm = load(mask);
    if (idx.all) for (auto& e : col) T[{e.first, 0}] = e.second;
    else for (size_t k = 0; k < idx.v.size(); k++) {
      auto it = std::lower_bound(col.begin(), col.end(), idx.v[k], [](const std::pair<uint64_t, Val>& e, uint64_t x) { return e.first < x; });
      if (it != col.end() && it->first == idx.v[k]) T[{k, 0}] = it->second;
    }
    write_back(C, w->type->code, T, A->type->code, MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}, dv.replace, accum, everywhere);
    store(w, C);
  });
}

static GrB_Info matrix_extract_any(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const GrB_Descriptor desc) {
  if (!C || !A) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_m(A, "extract"); if (Mask) check_m(Mask, "extract");
    const DescView dv(desc);
    const uint64_t ar = dv.tran0 ? A->ncols : A->nrows, ac = dv.tran0 ? A->nrows : A->ncols;
    if (extract_on_device(A, dev_capable(C) && dev_capable(Mask), ia.in_hbm() || ja.in_hbm())) { extract_matrix_device(C, Mask, accum, A, ia, ja, dv, ar, ac); return; }
    HostList hli, hlj; const GrB_Index* I = hli.get(ia); const GrB_Index* J = hlj.get(ja); const GrB_Index ni = ia.n, nj = ja.n;
    const Sel ri(I, ni, ar, "extract"), ci(J, nj, ac, "extract");
    if (C->nrows != ri.size() || C->ncols != ci.size() || (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols))) fail(GrB_DIMENSION_MISMATCH, "extract: output shape must be |I| x |J|");
    if (!Mask && !dv.mask_comp && !accum && ri.increasing() && ci.increasing()) {       // a slice `A[a:b, c:d]` into a fresh output: one pass over A's tuples
      mat_to_host(A); const size_t ts = A->type->size; const int acode = A->type->code, ccode = C->type->code;
      struct E { uint64_t i, j; Val v; }; std::vector<E> out;
      for (size_t p = 0; p < A->hi.size(); p++) {
        const uint64_t si = dv.tran0 ? A->hj[p] : A->hi[p], sj = dv.tran0 ? A->hi[p] : A->hj[p];
        const uint64_t a = ri.find_sorted(si); if (a == ~0ull) continue;
        const uint64_t b = ci.find_sorted(sj); if (b == ~0ull) continue;
        Val v{}; memcpy(v.data(), &A->hx[p * ts], ts);
        out.push_back({a, b, cast(ccode, acode, v)});
      }
      if (dv.tran0) std::sort(out.begin(), out.end(), [](const E& x, const E& y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
      const size_t cs = C->type->size;
      C->hi.clear(); C->hj.clear(); C->hx.clear(); C->pending.clear(); C->iso_full = false;
      C->hi.reserve(out.size()); C->hj.reserve(out.size()); C->hx.reserve(out.size() * cs);
      for (auto& e : out) { C->hi.push_back(e.i); C->hj.push_back(e.j); C->hx.insert(C->hx.end(), e.v.data(), e.v.data() + cs); }
      C->host_valid = true; mat_invalidate_device(C);
      return;
    }
    Map Am = load(A, dv.tran0), T, Cm = load(C, false), Mm; if (Mask) Mm = load(Mask, false);
    std::multimap<uint64_t, uint64_t> rpos, cpos;                       // source index -> output positions (an index may repeat; GrB_ALL is the identity and is not listed)
    if (!ri.all) for (size_t k = 0; k < ri.v.size(); k++) rpos.insert({ri.v[k], k});
    if (!ci.all) for (size_t k = 0; k < ci.v.size(); k++) cpos.insert({ci.v[k], k});
    for (auto& kv : Am) {
      std::vector<uint64_t> ra, ca;
      if (ri.all) ra.push_back(kv.first.first); else { auto rr = rpos.equal_range(kv.first.first); for (auto a = rr.first; a != rr.second; ++a) ra.push_back(a->second); }
      if (ci.all) ca.push_back(kv.first.second); else { auto cc = cpos.equal_range(kv.first.second); for (auto b = cc.first; b != cc.second; ++b) ca.push_back(b->second); }
      for (uint64_t a : ra) for (uint64_t b : ca) T[{a, b}] = kv.second;
    }
    write_back(Cm, C->type->code, T, A->type->code, MaskView{&Mm, Mask ? Mask->type->code : 0, dv.mask_struct, dv.mask_comp, Mask != nullptr}, dv.replace, accum, everywhere);
    store(C, Cm);
  });
}

// ---- assign: C(I,J)<M> = accum(C(I,J), A) --------------------------------------------------------------------------------------
namespace {
// the region update: positions of the index grid take A's entry (or lose theirs), combined with accum when given
void region_update(Map& C, int ccode, const Map& A, int acode, const std::vector<uint64_t>& ri, const std::vector<uint64_t>& ci, GrB_BinaryOp accum, const MaskView& mk, bool replace,
                   bool whole_mask /* GrB_assign: mask and replace span all of C */, bool row_scope, bool col_scope, uint64_t fixed) {
  if (accum) check_binop(accum, "accum");
  Map out;
  auto in_region = [&](const std::pair<uint64_t, uint64_t>&) { return false; };   (void)in_region;
  // new values over the region
  std::map<std::pair<uint64_t, uint64_t>, std::pair<bool, Val>> upd;               // position -> (has value, value in C's type)
  for (size_t a = 0; a < ri.size(); a++) for (size_t b = 0; b < ci.size(); b++) {
    const std::pair<uint64_t, uint64_t> p{ri[a], ci[b]};
    auto ia = A.find({a, b}); auto ic = C.find(p);
    if (accum) {
      if (ia != A.end() && ic != C.end()) upd[p] = {true, combine(accum, ccode, ic->second, acode, ia->second)};
      else if (ia != A.end()) upd[p] = {true, cast(ccode, acode, ia->second)};
      else if (ic != C.end()) upd[p] = {true, ic->second};
      else upd[p] = {false, Val{}};
    } else upd[p] = ia != A.end() ? std::make_pair(true, cast(ccode, acode, ia->second)) : std::make_pair(false, Val{});
  }
  auto in_scope = [&](const std::pair<uint64_t, uint64_t>& p) { return whole_mask || (row_scope && p.first == fixed) || (col_scope && p.second == fixed); };
  auto mkey = [&](const std::pair<uint64_t, uint64_t>& p) { return row_scope ? std::make_pair(p.second, (uint64_t)0) : (col_scope ? std::make_pair(p.first, (uint64_t)0) : p); };
  for (auto& kv : C) {
    const bool touched = upd.count(kv.first) != 0;
    const bool allowed = mk.allows(mkey(kv.first));
    if (touched && allowed) continue;                                    // replaced below
    if (!allowed && replace && in_scope(kv.first)) continue;             // deleted by replace
    out[kv.first] = kv.second;
  }
  for (auto& kv : upd) if (kv.second.first && mk.allows(mkey(kv.first))) out[kv.first] = kv.second.second;
  C.swap(out);
}

// ---- assign: which route ----------------------------------------------------------------------------------------------------------
// The device route (grb_assign.hip) is taken when a HIP device is present, every container of the call has an HBM layout (dev_capable; none a
// bitmap-only batch matrix), the operand is not the output, a mask object accompanies a complemented mask, and C either lives in HBM only or C or
// the operand holds at least N entries, N measured per entry point against this file's host route, upload included.
// Small host-resident containers — notebook slices — keep the host route.  GRB_MI355X_ASSIGN=0 forces the host route, =1 the device route wherever it
// is legal (read per call: a test hook).  A list that names an index twice is found on the device and handed back to the host route (which takes the
// last occurrence): the `*_device` functions return false for it, before anything was written.
constexpr uint64_t ASSIGN_DEVICE_MIN_ENTRIES = 30000;            // GrB_Matrix_assign
constexpr uint64_t ASSIGN_ROW_DEVICE_MIN_ENTRIES = 3000000;      // GrB_Row_assign: the host replaces the row's run of tuples in place, cheap up to ~1e6 entries
constexpr uint64_t ASSIGN_COL_DEVICE_MIN_ENTRIES = 100000;       // GrB_Col_assign: the host's one merge pass
constexpr uint64_t ASSIGN_VEC_DEVICE_MIN_ENTRIES = 500;          // GrB_Vector_assign: the host route is map-based for every shape (the smallest size measured; the device route won all)
uint64_t entries_known(GrB_Vector u) { return u->host_valid ? vec_nvals(u) : (u->facts.dnvals_known ? u->facts.dnvals : 0); }      // (no device work for a count)
// `operand_entries`: asked only after the variable, the device and the residency of C have not decided
// `list_in_hbm`: as for extract — the device route wherever it is legal
template <class F> bool assign_on_device(GrB_Matrix C, bool others_capable, uint64_t min_entries, F&& operand_entries, bool list_in_hbm) {
  const int env = route_env("GRB_MI355X_ASSIGN");
  if (env == 0 || !device_ok() || !others_capable || !dev_capable(C) || mat_bitmap_only(C)) return false;
  if (env == 1 || list_in_hbm) return true;
  if (C->dev_valid && !C->host_valid) return true;                      // it lives in HBM: it is not downloaded for this
  return mat_nvals(C) >= min_entries || operand_entries() >= min_entries;
}
template <class F> bool assign_on_device(GrB_Vector w, bool others_capable, uint64_t min_entries, F&& operand_entries, bool list_in_hbm) {
  const int env = route_env("GRB_MI355X_ASSIGN");
  if (env == 0 || !device_ok() || !others_capable || !dev_capable(w)) return false;
  if (env == 1 || list_in_hbm) return true;
  if (w->dev_valid && !w->host_valid) return true;
  return entries_known(w) >= min_entries || operand_entries() >= min_entries;
}
bool mat_capable(GrB_Matrix A) { return dev_capable(A) && !(A && mat_bitmap_only(A)); }
const char* accum_name(GrB_BinaryOp accum) { return accum ? accum->name : "none"; }

// C(I, J) := T (T in C's coordinates, nothing outside I x J), then C<M, replace> = that: Z = (C without its entries inside I x J) u T, written back
// without an accumulator.  csr_compact and csr_ewise(SECOND) of the tree; the two patterns are disjoint.
void region_replace(GrB_Matrix C, GrB_Matrix Mask, const DescView& dv, DevCSR& T, int tcode, const ExIdx& ri, const DevBuf& inv_i, const ExIdx& ci, const DevBuf& inv_j) {
  const int ccode = C->type->code; const size_t cs = C->type->size;
  if (!C->csr.nnz) { matrix_write_back(C, T, tcode, Mask, dv, nullptr, false); return; }
  DevBuf keep(C->csr.nnz + 1); DevCSR Rest;
  assign_region_keep(C->csr, ri, inv_i, ci, inv_j, keep.as<uint8_t>());
  csr_compact(C->csr, C->csr.val.p, cs, keep.as<uint8_t>(), Rest);
  if (!Rest.nnz) { matrix_write_back(C, T, tcode, Mask, dv, nullptr, false); return; }
  if (!T.nnz) { matrix_write_back(C, Rest, ccode, Mask, dv, nullptr, false); return; }
  DevBuf tc; const void* tv = cast_values(ccode, tcode, T.val.p, T.nnz, tc);
  DevCSR Z; csr_ewise(ccode, Rest, Rest.val.p, T, tv, B_SECOND, true, Z);
  matrix_write_back(C, Z, ccode, Mask, dv, nullptr, false);
}

bool assign_matrix_device(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const DescView& dv) {
  ExIdx ri, ci; extract_parse(ri, ia, C->nrows, "assign"); extract_parse(ci, ja, C->ncols, "assign");
  const uint64_t ar = dv.tran0 ? A->ncols : A->nrows, ac = dv.tran0 ? A->nrows : A->ncols;
  if (ar != ri.n || ac != ci.n || (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols))) fail(GrB_DIMENSION_MISMATCH, "assign: the matrix must be |I| x |J|");
  if (accum) check_binop(accum, "accum");
  DevBuf keep_i, keep_j, inv_i, inv_j; extract_upload(ri, keep_i); extract_upload(ci, keep_j);
  if (!assign_inverse(ri, C->nrows, inv_i) || !assign_inverse(ci, C->ncols, inv_j)) return false;
  mat_to_device(C); mat_to_device(A);
  // op(A) under GrB_DESC_T0: the operand (the smaller side) is transposed, never C
  const DevCSR& Ad = dv.tran0 ? mat_csc(A) : A->csr;
  DevCSR T; AssignPlan plan;
  assign_relocate(Ad, A->type->size, ri, ci, (uint32_t)C->nrows, (uint32_t)C->ncols, T, plan);
  g_last_plan = std::string("assign_matrix<rows=") + kind_name(ri) + ",cols=" + kind_name(ci) + ",rowsort=" + (plan.rowsort ? "1" : "0") + ",transpose=" + (dv.tran0 ? "1" : "0") + ",accum=" + accum_name(accum) +
                "> " + parse_name(ri) + parse_name(ci) + "k_assign_rowlen k_assign_move " + (accum ? "" : "k_assign_region_keep ");
  if (accum) matrix_write_back(C, T, A->type->code, Mask, dv, accum, false);      // accum(C, T) on the union of the patterns: entries of C inside the region that A lacks are kept
  else region_replace(C, Mask, dv, T, A->type->code, ri, inv_i, ci, inv_j);
  return true;
}

// line<allow, replace>(I) = accum(line(I), u) on a bitmap of type `lcode`, in place: u's values go through the accumulator's domain as the host's `combine` does
void line_assign(int lcode, uint64_t n, void* lval, uint8_t* lpres, const uint8_t* allow, const ExIdx& idx, const DevBuf& inv, GrB_Vector u, GrB_BinaryOp accum, bool replace) {
  const int ecode = accum ? accum->xtype->code : lcode;
  DevBuf uc, lc;
  const void* uv = cast_values(ecode, u->type->code, u->dval.p, u->n, uc);
  if (ecode == lcode) { assign_vector(lcode, n, lval, lpres, allow, idx, inv, uv, u->dpres.as<uint8_t>(), accum ? accum->opcode : -1, replace); }
  else {
    lc.alloc(n * type_size(ecode) + 1);
    vec_cast_values(ecode, lc.p, lcode, lval, n);
    assign_vector(ecode, n, lc.p, lpres, allow, idx, inv, uv, u->dpres.as<uint8_t>(), accum->opcode, replace);
    assign_cast_touched(lcode, lval, ecode, lc.p, n, allow, idx, inv, u->dpres.as<uint8_t>());      // only what the assign wrote comes back: every other value of the line keeps its bits
  }
  GRB_HIP(hipStreamSynchronize(stream()));                              // (the cast copies return to the pool)
}

bool assign_vector_device(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Vector u, const IdxArg& ia, const DescView& dv) {
  ExIdx idx; extract_parse(idx, ia, w->n, "assign");
  if (u->n != idx.n || (mask && mask->n != w->n)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of indices");
  if (accum) check_binop(accum, "accum");
  DevBuf keep, inv; extract_upload(idx, keep);
  if (!assign_inverse(idx, w->n, inv)) return false;
  DevBuf allow_buf; bool nothing = false;
  const uint8_t* allow = vector_allow(mask, dv, w->n, allow_buf, &nothing);
  vec_to_device(u); vec_to_device(w);
  line_assign(w->type->code, w->n, w->dval.p, w->dpres.as<uint8_t>(), allow, idx, inv, u, accum, dv.replace);
  vec_invalidate_host(w);
  g_last_plan = std::string("assign_vector<index=") + kind_name(idx) + ",accum=" + accum_name(accum) + "> " + parse_name(idx) + "k_assign_vector ";
  return true;
}

// C(i, J) = u (`is_row`) or C(I, j) = u: the line of C as a bitmap, the vector kernel on it under the vector mask, then the line put back as a region of C
bool assign_line_device(GrB_Matrix C, GrB_Vector mask, GrB_BinaryOp accum, GrB_Vector u, bool is_row, uint64_t fixed, const IdxArg& la, const DescView& dv) {
  const uint64_t len = is_row ? C->ncols : C->nrows;
  const char* const msg = is_row ? "assign: the vector's size must equal the number of column indices" : "assign: the vector's size must equal the number of row indices";
  ExIdx idx; extract_parse(idx, la, len, "assign");
  if (u->n != idx.n || (mask && mask->n != len)) fail(GrB_DIMENSION_MISMATCH, msg);
  if (accum) check_binop(accum, "accum");
  if (!len) return false;
  DevBuf keep, inv; extract_upload(idx, keep);
  if (!assign_inverse(idx, len, inv)) return false;
  DevBuf allow_buf; bool nothing = false;
  const uint8_t* allow = vector_allow(mask, dv, len, allow_buf, &nothing);
  mat_to_device(C); vec_to_device(u);
  const int ccode = C->type->code; const size_t cs = C->type->size;
  ExIdx all; all.kind = EX_ALL; all.n = len;
  DevBuf lval(len * cs + 8), lpres(len + 1);
  extract_line(C->csr, cs, is_row, (uint32_t)fixed, all, lval.p, lpres.as<uint8_t>());
  line_assign(ccode, len, lval.p, lpres.as<uint8_t>(), allow, idx, inv, u, accum, dv.replace);
  DevCSR Tl, T; AssignPlan plan;
  assign_line_to_csr(cs, len, lval.p, lpres.as<uint8_t>(), is_row, Tl);
  ExIdx one; one.kind = EX_RANGE; one.lo = (uint32_t)fixed; one.step = 1; one.n = 1;
  const ExIdx& ri = is_row ? one : all; const ExIdx& ci = is_row ? all : one;
  assign_relocate(Tl, cs, ri, ci, (uint32_t)C->nrows, (uint32_t)C->ncols, T, plan);
  g_last_plan = std::string(is_row ? "assign_row<index=" : "assign_col<index=") + kind_name(idx) + ",accum=" + accum_name(accum) + "> " + parse_name(idx) + (is_row ? "k_extract_row_scatter" : "k_extract_lookup") +
                " k_assign_vector k_scatter_present k_assign_move k_assign_region_keep ";
  const DevBuf none_i, none_j;
  region_replace(C, nullptr, DescView(nullptr), T, ccode, ri, none_i, ci, none_j);
  return true;
}

// ---- kronecker: which route -------------------------------------------------------------------------------------------------------
// The device route (grb_kron.hip) is taken when a HIP device is present, C, both operands and the mask have an HBM layout (mat_capable), neither
// operand is the output, a mask object accompanies a complemented mask, the product fits the 32-bit device layout (ar br and ac bc follow from C's
// own shape; nnz(A) nnz(B) <= KRON_MAX_ENTRIES) and either C or an operand lives in HBM only (it is not downloaded for this) or the product has at
// least KRON_DEVICE_MIN_ENTRIES entries (the crossover against this file's host route, upload included: DESIGN.md §8).  The 3 x 3 docstring
// examples keep the host route.  GRB_MI355X_KRON=0 forces the host route, =1 the device route wherever it is legal (read per call: a test hook).
// GRB_MI355X_KRON_TIME=1 puts HIP events around the fill kernel; GrBX_kron_fill_ms returns what they measured (tools/kron_probe.py).
constexpr uint64_t KRON_DEVICE_MIN_ENTRIES = 1000;              // provisional: reasoned from the assign route's fixed cost, not yet measured
thread_local float g_kron_fill_ms = 0.0f;
bool hbm_only(GrB_Matrix A) { return A->dev_valid && !A->host_valid; }
// (the count of a valid host mirror, or of the device CSR: no device work.  With element edits queued on an HBM-only matrix — grb_container.cpp — the CSR header is read
//  WITHOUT a flush here and in the threshold lambda of GrB_Matrix_assign below: the count is off by at most the queue's length, and it only picks a route.)
uint64_t entries_of(GrB_Matrix A) { return A->host_valid ? mat_nvals(A) : (uint64_t)A->csr.nnz; }
bool kron_on_device(GrB_Matrix C, GrB_Matrix Mask, GrB_Matrix A, GrB_Matrix B, const DescView& dv) {
  const int env = route_env("GRB_MI355X_KRON");
  if (env == 0 || !device_ok() || !mat_capable(C) || !mat_capable(A) || !mat_capable(B) || !mat_capable(Mask)) return false;
  if (A == C || B == C || (!Mask && dv.mask_comp)) return false;
  if (C->nrows > GRB_DIM_DEVICE_MAX || C->ncols > GRB_DIM_DEVICE_MAX) return false;
  const uint64_t na = entries_of(A), nb = entries_of(B);
  if (na > KRON_MAX_ENTRIES || nb > KRON_MAX_ENTRIES || na * nb > KRON_MAX_ENTRIES) return false;      // (each factor < 2^32: the product cannot wrap)
  if (env == 1) return true;
  if (hbm_only(C) || hbm_only(A) || hbm_only(B)) return true;
  return na * nb >= KRON_DEVICE_MIN_ENTRIES;
}
void kron_device(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, GrB_BinaryOp op, GrB_Matrix A, GrB_Matrix B, const DescView& dv) {
  if (accum) check_binop(accum, "accum");
  mat_to_device(A); mat_to_device(B);
  // op(A) / op(B) under GrB_DESC_T0 / T1: the cached transposes of the (small) operands, never a transposed T
  const DevCSR& Ad = dv.tran0 ? mat_csc(A) : A->csr; const DevCSR& Bd = dv.tran1 ? mat_csc(B) : B->csr;
  const int oc = op->xtype->code;                                       // T's type is the operator's domain, comparisons included, as on the host route
  DevBuf acast, bcast;
  const void* av = binop_uses_x(op->opcode) ? cast_values(oc, A->type->code, Ad.val.p, Ad.nnz, acast) : nullptr;
  const void* bv = binop_uses_y(op->opcode) ? cast_values(oc, B->type->code, Bd.val.p, Bd.nnz, bcast) : nullptr;
  const char* te = getenv("GRB_MI355X_KRON_TIME"); const bool timed = te && atoi(te) != 0;
  DevCSR T;
  kron_csr(oc, op->opcode, Ad, av, Bd, bv, T, timed ? &g_kron_fill_ms : nullptr);
  g_last_plan = std::string("kronecker<op=") + op->name + ",transpose0=" + (dv.tran0 ? "1" : "0") + ",transpose1=" + (dv.tran1 ? "1" : "0") + ",accum=" + accum_name(accum) + "> k_kron_rowptr k_kron_fill ";
  matrix_write_back(C, T, oc, Mask, dv, accum, false);
}
}  // namespace
// the whole-container fast paths forward to eWiseAdd without the caller's descriptor: only when it asks for nothing they would
// drop (a complemented mask without a mask object allows no writes at all; an invalid descriptor is the general path's error)
static inline bool plain_desc(GrB_Descriptor d) { return !d || (check_obj(d) && (d->mask & GrB_COMP) == 0); }

static GrB_Info vector_assign_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, const GrB_Descriptor desc) {
  const GrB_Index* const I = ia.I;
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  if (I == GrB_ALL && !mask && plain_desc(desc) && accum && check_obj(u) && device_ok() && u->n == w->n) return GrB_Vector_eWiseAdd_BinaryOp(w, nullptr, nullptr, accum, w, u, nullptr);   // w = accum(w, u), in HBM
  return guarded(w, [&] {
    check_v(u, "assign"); if (mask) check_v(mask, "assign");
    const DescView dv(desc);
    vec_gate(w); vec_gate(u);                                            // deferred work that involves them is completed first, as every reader does
    if (u != w && (mask || !dv.mask_comp) && assign_on_device(w, dev_capable(u) && dev_capable(mask), ASSIGN_VEC_DEVICE_MIN_ENTRIES, [&] { return entries_known(u); }, ia.in_hbm()) && assign_vector_device(w, mask, accum, u, ia, dv)) return;
    HostList hl; const auto idx = indices(hl.get(ia), ia.n, w->n, "assign");
    if (u->n != idx.size() || (mask && mask->n != w->n)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of indices");
    Map C = load(w), U = load(u), Mm; if (mask) Mm = load(mask);
    region_update(C, w->type->code, U, u->type->code, idx, std::vector<uint64_t>{0}, accum, MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}, dv.replace,
                  true, false, false, 0);
    store(w, C);
  });
}

static GrB_Info matrix_assign_any(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const GrB_Descriptor desc) {
  const GrB_Index* const I = ia.I; const GrB_Index* const J = ja.I;
  if (!C || !A) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  // the whole container, no mask, with an accumulator (`paths.assign_matrix(frontier, accum=PLUS)`, gap/bcmark.py:41): that is
  // C = accum(C, A) on the union of the patterns — the eWiseAdd kernel, in HBM (a dense ns x n `paths` must not visit the host)
  if (I == GrB_ALL && J == GrB_ALL && !Mask && plain_desc(desc) && accum && check_obj(A) && device_ok()) {      // (a complemented mask without a mask object allows nothing: not this path)
    const DescView dv0(desc);
    if (!dv0.tran0 && A->nrows == C->nrows && A->ncols == C->ncols) return GrB_Matrix_eWiseAdd_BinaryOp(C, nullptr, nullptr, accum, C, A, nullptr);
  }
  return guarded(C, [&] {
    check_m(A, "assign"); if (Mask) check_m(Mask, "assign");
    const DescView dv(desc);
    if (A != C && (Mask || !dv.mask_comp) && assign_on_device(C, mat_capable(A) && mat_capable(Mask), ASSIGN_DEVICE_MIN_ENTRIES, [&] { return A->host_valid ? mat_nvals(A) : (uint64_t)A->csr.nnz; }, ia.in_hbm() || ja.in_hbm()) && assign_matrix_device(C, Mask, accum, A, ia, ja, dv)) return;
    HostList hli, hlj; const auto ri = indices(hli.get(ia), ia.n, C->nrows, "assign"), ci = indices(hlj.get(ja), ja.n, C->ncols, "assign");
    const uint64_t ar = dv.tran0 ? A->ncols : A->nrows, ac = dv.tran0 ? A->nrows : A->ncols;
    if (ar != ri.size() || ac != ci.size() || (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols))) fail(GrB_DIMENSION_MISMATCH, "assign: the matrix must be |I| x |J|");
    if (!Mask && !dv.mask_comp && !dv.tran0 && C != A && strictly_increasing(ri) && strictly_increasing(ci) && C->type->code < T_FC32 && A->type->code < T_FC32) {
      // `M[a:b, c:d] = A` with increasing index lists: A's tuples stay sorted when they move to (I[i], J[j]) — one merge of C's tuples
      // (without those of the region, unless an accumulator keeps them) with A's
      if (accum) check_binop(accum, "accum");
      mat_to_host(C); mat_to_host(A);
      const size_t cs = C->type->size, as = A->type->size; const int ccode = C->type->code, acode = A->type->code;
      auto in_region = [&](uint64_t i, uint64_t j) { return std::binary_search(ri.begin(), ri.end(), i) && std::binary_search(ci.begin(), ci.end(), j); };
      std::vector<GrB_Index> ni2, nj2; std::vector<uint8_t> nx;
      const size_t nc = C->hi.size(), na = A->hi.size();
      ni2.reserve(nc + na); nj2.reserve(nc + na); nx.reserve((nc + na) * cs);
      auto put = [&](uint64_t i, uint64_t j, const Val& v) { ni2.push_back(i); nj2.push_back(j); nx.insert(nx.end(), v.data(), v.data() + cs); };
      size_t p = 0, q = 0;
      while (p < nc || q < na) {
        const uint64_t ai = q < na ? ri[A->hi[q]] : 0, aj = q < na ? ci[A->hj[q]] : 0;
        const bool take_c = q >= na || (p < nc && (C->hi[p] < ai || (C->hi[p] == ai && C->hj[p] < aj)));
        if (take_c) {                                                   // an entry of C with no counterpart in A: kept outside the region, and inside it under an accumulator
          if (accum || !in_region(C->hi[p], C->hj[p])) put(C->hi[p], C->hj[p], val_at(C, p));
          p++;
        } else {
          Val av{}; memcpy(av.data(), &A->hx[q * as], as);
          const bool both = p < nc && C->hi[p] == ai && C->hj[p] == aj;
          put(ai, aj, both && accum ? combine(accum, ccode, val_at(C, p), acode, av) : cast(ccode, acode, av));
          if (both) p++;
          q++;
        }
      }
      C->hi.swap(ni2); C->hj.swap(nj2); C->hx.swap(nx); C->host_valid = true; mat_invalidate_device(C);
      return;
    }
    Map Cm = load(C, false), Am = load(A, dv.tran0), Mm; if (Mask) Mm = load(Mask, false);
    region_update(Cm, C->type->code, Am, A->type->code, ri, ci, accum, MaskView{&Mm, Mask ? Mask->type->code : 0, dv.mask_struct, dv.mask_comp, Mask != nullptr}, dv.replace, true, false, false, 0);
    store(C, Cm);
  });
}

static GrB_Info row_assign_any(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const IdxArg& ja, const GrB_Descriptor desc) {
  const GrB_Index* const J = ja.I;
  if (!C || !u) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_v(u, "assign"); if (mask) check_v(mask, "assign");
    const DescView dv(desc);
    if (i >= C->nrows) fail(GrB_INVALID_INDEX, "assign: row index out of range");
    vec_gate(u);
    if ((mask || !dv.mask_comp) && assign_on_device(C, dev_capable(u) && dev_capable(mask), ASSIGN_ROW_DEVICE_MIN_ENTRIES, [&] { return entries_known(u); }, ja.in_hbm()) && assign_line_device(C, mask, accum, u, true, i, ja, dv)) return;
    if (!mask && !dv.mask_comp && J == GrB_ALL && u->n == C->ncols && C->type->code < T_FC32 && u->type->code < T_FC32) {   // `M[i] = v`: the row's run of tuples is replaced in place (GrB_ALL is never listed: C may be 2^60 wide)
      mat_to_host(C);
      const auto r = row_range(C, i); Line cur; cur.reserve(r.second - r.first);
      for (size_t p = r.first; p < r.second; p++) cur.push_back({C->hj[p], val_at(C, p)});
      replace_line(C, true, i, assigned_line(cur, C->type->code, u, accum));
      return;
    }
    if (J == GrB_ALL && u->n != C->ncols) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of column indices");   // (before the list is asked for: GrB_ALL over 2^60 columns is never materialised)
    HostList hl; const auto ci = indices(hl.get(ja), ja.n, C->ncols, "assign");
    if (u->n != ci.size() || (mask && mask->n != C->ncols)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of column indices");
    Map Cm = load(C, false), U = load(u), Ut, Mm; if (mask) Mm = load(mask);
    for (auto& kv : U) Ut[{0, kv.first.first}] = kv.second;             // the vector as a 1 x nj row
    region_update(Cm, C->type->code, Ut, u->type->code, std::vector<uint64_t>{i}, ci, accum, MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}, dv.replace,
                  false, true, false, i);
    store(C, Cm);
  });
}

static GrB_Info col_assign_any(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, GrB_Index j, const GrB_Descriptor desc) {
  const GrB_Index* const I = ia.I;
  if (!C || !u) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_v(u, "assign"); if (mask) check_v(mask, "assign");
    const DescView dv(desc);
    if (j >= C->ncols) fail(GrB_INVALID_INDEX, "assign: column index out of range");
    vec_gate(u);
    if ((mask || !dv.mask_comp) && assign_on_device(C, dev_capable(u) && dev_capable(mask), ASSIGN_COL_DEVICE_MIN_ENTRIES, [&] { return entries_known(u); }, ia.in_hbm()) && assign_line_device(C, mask, accum, u, false, j, ia, dv)) return;
    if (!mask && !dv.mask_comp && I == GrB_ALL && u->n == C->nrows && C->type->code < T_FC32 && u->type->code < T_FC32) {   // `M[:, j] = v`: one merge pass over the tuples (GrB_ALL is never listed)
      replace_line(C, false, j, assigned_line(line_of(C, false, j), C->type->code, u, accum));
      return;
    }
    if (I == GrB_ALL && u->n != C->nrows) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of row indices");   // (as in GrB_Row_assign: before the list is asked for)
    HostList hl; const auto ri = indices(hl.get(ia), ia.n, C->nrows, "assign");
    if (u->n != ri.size() || (mask && mask->n != C->nrows)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of row indices");
    Map Cm = load(C, false), U = load(u), Mm; if (mask) Mm = load(mask);
    region_update(Cm, C->type->code, U, u->type->code, ri, std::vector<uint64_t>{j}, accum, MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}, dv.replace,
                  false, false, true, j);
    store(C, Cm);
  });
}

// ---- a vector as an index list: the VALUES of its entries, in index order (what extractTuples returns as X) -----------------------
// With a device the list is made in HBM and nothing visits the host: the bitmap compaction of grb_tuples.hip (skipped for a vector whose facts say "all
// present": its value array is the list), then k_index_widen (skipped for the two 64-bit types), then the parse of grb_index.hip like any list in HBM.
// Without a device, or for an index vector that has no HBM layout, the list is made from the host mirror and the call is the host-list call.
namespace {
struct VecList {
  DevBuf compact, wide; std::vector<GrB_Index> host; std::string kernels;
  const GrB_Index* I = GrB_ALL; GrB_Index n = 0; bool hbm = false;
  IdxArg arg() const { return IdxArg{I, n, hbm}; }
};
void vector_as_list(GrB_Vector iv, GrB_Vector out, VecList& L) {
  if (!iv) return;                                                        // no vector: GrB_ALL
  check_v(iv, "index vector");
  if (iv == out) fail(GrB_INVALID_VALUE, "the index vector must not be the output");
  const int code = iv->type->code; const size_t ts = iv->type->size;
  if (code < T_INT8 || code > T_UINT64) fail(GrB_DOMAIN_MISMATCH, "an index vector must have an integer type");
  const bool is_signed = code == T_INT8 || code == T_INT16 || code == T_INT32 || code == T_INT64;
  if (!device_ok() || !dev_capable(iv) || iv->n > GRB_DIM_DEVICE_MAX) {
    vec_to_host(iv); L.n = iv->hi.size(); L.host.resize(L.n ? L.n : 1);
    for (GrB_Index k = 0; k < L.n; k++) cast_scalar(is_signed ? T_INT64 : T_UINT64, &L.host[k], code, &iv->hx[k * ts]);      // (sign-extended, then read as unsigned)
    L.I = L.host.data(); return;
  }
  L.hbm = true;
  vec_to_device(iv);                                                      // deferred work that writes it completes, queued edits are applied, a host-resident vector is uploaded
  const uint64_t len = iv->n; const void* vals = iv->dval.p;
  if (len && iv->facts.dnvals_known && iv->facts.dnvals == len) L.n = len;
  else if (len) {
    DevBuf offs;
    L.n = tuples_count_bitmap(iv->dpres.as<uint8_t>(), len, offs);
    iv->facts.dnvals = L.n; iv->facts.dnvals_known = true;                // (learnt by reading the image, as GrBX_Vector_extractTuples_at records it)
    L.kernels = "k_tuples_count ";
    if (L.n) { L.compact.alloc(L.n * ts + 8); tuples_from_bitmap(iv->dpres.as<uint8_t>(), iv->dval.p, ts, len, offs, nullptr, L.compact.p); L.kernels += "k_tuples_scatter "; }
    GRB_HIP(hipStreamSynchronize(stream()));                              // `offs` goes out of scope
    vals = L.compact.p;
  }
  if (!L.n) { L.wide.alloc(8); L.I = L.wide.as<GrB_Index>(); return; }     // (an empty list still needs an address that is not NULL)
  if (ts == 8) { L.I = (const GrB_Index*)vals; return; }
  L.wide.alloc(L.n * 8); index_widen(code, vals, L.n, L.wide.as<uint64_t>()); L.kernels += "k_index_widen ";
  L.I = L.wide.as<GrB_Index>();
}
// The list's own kernels go in front of the operation's in the plan string — only when THIS call wrote one: the plan is set aside before the dispatch, and a
// call that ended on a host route (which writes none) gets the earlier word back untouched.
struct VectorListPlan {
  std::string before;
  VectorListPlan() { before.swap(g_last_plan); }
  void done(const VecList& a, const VecList& b) {
    if (g_last_plan.empty()) { g_last_plan.swap(before); return; }
    const size_t at = g_last_plan.find("> ");
    if (at != std::string::npos) g_last_plan.insert(at + 2, a.kernels + b.kernels);
  }
};
bool is_range_code(GrB_Index n) { return n == GXB_RANGE || n == GXB_STRIDE || n == GXB_BACKWARDS; }
// the `location` of an index argument: 0 a host array (or GrB_ALL, or a range triple), 1 a list of `ni` 64-bit indices in HBM (or GrB_ALL)
GrB_Info location_ok(int location, const GrB_Index* I, GrB_Index ni) {
  if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  if (location == 1 && I != GrB_ALL && is_range_code(ni)) return GrB_INVALID_VALUE;
  return GrB_SUCCESS;
}
}  // namespace

extern "C" {

GrB_Info GrB_Vector_extract(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc) {
  return vector_extract_any(w, mask, accum, u, IdxArg{I, ni, false}, desc);
}
GrB_Info GrB_Col_extract(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc) {
  return col_extract_any(w, mask, accum, A, IdxArg{I, ni, false}, j, desc);
}
GrB_Info GrB_Matrix_extract(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj,
                            const GrB_Descriptor desc) {
  return matrix_extract_any(C, Mask, accum, A, IdxArg{I, ni, false}, IdxArg{J, nj, false}, desc);
}
GrB_Info GrB_Vector_assign(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc) {
  return vector_assign_any(w, mask, accum, u, IdxArg{I, ni, false}, desc);
}
GrB_Info GrB_Matrix_assign(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj,
                           const GrB_Descriptor desc) {
  return matrix_assign_any(C, Mask, accum, A, IdxArg{I, ni, false}, IdxArg{J, nj, false}, desc);
}
GrB_Info GrB_Row_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const GrB_Index* J, GrB_Index nj, const GrB_Descriptor desc) {
  return row_assign_any(C, mask, accum, u, i, IdxArg{J, nj, false}, desc);
}
GrB_Info GrB_Col_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc) {
  return col_assign_any(C, mask, accum, u, IdxArg{I, ni, false}, j, desc);
}

// ---- the same seven with an index list that may lie in HBM: location 0 IS the GrB_ call; location 1: `ni` 64-bit indices at a device address (GrB_ALL is
// accepted with either value; a range code as the count of a list in HBM is GrB_INVALID_VALUE).  The call takes the device route wherever that route is legal —
// the entry-count thresholds do not apply, GRB_MI355X_EXTRACT / GRB_MI355X_ASSIGN = 0 still force the host route — and the list is parsed where it lies
// (grb_index.hip).  Where the device route is not legal (a hypersparse, complex, full one-valued or bitmap-only container, an operand that is the output, an assign
// whose list names an index twice) the list is copied down once and the host route answers.
GrB_Info GrBX_Vector_extract_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc, int location) {
  if (!w) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  if (!location) return GrB_Vector_extract(w, mask, accum, u, I, ni, desc);
  return vector_extract_any(w, mask, accum, u, IdxArg{I, ni, true}, desc);
}
GrB_Info GrBX_Col_extract_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc, int location) {
  if (!w) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  if (!location) return GrB_Col_extract(w, mask, accum, A, I, ni, j, desc);
  return col_extract_any(w, mask, accum, A, IdxArg{I, ni, true}, j, desc);
}
GrB_Info GrBX_Matrix_extract_at(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj,
                                const GrB_Descriptor desc, int location_i, int location_j) {
  if (!C) return GrB_NULL_POINTER;
  if (const GrB_Info e = location_ok(location_i, I, ni)) return e; if (const GrB_Info e = location_ok(location_j, J, nj)) return e;
  if (!location_i && !location_j) return GrB_Matrix_extract(C, Mask, accum, A, I, ni, J, nj, desc);
  return matrix_extract_any(C, Mask, accum, A, IdxArg{I, ni, location_i == 1}, IdxArg{J, nj, location_j == 1}, desc);
}
GrB_Info GrBX_Vector_assign_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc, int location) {
  if (!w) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  if (!location) return GrB_Vector_assign(w, mask, accum, u, I, ni, desc);
  return vector_assign_any(w, mask, accum, u, IdxArg{I, ni, true}, desc);
}
GrB_Info GrBX_Matrix_assign_at(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj,
                               const GrB_Descriptor desc, int location_i, int location_j) {
  if (!C) return GrB_NULL_POINTER;
  if (const GrB_Info e = location_ok(location_i, I, ni)) return e; if (const GrB_Info e = location_ok(location_j, J, nj)) return e;
  if (!location_i && !location_j) return GrB_Matrix_assign(C, Mask, accum, A, I, ni, J, nj, desc);
  return matrix_assign_any(C, Mask, accum, A, IdxArg{I, ni, location_i == 1}, IdxArg{J, nj, location_j == 1}, desc);
}
GrB_Info GrBX_Row_assign_at(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const GrB_Index* J, GrB_Index nj, const GrB_Descriptor desc, int location) {
  if (!C) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, J, nj)) return e;
  if (!location) return GrB_Row_assign(C, mask, accum, u, i, J, nj, desc);
  return row_assign_any(C, mask, accum, u, i, IdxArg{J, nj, true}, desc);
}
GrB_Info GrBX_Col_assign_at(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc, int location) {
  if (!C) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  if (!location) return GrB_Col_assign(C, mask, accum, u, I, ni, j, desc);
  return col_assign_any(C, mask, accum, u, IdxArg{I, ni, true}, j, desc);
}
GrB_Info GrBX_index_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = (uint64_t)INDEX_PARSE_THREADS * INDEX_PARSE_PER_LANE; out[1] = INDEX_PARSE_GRID_CAP; return GrB_SUCCESS;
}

// the parse alone (tools/index_probe.py times it): `ni` 64-bit indices in HBM against `dim`, with the errors of the entry points above
GrB_Info GrBX_index_parse(const GrB_Index* I, GrB_Index ni, GrB_Index dim, int* increasing) {
  if (!increasing) return GrB_NULL_POINTER;
  return guarded((GrB_Vector) nullptr, [&] { need_device(); ExIdx x; index_parse_device(x, I, ni, dim, "index parse"); *increasing = x.increasing ? 1 : 0; });
}

// ---- vectors as index lists (GxB_Vector_extract_Vector / GxB_Vector_assign_Vector / GxB_Matrix_extract_Vector of newer SuiteSparse): a NULL vector means all
GrB_Info GrBX_Vector_extract_Vector(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Vector Ivec, const GrB_Descriptor desc) {
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  VecList L; if (const GrB_Info e = guarded(w, [&] { vector_as_list(Ivec, w, L); })) return e;
  VectorListPlan plan; const GrB_Info info = vector_extract_any(w, mask, accum, u, L.arg(), desc);
  plan.done(L, VecList()); return info;
}
GrB_Info GrBX_Vector_assign_Vector(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Vector Ivec, const GrB_Descriptor desc) {
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  VecList L; if (const GrB_Info e = guarded(w, [&] { vector_as_list(Ivec, w, L); })) return e;
  VectorListPlan plan; const GrB_Info info = vector_assign_any(w, mask, accum, u, L.arg(), desc);
  plan.done(L, VecList()); return info;
}
GrB_Info GrBX_Matrix_extract_Vector(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Vector Ivec, const GrB_Vector Jvec, const GrB_Descriptor desc) {
  if (!C || !A) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  VecList Li, Lj; if (const GrB_Info e = guarded(C, [&] { vector_as_list(Ivec, nullptr, Li); vector_as_list(Jvec, nullptr, Lj); })) return e;
  VectorListPlan plan; const GrB_Info info = matrix_extract_any(C, Mask, accum, A, Li.arg(), Lj.arg(), desc);
  plan.done(Li, Lj); return info;
}

GrB_Info GrB_Matrix_kronecker_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  if (!C || !A || !B || !op) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_m(A, "kronecker"); check_m(B, "kronecker"); if (Mask) check_m(Mask, "kronecker"); check_binop(op, "kronecker");
    const DescView dv(desc);
    const uint64_t ar = dv.tran0 ? A->ncols : A->nrows, ac = dv.tran0 ? A->nrows : A->ncols, br = dv.tran1 ? B->ncols : B->nrows, bc = dv.tran1 ? B->nrows : B->ncols;
    if (C->nrows != ar * br || C->ncols != ac * bc || (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols))) fail(GrB_DIMENSION_MISMATCH, "kronecker: dimensions do not conform");
    if (kron_on_device(C, Mask, A, B, dv)) { kron_device(C, Mask, accum, op, A, B, dv); return; }
    Map Am = load(A, dv.tran0), Bm = load(B, dv.tran1), T, Cm = load(C, false), Mm; if (Mask) Mm = load(Mask, false);
    const int oc = op->xtype->code, zc = op->ztype->code;
    for (auto& a : Am) for (auto& b : Bm) {
      Val x = cast(oc, A->type->code, a.second), y = cast(oc, B->type->code, b.second), z{};
      dispatch_type(oc, [&]<class T>() { T p, q; memcpy(&p, x.data(), sizeof(T)); memcpy(&q, y.data(), sizeof(T)); T r = apply_binop<T>(op->opcode, p, q); memcpy(z.data(), &r, sizeof(T)); });
      T[{a.first.first * br + b.first.first, a.first.second * bc + b.first.second}] = z;
    }
    (void)zc;
    write_back(Cm, C->type->code, T, oc, MaskView{&Mm, Mask ? Mask->type->code : 0, dv.mask_struct, dv.mask_comp, Mask != nullptr}, dv.replace, accum, everywhere);
    store(C, Cm);
  });
}
// the C API 1.3 / SuiteSparse 5.1 spellings: a monoid stands for its operator, a semiring for its multiplier
GrB_Info GrB_Matrix_kronecker_Monoid(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  if (!op) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT;
  return GrB_Matrix_kronecker_BinaryOp(C, Mask, accum, op->op, A, B, desc);
}
GrB_Info GrB_Matrix_kronecker_Semiring(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  if (!op) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT;
  if (C && check_obj(C) && check_obj(op->mul) && is_positional_semiring(op)) return guarded(C, [&] { possr_refuse_elementwise(op, "kronecker"); });
  return GrB_Matrix_kronecker_BinaryOp(C, Mask, accum, op->mul, A, B, desc);
}
GrB_Info GxB_kron(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  return GrB_Matrix_kronecker_BinaryOp(C, Mask, accum, op, A, B, desc);
}
GrB_Info GrBX_kron_fill_ms(float* ms) { if (!ms) return GrB_NULL_POINTER; *ms = g_kron_fill_ms; return GrB_SUCCESS; }


// apply with the bound operand in a GxB_Scalar: forwarded to the typed entry point of the scalar's type
#define GRB_CASE1(SUF, CT, CODE) case CODE: { CT v; memcpy(&v, x->x, sizeof(CT)); return FN1(SUF)(C, M, accum, op, v, A, desc); }
#define GRB_CASE2(SUF, CT, CODE) case CODE: { CT v; memcpy(&v, x->x, sizeof(CT)); return FN2(SUF)(C, M, accum, op, A, v, desc); }
#define GRB_SCALAR_OK(x) if (!x) return GrB_NULL_POINTER; if (!check_obj(x)) return GrB_UNINITIALIZED_OBJECT; if (!x->has) return GrB_INVALID_VALUE;
GrB_Info GxB_Matrix_apply_BinaryOp1st(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GxB_Scalar x, const GrB_Matrix A, const GrB_Descriptor desc) {
  GRB_SCALAR_OK(x)
#define FN1(SUF) GxB_Matrix_apply_BinaryOp1st_##SUF
  switch (x->type->code) { GRB_FOR_TYPES(GRB_CASE1) default: return GrB_DOMAIN_MISMATCH; }
#undef FN1
}
GrB_Info GxB_Matrix_apply_BinaryOp2nd(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GxB_Scalar x, const GrB_Descriptor desc) {
  GRB_SCALAR_OK(x)
#define FN2(SUF) GxB_Matrix_apply_BinaryOp2nd_##SUF
  switch (x->type->code) { GRB_FOR_TYPES(GRB_CASE2) default: return GrB_DOMAIN_MISMATCH; }
#undef FN2
}
GrB_Info GxB_Vector_apply_BinaryOp1st(GrB_Vector C, const GrB_Vector M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GxB_Scalar x, const GrB_Vector A, const GrB_Descriptor desc) {
  GRB_SCALAR_OK(x)
#define FN1(SUF) GxB_Vector_apply_BinaryOp1st_##SUF
  switch (x->type->code) { GRB_FOR_TYPES(GRB_CASE1) default: return GrB_DOMAIN_MISMATCH; }
#undef FN1
}
GrB_Info GxB_Vector_apply_BinaryOp2nd(GrB_Vector C, const GrB_Vector M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Vector A, const GxB_Scalar x, const GrB_Descriptor desc) {
  GRB_SCALAR_OK(x)
#define FN2(SUF) GxB_Vector_apply_BinaryOp2nd_##SUF
  switch (x->type->code) { GRB_FOR_TYPES(GRB_CASE2) default: return GrB_DOMAIN_MISMATCH; }
#undef FN2
}

double GxB_ALWAYS_HYPER = 1.0, GxB_NEVER_HYPER = -1.0, GxB_HYPER_DEFAULT = 0.0625;      // hyper_switch settings (stored options only)


// ---- a scalar into a region, on the host mirror ------------------------------------------------------------------
// Used for containers that have no HBM layout: complex ones (`Matrix.dense(FC64, 10, 10)` is `M[:, :] = 0j`,
// pygraphblas/matrix.py:225-230; tests/test_matrix.py:853) and those whose dimensions exceed the 32-bit device layout
// (the hypersparse default, GxB_INDEX_MAX: `Matrix.sparse(float, fill=3.14, mask=mask)`, pygraphblas/matrix.py:154-162,
// `Matrix.iso(3)`, :234-266).  Container bookkeeping, like setElement — never on the mxm / mxv / vxm path.
typedef struct { float re, im; } GxB_FC32_t;
typedef struct { double re, im; } GxB_FC64_t;
}  // extern "C"
namespace grb {
void host_assign_scalar(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, GrB_Descriptor desc) {
  if (Mask) check_m(Mask, "assign");
  const DescView dv(desc);
  if (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols)) fail(GrB_DIMENSION_MISMATCH, "assign: mask dimensions");
  const bool all = (I == GrB_ALL && J == GrB_ALL);
  const int ccode = C->type->code;
  Val v{}; memcpy(v.data(), x, (size_t)type_size(xcode));
  const double positions = index_count(I, ni, C->nrows) * index_count(J, nj, C->ncols);      // (ni / nj may be a range sentinel, not a count)
  if (all && Mask && !dv.mask_comp) {                    // the result's pattern is bounded by the mask's
    Map Cm = load(C, false), Mm = load(Mask, false), T;
    const MaskView mk{&Mm, Mask->type->code, dv.mask_struct, false, true};
    for (auto& kv : Mm) if (mk.allows(kv.first)) T[kv.first] = v;
    write_back(Cm, ccode, T, xcode, mk, dv.replace, accum, everywhere);
    store(C, Cm); return;
  }
  if (all && !Mask && positions > 16777216.0) {          // every position of a container too large to enumerate: one stored value
    if (accum && mat_nvals(C) != 0) fail(GrB_INSUFFICIENT_SPACE, "assign: accumulating a scalar into every position of a container of this dimension");
    GrB_Matrix_clear(C); C->iso_full = true; memset(C->iso_val, 0, 16); cast_scalar(ccode, C->iso_val, xcode, x); return;
  }
  if (positions > 16777216.0) fail(GrB_INSUFFICIENT_SPACE, "assign: a scalar over more than 2^24 positions of a host-side container");
  const auto ri = indices(I, ni, C->nrows, "assign"), ci = indices(J, nj, C->ncols, "assign");
  Map Cm = load(C, false), Am, Mm; if (Mask) Mm = load(Mask, false);
  for (size_t a = 0; a < ri.size(); a++) for (size_t b = 0; b < ci.size(); b++) Am[{a, b}] = v;
  region_update(Cm, ccode, Am, xcode, ri, ci, accum, MaskView{&Mm, Mask ? Mask->type->code : 0, dv.mask_struct, dv.mask_comp, Mask != nullptr}, dv.replace, true, false, false, 0);
  store(C, Cm);
}
void host_assign_scalar(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, GrB_Descriptor desc) {
  if (mask) check_v(mask, "assign");
  const DescView dv(desc);
  if (mask && mask->n != w->n) fail(GrB_DIMENSION_MISMATCH, "assign: mask size");
  const bool all = (I == GrB_ALL);
  const int wcode = w->type->code;
  Val v{}; memcpy(v.data(), x, (size_t)type_size(xcode));
  const double positions = index_count(I, ni, w->n);
  if (all && mask && !dv.mask_comp) {
    Map C = load(w), Mm = load(mask), T;
    const MaskView mk{&Mm, mask->type->code, dv.mask_struct, false, true};
    for (auto& kv : Mm) if (mk.allows(kv.first)) T[kv.first] = v;
    write_back(C, wcode, T, xcode, mk, dv.replace, accum, everywhere);
    store(w, C); return;
  }
  if (all && !mask && positions > 16777216.0) {
    if (accum && vec_nvals(w) != 0) fail(GrB_INSUFFICIENT_SPACE, "assign: accumulating a scalar into every position of a container of this dimension");
    GrB_Vector_clear(w); w->iso_full = true; memset(w->iso_val, 0, 16); cast_scalar(wcode, w->iso_val, xcode, x); return;
  }
  if (positions > 16777216.0) fail(GrB_INSUFFICIENT_SPACE, "assign: a scalar over more than 2^24 positions of a host-side container");
  const auto idx = indices(I, ni, w->n, "assign");
  Map C = load(w), U, Mm; if (mask) Mm = load(mask);
  for (size_t a = 0; a < idx.size(); a++) U[{a, 0}] = v;
  region_update(C, wcode, U, xcode, idx, std::vector<uint64_t>{0}, accum, MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}, dv.replace, true, false, false, 0);
  store(w, C);
}
}  // namespace grb
extern "C" {
static GrB_Info mat_assign_complex(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, GrB_Descriptor desc) {
  if (!C) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] { host_assign_scalar(C, Mask, accum, x, xcode, I, ni, J, nj, desc); });
}
static GrB_Info vec_assign_complex(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, GrB_Descriptor desc) {
  if (!w) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] { host_assign_scalar(w, mask, accum, x, xcode, I, ni, desc); });
}
GrB_Info GxB_Matrix_assign_FC32(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, GxB_FC32_t x, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, const GrB_Descriptor desc) { return mat_assign_complex(C, M, accum, &x, T_FC32, I, ni, J, nj, desc); }
GrB_Info GxB_Matrix_assign_FC64(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, GxB_FC64_t x, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, const GrB_Descriptor desc) { return mat_assign_complex(C, M, accum, &x, T_FC64, I, ni, J, nj, desc); }
GrB_Info GxB_Vector_assign_FC32(GrB_Vector w, const GrB_Vector m, const GrB_BinaryOp accum, GxB_FC32_t x, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc) { return vec_assign_complex(w, m, accum, &x, T_FC32, I, ni, desc); }
GrB_Info GxB_Vector_assign_FC64(GrB_Vector w, const GrB_Vector m, const GrB_BinaryOp accum, GxB_FC64_t x, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc) { return vec_assign_complex(w, m, accum, &x, T_FC64, I, ni, desc); }

// ---- GxB_Matrix_diag / GxB_Vector_diag (Matrix.from_diag, Matrix.vector_diag: pygraphblas/matrix.py:333-375, 2225-2277) ----
}  // extern "C"
namespace {
// ---- diagonals: which route -------------------------------------------------------------------------------------------------------
// The device route (grb_diag.hip) is taken when a HIP device is present, the vector and the matrix of the call have an HBM layout (dev_capable /
// mat_capable) and the operand either lives in HBM only (it is not downloaded for this, and its entry count is not asked) or holds at least N entries,
// one N per entry point: the crossover against this file's host route below, upload of a host-resident operand included.  Small
// host-resident containers — the 3 x 3 docstring examples — keep the host route.  GRB_MI355X_DIAG=0 forces the host route, =1 the device route wherever
// it is legal (read per call: a test hook).  The argument and dimension checks come before the choice and are the same on both routes.
constexpr uint64_t DIAG_MATRIX_DEVICE_MIN_ENTRIES = 1000;       // GxB_Matrix_diag: measured, the host route is one std::map insertion per entry (0.11 ms against 0.07 ms at 1e3 entries)
constexpr uint64_t DIAG_VECTOR_DEVICE_MIN_ENTRIES = 10000;      // GxB_Vector_diag: measured, the host route is one pass over A's tuples (0.11 ms against 0.07 ms at 1e4 entries)
bool diag_matrix_on_device(GrB_Matrix C, GrB_Vector v) {
  const int env = route_env("GRB_MI355X_DIAG");
  if (env == 0 || !device_ok() || !mat_capable(C) || !dev_capable(v)) return false;
  if (env == 1) return true;
  vec_gate(v);                                                          // deferred work that involves v is completed first, as every reader does
  if (v->dev_valid && !v->host_valid) return true;                      // it lives in HBM: it is not downloaded for this
  return v->host_valid && vec_nvals(v) >= DIAG_MATRIX_DEVICE_MIN_ENTRIES;   // (the count of a valid host mirror: no device work)
}
bool diag_vector_on_device(GrB_Vector v, GrB_Matrix A) {
  const int env = route_env("GRB_MI355X_DIAG");
  if (env == 0 || !device_ok() || !mat_capable(A) || !dev_capable(v)) return false;
  if (env == 1) return true;
  if (hbm_only(A)) return true;
  return A->host_valid && mat_nvals(A) >= DIAG_VECTOR_DEVICE_MIN_ENTRIES;
}
}  // namespace
extern "C" {
GrB_Info GrBX_diag_thresholds(uint64_t* matrix_min_entries, uint64_t* vector_min_entries) {
  if (!matrix_min_entries || !vector_min_entries) return GrB_NULL_POINTER;
  *matrix_min_entries = DIAG_MATRIX_DEVICE_MIN_ENTRIES; *vector_min_entries = DIAG_VECTOR_DEVICE_MIN_ENTRIES; return GrB_SUCCESS;
}
// (the descriptor has no field either operation reads: it is ignored on both routes)
GrB_Info GxB_Matrix_diag(GrB_Matrix C, const GrB_Vector v, int64_t k, const GrB_Descriptor desc) {
  (void)desc; if (!C || !v) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_v(v, "diag");
    const uint64_t ak = diag_abs(k); uint64_t n = 0;
    if (!diag_dim(v->n, k, &n) || C->nrows != n || C->ncols != n) fail(GrB_DIMENSION_MISMATCH, "diag: C must be square of dimension size(v) + |k|");
    g_last_plan.clear();
    if (diag_matrix_on_device(C, v)) {
      vec_to_device(v);                                                  // (completes deferred work on v: a lazily filled `v[:] = s` arrives as its bitmap)
      DevCSR T;
      const bool full = diag_to_csr(v->type->code, v->n, v->dval.p, v->dpres.as<uint8_t>(), k, T, v->facts.dnvals_known && v->facts.dnvals == v->n);
      g_last_plan = std::string("diag_matrix<k=") + std::to_string(k) + ",full=" + (full ? "1" : "0") + "> k_diag_fill ";
      const DescView dv(nullptr);
      matrix_write_back(C, T, v->type->code, nullptr, dv, nullptr, false);      // C becomes exactly T in C's type: its entries and pending edits are gone, as below
      return;
    }
    Map V = load(v), out;
    for (auto& kv : V) { const uint64_t i = kv.first.first; out[k >= 0 ? std::make_pair(i, i + ak) : std::make_pair(i + ak, i)] = cast(C->type->code, v->type->code, kv.second); }
    store(C, out);
  });
}
GrB_Info GxB_Vector_diag(GrB_Vector v, const GrB_Matrix A, int64_t k, const GrB_Descriptor desc) {
  (void)desc; if (!v || !A) return GrB_NULL_POINTER; if (!check_obj(v)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(v, [&] {
    check_m(A, "diag");
    const uint64_t len = diag_len(A->nrows, A->ncols, k);
    if (v->n != len) fail(GrB_DIMENSION_MISMATCH, "diag: the vector must have the length of the k-th diagonal");
    g_last_plan.clear();
    if (diag_vector_on_device(v, A)) {
      mat_to_device(A);
      const size_t ts = A->type->size;
      DevBuf tval(len * ts + 8), tpres(len + 1);
      csr_diag_to_bitmap(ts, A->csr, k, len, tval.p, tpres.as<uint8_t>());
      g_last_plan = std::string("diag_vector<k=") + std::to_string(k) + "> k_diag_read ";
      vec_overwritten(v);
      vector_write_back(v, A->type->code, tval, tpres, nullptr, nullptr, false, false);
      return;
    }
    mat_to_host(A); Map out;                                              // one pass over A's sorted tuples: no map of the whole matrix
    const uint64_t r0 = diag_row0(k), c0 = diag_col0(k);
    for (size_t p = 0; p < A->hi.size(); p++) {
      const uint64_t i = A->hi[p], j = A->hj[p];
      if (i >= r0 && j >= c0 && i - r0 == j - c0) out[{i - r0, 0}] = cast(v->type->code, A->type->code, val_at(A, p));
    }
    store(v, out);
  });
}
}  // extern "C"

// ---- GxB_Matrix_sort / GxB_Vector_sort / GrBX_*_select_topk ------------------------------------------------------------------------------
namespace {
// The comparator: GrB_LT_<T> or GrB_GT_<T> of a real type, nothing else (LE / GE are not strict; user-defined and positional operators and complex types have
// no key).  The comparison runs in T: on the operand's values cast to it.
struct SortOp { int code; bool gt; };
SortOp sort_op(GrB_BinaryOp op, const char* what) {
  if (!check_obj(op)) fail(GrB_UNINITIALIZED_OBJECT, std::string(what) + ": the comparator is not initialised");
  if (is_user(op) || (op->opcode != B_LT && op->opcode != B_GT) || !check_obj(op->xtype) || op->xtype->code >= T_FC32)
    fail(GrB_DOMAIN_MISMATCH, std::string(what) + ": the comparator must be GrB_LT_<T> or GrB_GT_<T> of a real type, not " + op->name);
  return {op->xtype->code, op->opcode == B_GT};
}
void sort_real(const GrB_Type t, const char* what) { if (t->code >= T_FC32) fail(GrB_DOMAIN_MISMATCH, std::string(what) + ": complex values have no order"); }

// ---- which route ----------------------------------------------------------------------------------------------------------------------
// As index-list extract: the device route (grb_sort.hip) when a HIP device is present, every container of the call has an HBM layout and the operand lives in
// HBM only or holds at least EXTRACT_DEVICE_MIN_ENTRIES entries.  GRB_MI355X_SORT=0 forces the host route, =1 the device route wherever it is legal, =prim keeps
// the choice and sends every row through the segmented radix sort (for comparison only).  Read per call: test hooks.
struct SortRoute { bool device, prim; };
int sort_env(bool* prim) { const char* e = getenv("GRB_MI355X_SORT"); *prim = e && !strcmp(e, "prim"); return *prim ? -1 : route_env("GRB_MI355X_SORT"); }
SortRoute sort_route(GrB_Matrix A, bool others_capable) {
  bool prim = false; const int env = sort_env(&prim);
  if (env == 0 || !device_ok() || !others_capable || !mat_capable(A)) return {false, prim};
  if (env == 1 || hbm_only(A)) return {true, prim};
  return {A->host_valid && mat_nvals(A) >= EXTRACT_DEVICE_MIN_ENTRIES, prim};
}
SortRoute sort_route(GrB_Vector u, bool others_capable) {
  bool prim = false; const int env = sort_env(&prim);
  if (env == 0 || !device_ok() || !others_capable || !dev_capable(u)) return {false, prim};
  if (env == 1) return {true, prim};
  vec_gate(u);
  if (u->dev_valid && !u->host_valid) return {true, prim};
  return {u->host_valid && vec_nvals(u) >= EXTRACT_DEVICE_MIN_ENTRIES, prim};
}
std::string sort_plan_head(bool topk, const char* on, const char* by, const SortOp& so, const SortPlan& sp, uint64_t k, uint64_t nvals) {
  std::string s = std::string(topk ? "topk<on=" : "sort<on=") + on + (by ? std::string(",by=") + by : std::string()) + ",op=" + (so.gt ? "gt" : "lt") + ",key=" + std::to_string(sp.key_bits);
  if (by) s += ",wave=" + std::to_string(sp.wave) + ",lds=" + std::to_string(sp.lds) + ",prim=" + std::to_string(sp.prim);
  else s += ",nvals=" + std::to_string(nvals);
  if (topk) s += ",k=" + std::to_string(k);
  return s + "> ";
}
const DescView no_desc(nullptr);

// C = the lines of op(A) in sorted order / P = where each value came from (sort), or C = the first min(k, len) entries of every line at their own coordinates
// (topk; P is nullptr).  The checks are done; the outputs may alias A: everything is computed before the first of them is written.
void sort_matrix_device(GrB_Matrix C, GrB_Matrix P, const SortOp& so, GrB_Matrix A, bool tran, bool prim, bool topk, uint64_t k) {
  mat_to_device(A);
  const DevCSR& R = tran ? mat_csc(A) : A->csr;
  const int acode = A->type->code; const size_t ts = A->type->size;
  DevBuf kcast, perm, ocol; SortPlan sp;
  const void* kv = cast_values(so.code, acode, R.val.p, R.nnz, kcast);                // (the operator's type is A's: no pass)
  csr_sort_positions(R, so.code, kv, so.gt, prim, perm, ocol, sp);
  std::string plan = sort_plan_head(topk, "matrix", tran ? "col" : "row", so, sp, k, 0) + (kv != R.val.p ? "k_cast_values " : "") + sp.kernels;
  DevCSR T, Tp, Tt, Tpt;
  if (topk) {
    DevBuf keep(R.nnz + 16);
    topk_flags(R.nnz, perm, ocol, k, keep.as<uint8_t>());
    csr_compact(R, R.val.p, ts, keep.as<uint8_t>(), T);
    plan += "k_topk_flags csr_compact ";
  } else {
    csr_sort_fill(R, ts, perm, ocol, C ? &T : nullptr, P ? &Tp : nullptr);
    plan += "k_sort_gather ";
  }
  if (tran) {
    if (C) { csr_transpose(T, ts, Tt); T.clear(); }
    if (P) { csr_transpose(Tp, 8, Tpt); Tp.clear(); }
    plan += "csr_transpose ";
  }
  GRB_HIP(hipStreamSynchronize(stream()));
  if (C) matrix_write_back(C, tran ? Tt : T, acode, nullptr, no_desc, nullptr, false);      // C becomes exactly T in C's type: its entries and pending edits are gone
  if (P) matrix_write_back(P, tran ? Tpt : Tp, T_INT64, nullptr, no_desc, nullptr, false);
  g_last_plan = plan;
}

// one line of the host route: places of A's tuples, in index order on entry, in sorted order on return
void sort_line(std::vector<size_t>& ord, size_t a, size_t b, const std::vector<uint64_t>& key) {
  std::stable_sort(ord.begin() + a, ord.begin() + b, [&](size_t x, size_t y) { return key[x] < key[y]; });
}
uint64_t host_key(const SortOp& so, int code, const uint8_t* x) { Val v{}, c; memcpy(v.data(), x, (size_t)type_size(code)); c = cast(so.code, code, v); return sort_key_at(so.code, c.data(), so.gt); }
Val index_val(uint64_t i) { Val v{}; const int64_t x = (int64_t)i; memcpy(v.data(), &x, 8); return v; }

void sort_matrix_host(GrB_Matrix C, GrB_Matrix P, const SortOp& so, GrB_Matrix A, bool tran, bool topk, uint64_t k) {
  mat_to_host(A);
  const size_t n = A->hi.size(); const int acode = A->type->code; const size_t ts = A->type->size;
  std::vector<uint64_t> key(n); std::vector<size_t> ord(n);
  for (size_t p = 0; p < n; p++) { key[p] = host_key(so, acode, &A->hx[p * ts]); ord[p] = p; }
  const std::vector<GrB_Index>& line = tran ? A->hj : A->hi; const std::vector<GrB_Index>& idx = tran ? A->hi : A->hj;
  if (tran) std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return A->hj[x] < A->hj[y]; });      // by column; rows stay ascending within one
  Map Cm, Pm;
  for (size_t a = 0; a < n;) {
    size_t b = a; while (b < n && line[ord[b]] == line[ord[a]]) b++;
    sort_line(ord, a, b, key);
    for (size_t q = 0; a + q < b; q++) {
      const size_t p = ord[a + q];
      if (topk) { if (q < k) Cm[{A->hi[p], A->hj[p]}] = cast(C->type->code, acode, val_at(A, p)); continue; }
      const auto at = tran ? std::make_pair((uint64_t)q, (uint64_t)line[p]) : std::make_pair((uint64_t)line[p], (uint64_t)q);
      if (C) Cm[at] = cast(C->type->code, acode, val_at(A, p));
      if (P) Pm[at] = index_val(idx[p]);
    }
    a = b;
  }
  if (C) store(C, Cm);
  if (P) store(P, Pm);
}

void sort_matrix(GrB_Matrix C, GrB_Matrix P, GrB_BinaryOp op, GrB_Matrix A, GrB_Descriptor desc, bool topk, uint64_t k) {
  const char* what = topk ? "select_topk" : "sort";
  check_m(A, what); if (C) check_m(C, what); if (P) check_m(P, what);
  const SortOp so = sort_op(op, what);
  sort_real(A->type, what); if (C) sort_real(C->type, what);
  const DescView dv(desc);
  for (GrB_Matrix O : {C, P}) if (O && (O->nrows != A->nrows || O->ncols != A->ncols)) fail(GrB_DIMENSION_MISMATCH, std::string(what) + ": the outputs must have A's dimensions");
  if (P && P->type->code != T_INT64) fail(GrB_DOMAIN_MISMATCH, std::string(what) + ": P must be GrB_INT64");
  g_last_plan.clear();
  const SortRoute rt = sort_route(A, mat_capable(C) && mat_capable(P));
  if (rt.device) sort_matrix_device(C, P, so, A, dv.tran0, rt.prim, topk, k);
  else sort_matrix_host(C, P, so, A, dv.tran0, topk, k);
}

void sort_vector_device(GrB_Vector w, GrB_Vector p, const SortOp& so, GrB_Vector u, bool topk, uint64_t k) {
  vec_to_device(u);
  const uint64_t n = u->n; const int ucode = u->type->code; const size_t ts = u->type->size;
  DevBuf kcast, sidx; SortPlan sp;
  const void* kv = cast_values(so.code, ucode, u->dval.p, n, kcast);
  const uint64_t nvals = vec_sort_positions(so.code, kv, u->dpres.as<uint8_t>(), n, so.gt, sidx, sp);
  std::string plan = sort_plan_head(topk, "vector", nullptr, so, sp, k, nvals) + (kv != u->dval.p ? "k_cast_values " : "") + sp.kernels;
  DevBuf tval(n * ts + 8), tpres(n + 1), pval, ppres;
  if (topk) {
    const uint64_t keep = topk_keep(k, nvals);
    if (n) GRB_HIP(hipMemcpyAsync(tval.p, u->dval.p, n * ts, hipMemcpyDeviceToDevice, stream()));
    vec_topk_flags(sidx, keep, n, tpres.as<uint8_t>());
    plan += "k_vec_topk_flags ";
    GRB_HIP(hipStreamSynchronize(stream()));
    vec_overwritten(w);
    vector_write_back(w, ucode, tval, tpres, nullptr, nullptr, false, false, keep);
  } else {
    if (p) { pval.alloc(n * 8 + 8); ppres.alloc(n + 1); }
    vec_sort_fill(ts, u->dval.p, sidx, nvals, n, w ? tval.p : nullptr, w ? tpres.as<uint8_t>() : nullptr, p ? pval.p : nullptr, p ? ppres.as<uint8_t>() : nullptr);
    plan += "k_vec_sort_fill ";
    GRB_HIP(hipStreamSynchronize(stream()));
    if (w) { vec_overwritten(w); vector_write_back(w, ucode, tval, tpres, nullptr, nullptr, false, false, nvals); }
    if (p) { vec_overwritten(p); vector_write_back(p, T_INT64, pval, ppres, nullptr, nullptr, false, false, nvals); }
  }
  g_last_plan = plan;
}

void sort_vector_host(GrB_Vector w, GrB_Vector p, const SortOp& so, GrB_Vector u, bool topk, uint64_t k) {
  vec_to_host(u);
  const size_t n = u->hi.size(); const int ucode = u->type->code; const size_t ts = u->type->size;
  std::vector<uint64_t> key(n); std::vector<size_t> ord(n);
  for (size_t q = 0; q < n; q++) { key[q] = host_key(so, ucode, &u->hx[q * ts]); ord[q] = q; }
  sort_line(ord, 0, n, key);
  Map Wm, Pm;
  for (size_t q = 0; q < n; q++) {
    const size_t s = ord[q]; Val v{}; memcpy(v.data(), &u->hx[s * ts], ts);
    if (topk) { if (q < k) Wm[{u->hi[s], 0}] = cast(w->type->code, ucode, v); continue; }
    if (w) Wm[{q, 0}] = cast(w->type->code, ucode, v);
    if (p) Pm[{q, 0}] = index_val(u->hi[s]);
  }
  if (w) { vec_overwritten(w); store(w, Wm); }
  if (p) { vec_overwritten(p); store(p, Pm); }
}

void sort_vector(GrB_Vector w, GrB_Vector p, GrB_BinaryOp op, GrB_Vector u, bool topk, uint64_t k) {
  const char* what = topk ? "select_topk" : "sort";
  check_v(u, what); if (w) check_v(w, what); if (p) check_v(p, what);
  const SortOp so = sort_op(op, what);
  sort_real(u->type, what); if (w) sort_real(w->type, what);
  for (GrB_Vector o : {w, p}) if (o && o->n != u->n) fail(GrB_DIMENSION_MISMATCH, std::string(what) + ": the outputs must have u's size");
  if (p && p->type->code != T_INT64) fail(GrB_DOMAIN_MISMATCH, std::string(what) + ": p must be GrB_INT64");
  g_last_plan.clear();
  const SortRoute rt = sort_route(u, dev_capable(w) && dev_capable(p));
  if (rt.device) sort_vector_device(w, p, so, u, topk, k);
  else sort_vector_host(w, p, so, u, topk, k);
}
}  // namespace
extern "C" {
GrB_Info GrBX_sort_thresholds(uint64_t* wave_max, uint64_t* lds_max) {
  if (!wave_max || !lds_max) return GrB_NULL_POINTER;
  *wave_max = SORT_WAVE_EDGE; *lds_max = SORT_LDS_EDGE; return GrB_SUCCESS;      // the edges the default route uses (grb_sort_keys.hpp)
}
// (of the descriptor only GrB_INP0 is read: there is no mask and no accumulator)
GrB_Info GxB_Matrix_sort(GrB_Matrix C, GrB_Matrix P, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Descriptor desc) {
  if ((!C && !P) || !op || !A) return GrB_NULL_POINTER;
  GrB_Matrix out = C ? C : P; if (!check_obj(out)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(out, [&] { sort_matrix(C, P, op, A, desc, false, 0); });
}
GrB_Info GxB_Vector_sort(GrB_Vector w, GrB_Vector p, const GrB_BinaryOp op, const GrB_Vector u, const GrB_Descriptor desc) {
  if ((!w && !p) || !op || !u) return GrB_NULL_POINTER;
  GrB_Vector out = w ? w : p; if (!check_obj(out)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(out, [&] { const DescView dv(desc); (void)dv; sort_vector(w, p, op, u, false, 0); });
}
GrB_Info GrBX_Matrix_select_topk(GrB_Matrix C, const GrB_BinaryOp op, const GrB_Matrix A, GrB_Index k, const GrB_Descriptor desc) {
  if (!C || !op || !A) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] { sort_matrix(C, nullptr, op, A, desc, true, k); });
}
GrB_Info GrBX_Vector_select_topk(GrB_Vector w, const GrB_BinaryOp op, const GrB_Vector u, GrB_Index k, const GrB_Descriptor desc) {
  if (!w || !op || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] { const DescView dv(desc); (void)dv; sort_vector(w, nullptr, op, u, true, k); });
}
}  // extern "C"
