// grb_sort_ops.cpp — sort the lines of a matrix or a vector by value, and top-k selection, both routes.
//
//   GxB_Matrix_sort, GxB_Vector_sort, GrBX_{Matrix,Vector}_select_topk   <- Matrix.sort, Vector.sort, Matrix.topk, Vector.topk (no reference counterpart: the SuiteSparse 6.1 entry points)
//
// The host route works on the host mirror (grb_hostmap.hpp: a stable sort per line); the kernels of the device route are in grb_sort.hip, the order of the
// keys in grb_sort_keys.hpp.
//
// Route (the rule and SORT_DEVICE_MIN_ENTRIES: grb_route.hpp): hook GRB_MI355X_SORT; legal when every container of the call has an HBM layout; by size on the
// operand's host-mirror count.  GRB_MI355X_SORT=prim keeps the by-size choice and sends every row through the segmented radix sort (for comparison only).
#include "grb_hostmap.hpp"
#include "grb_matops.hpp"
#include "grb_sort.hpp"

using namespace grb;
using namespace grb::hostmap;

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

struct SortRoute { bool device, prim; };
int sort_env(bool* prim) { const char* e = getenv("GRB_MI355X_SORT"); *prim = e && !strcmp(e, "prim"); return *prim ? -1 : route_env("GRB_MI355X_SORT"); }
SortRoute sort_route(GrB_Matrix A, bool others_capable) {
  bool prim = false; const RouteStep s = route_first(sort_env(&prim), device_ok(), others_capable && mat_capable(A), false);
  return {s == ROUTE_BY_SIZE ? route_by_host_count(A, SORT_DEVICE_MIN_ENTRIES) : s == ROUTE_DEVICE, prim};
}
SortRoute sort_route(GrB_Vector u, bool others_capable) {
  bool prim = false; const RouteStep s = route_first(sort_env(&prim), device_ok(), others_capable && dev_capable(u), false);
  if (s != ROUTE_BY_SIZE) return {s == ROUTE_DEVICE, prim};
  vec_gate(u);                                                          // deferred work that involves u is completed first, as every reader does
  return {route_by_host_count(u, SORT_DEVICE_MIN_ENTRIES), prim};
}
std::string sort_plan_head(bool topk, const char* on, const char* by, const SortOp& so, const SortPlan& sp, uint64_t k, uint64_t nvals) {
  std::string s = std::string(topk ? "topk<on=" : "sort<on=") + on + (by ? std::string(",by=") + by : std::string()) + ",op=" + (so.gt ? "gt" : "lt") + ",key=" + std::to_string(sp.key_bits);
  if (by) s += ",wave=" + std::to_string(sp.wave) + ",lds=" + std::to_string(sp.lds) + ",prim=" + std::to_string(sp.prim);
  else s += ",nvals=" + std::to_string(nvals);
  if (topk) s += ",k=" + std::to_string(k);
  return s + "> ";
}


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
// (of the descriptor only GrB_INP0 is read: there is no mask and no accumulator; the vector forms read nothing of it and only validate it)
GrB_Info GxB_Matrix_sort(GrB_Matrix C, GrB_Matrix P, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Descriptor desc) {
  if ((!C && !P) || !op || !A) return GrB_NULL_POINTER;
  GrB_Matrix out = C ? C : P; if (!check_obj(out)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(out, [&] { sort_matrix(C, P, op, A, desc, false, 0); });
}
GrB_Info GxB_Vector_sort(GrB_Vector w, GrB_Vector p, const GrB_BinaryOp op, const GrB_Vector u, const GrB_Descriptor desc) {
  if ((!w && !p) || !op || !u) return GrB_NULL_POINTER;
  GrB_Vector out = w ? w : p; if (!check_obj(out)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(out, [&] { const DescView dv(desc); sort_vector(w, p, op, u, false, 0); });
}
GrB_Info GrBX_Matrix_select_topk(GrB_Matrix C, const GrB_BinaryOp op, const GrB_Matrix A, GrB_Index k, const GrB_Descriptor desc) {
  if (!C || !op || !A) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] { sort_matrix(C, nullptr, op, A, desc, true, k); });
}
GrB_Info GrBX_Vector_select_topk(GrB_Vector w, const GrB_BinaryOp op, const GrB_Vector u, GrB_Index k, const GrB_Descriptor desc) {
  if (!w || !op || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] { const DescView dv(desc); sort_vector(w, nullptr, op, u, true, k); });
}
}  // extern "C"
