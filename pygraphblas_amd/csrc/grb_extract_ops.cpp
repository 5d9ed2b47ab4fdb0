// grb_extract_ops.cpp — index-list extract, both routes: sub-vector, column (or row) of a matrix, sub-matrix.
//
//   GrB_Vector_extract, GrB_Col_extract, GrB_Matrix_extract     <- Vector / Matrix slicing  (pygraphblas/vector.py:1526-1573, matrix.py:2807-2990)
//
// The host route works on the host mirror (grb_hostmap.hpp); the kernels of the device route are in grb_extract.hip, its write-back in grb_matrix_ops.cpp /
// grb_vector_ops.cpp.  The entry points with a list in HBM (GrBX_*_at, GrBX_*_Vector) are in grb_index_ops.cpp and end in the same `_any` functions.
//
// Route (the rule and EXTRACT_DEVICE_MIN_ENTRIES: grb_route.hpp): hook GRB_MI355X_EXTRACT; legal when every container of the call has an HBM layout and the
// operand is not a bitmap-only batch matrix; forced by a list in HBM; by size on the operand's host-mirror count.  Small host-resident containers — notebook slices — keep the host route.
// GRB_MI355X_EXTRACT_BISECT=1 makes a column list bisect instead of using its table (read per call: a test hook).
#include "grb_hostmap.hpp"
#include "grb_index_ops.hpp"
#include "grb_matops.hpp"

using namespace grb;
using namespace grb::hostmap;

namespace {

bool extract_bisect_env() { const char* e = getenv("GRB_MI355X_EXTRACT_BISECT"); return e && atoi(e) != 0; }

// `list_in_hbm`: an index list of the call lies in HBM (IdxArg)
bool extract_on_device(GrB_Matrix A, bool others_capable, bool list_in_hbm) {
  const RouteStep s = route_first(route_env("GRB_MI355X_EXTRACT"), device_ok(), others_capable && dev_capable(A) && !mat_bitmap_only(A), list_in_hbm);
  return s == ROUTE_BY_SIZE ? route_by_host_count(A, EXTRACT_DEVICE_MIN_ENTRIES) : s == ROUTE_DEVICE;
}
bool extract_on_device(GrB_Vector u, bool others_capable, bool list_in_hbm) {
  const RouteStep s = route_first(route_env("GRB_MI355X_EXTRACT"), device_ok(), others_capable && dev_capable(u), list_in_hbm);
  if (s != ROUTE_BY_SIZE) return s == ROUTE_DEVICE;
  vec_gate(u);                                                          // deferred work that involves u is completed first, as every reader does
  return route_by_host_count(u, EXTRACT_DEVICE_MIN_ENTRIES);
}

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

namespace grb {

GrB_Info vector_extract_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, const GrB_Descriptor desc) {
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
    write_back(C, w->type->code, T, u->type->code, mask_view(Mm, mask, dv), dv.replace, accum, everywhere);
    store(w, C);
  });
}

GrB_Info col_extract_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, GrB_Index j, const GrB_Descriptor desc) {
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
    write_back(C, w->type->code, T, A->type->code, mask_view(Mm, mask, dv), dv.replace, accum, everywhere);
    store(w, C);
  });
}

GrB_Info matrix_extract_any(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const GrB_Descriptor desc) {
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
    write_back(Cm, C->type->code, T, A->type->code, mask_view(Mm, Mask, dv), dv.replace, accum, everywhere);
    store(C, Cm);
  });
}

}  // namespace grb

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

}  // extern "C"
