// grb_assign_ops.cpp — index-list assign, both routes: C(I,J)<M> = accum(C(I,J), A), the row and column forms, w(I) = u, and a scalar into a region of a
// container that has no HBM layout.
//
//   GrB_Vector_assign, GrB_Row_assign, GrB_Col_assign, GrB_Matrix_assign <- slice assignment (pygraphblas/vector.py:1447-1492, matrix.py:2992-3130)
//   GxB_{Matrix,Vector}_assign_FC32 / _FC64, host_assign_scalar          <- `M[:, :] = 0j`, Matrix.sparse(fill=...), Matrix.iso (matrix.py:154-162, 225-266)
//
// The host route works on the host mirror (grb_hostmap.hpp); the kernels of the device route are in grb_assign.hip (and grb_extract.hip for a line of C), its
// write-back in grb_matrix_ops.cpp / grb_vector_ops.cpp.  The entry points with a list in HBM (GrBX_*_at, GrBX_*_Vector) are in grb_index_ops.cpp.
//
// Route (the rule and the four ASSIGN_*_DEVICE_MIN_ENTRIES: grb_route.hpp): hook GRB_MI355X_ASSIGN; legal when every container of the call has an HBM layout
// (none a bitmap-only batch matrix), the operand is not the output and a mask object accompanies a complemented mask; forced by a list in HBM; by size when C
// lives in HBM only, or C or the operand holds at least the entry point's N entries.  A list that names an index twice is found on the device and handed back to
// the host route (which takes the last occurrence): the `*_device` functions return false for it, before anything was written.
#include "grb_hostmap.hpp"
#include "grb_index_ops.hpp"
#include "grb_assign.hpp"
#include "grb_matops.hpp"

extern "C" {
GrB_Info GrB_Matrix_eWiseAdd_BinaryOp(GrB_Matrix, const GrB_Matrix, const GrB_BinaryOp, const GrB_BinaryOp, const GrB_Matrix, const GrB_Matrix, const GrB_Descriptor);
GrB_Info GrB_Vector_eWiseAdd_BinaryOp(GrB_Vector, const GrB_Vector, const GrB_BinaryOp, const GrB_BinaryOp, const GrB_Vector, const GrB_Vector, const GrB_Descriptor);
}

using namespace grb;
using namespace grb::hostmap;

namespace {

// `operand_entries`: asked only after the hook, the device, the list and the count of C have not decided; C's own count is taken as it is (mat_nvals / entries_known)
template <class F> bool assign_on_device(GrB_Matrix C, bool others_capable, uint64_t min_entries, F&& operand_entries, bool list_in_hbm) {
  const RouteStep s = route_first(route_env("GRB_MI355X_ASSIGN"), device_ok(), others_capable && dev_capable(C) && !mat_bitmap_only(C), list_in_hbm);
  if (s != ROUTE_BY_SIZE) return s == ROUTE_DEVICE;
  return route_by_size(hbm_only(C), true, hbm_only(C) ? 0 : mat_nvals(C), min_entries) || route_by_size(false, true, operand_entries(), min_entries);
}
template <class F> bool assign_on_device(GrB_Vector w, bool others_capable, uint64_t min_entries, F&& operand_entries, bool list_in_hbm) {
  const RouteStep s = route_first(route_env("GRB_MI355X_ASSIGN"), device_ok(), others_capable && dev_capable(w), list_in_hbm);
  if (s != ROUTE_BY_SIZE) return s == ROUTE_DEVICE;
  return route_by_size(hbm_only(w), true, entries_known(w), min_entries) || route_by_size(false, true, operand_entries(), min_entries);
}

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
  DevCSR Z; csr_ewise(ccode, Rest, Rest.val.p, T, tv, B_SECOND, EW_ADD, Z);
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

// the whole-container fast paths forward to eWiseAdd without the caller's descriptor: only when it asks for nothing they would
// drop (a complemented mask without a mask object allows no writes at all; an invalid descriptor is the general path's error)
bool plain_desc(GrB_Descriptor d) { return !d || (check_obj(d) && (d->mask & GrB_COMP) == 0); }

}  // namespace

namespace grb {

GrB_Info vector_assign_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, const GrB_Descriptor desc) {
  const GrB_Index* const I = ia.I;
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  if (I == GrB_ALL && !mask && plain_desc(desc) && accum && check_obj(u) && device_ok() && u->n == w->n) return GrB_Vector_eWiseAdd_BinaryOp(w, nullptr, nullptr, accum, w, u, nullptr);   // w = accum(w, u), in HBM
  return guarded(w, [&] {
    check_v(u, "assign"); if (mask) check_v(mask, "assign");
    const DescView dv(desc);
    vec_gate(w); vec_gate(u);                                            // deferred work that involves them is completed first, as every reader does
    if (u != w && (mask || !dv.mask_comp) && assign_on_device(w, dev_capable(u) && dev_capable(mask), ASSIGN_VEC_DEVICE_MIN_ENTRIES, [&] { return entries_known(u); }, ia.in_hbm()) && assign_vector_device(w, mask, accum, u, ia, dv)) return;
    HostList hl; const auto idx = expand_index_list(hl.get(ia), ia.n, w->n, "assign");
    if (u->n != idx.size() || (mask && mask->n != w->n)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of indices");
    Map C = load(w), U = load(u), Mm; if (mask) Mm = load(mask);
    region_update(C, w->type->code, U, u->type->code, idx, std::vector<uint64_t>{0}, accum, mask_view(Mm, mask, dv), dv.replace,
                  true, false, false, 0);
    store(w, C);
  });
}

GrB_Info matrix_assign_any(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const GrB_Descriptor desc) {
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
    if (A != C && (Mask || !dv.mask_comp) && assign_on_device(C, mat_capable(A) && mat_capable(Mask), ASSIGN_DEVICE_MIN_ENTRIES, [&] { return entries_of(A); }, ia.in_hbm() || ja.in_hbm()) && assign_matrix_device(C, Mask, accum, A, ia, ja, dv)) return;
    HostList hli, hlj; const auto ri = expand_index_list(hli.get(ia), ia.n, C->nrows, "assign"), ci = expand_index_list(hlj.get(ja), ja.n, C->ncols, "assign");
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
    region_update(Cm, C->type->code, Am, A->type->code, ri, ci, accum, mask_view(Mm, Mask, dv), dv.replace, true, false, false, 0);
    store(C, Cm);
  });
}

GrB_Info row_assign_any(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const IdxArg& ja, const GrB_Descriptor desc) {
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
    HostList hl; const auto ci = expand_index_list(hl.get(ja), ja.n, C->ncols, "assign");
    if (u->n != ci.size() || (mask && mask->n != C->ncols)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of column indices");
    Map Cm = load(C, false), U = load(u), Ut, Mm; if (mask) Mm = load(mask);
    for (auto& kv : U) Ut[{0, kv.first.first}] = kv.second;             // the vector as a 1 x nj row
    region_update(Cm, C->type->code, Ut, u->type->code, std::vector<uint64_t>{i}, ci, accum, mask_view(Mm, mask, dv), dv.replace,
                  false, true, false, i);
    store(C, Cm);
  });
}

GrB_Info col_assign_any(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, GrB_Index j, const GrB_Descriptor desc) {
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
    HostList hl; const auto ri = expand_index_list(hl.get(ia), ia.n, C->nrows, "assign");
    if (u->n != ri.size() || (mask && mask->n != C->nrows)) fail(GrB_DIMENSION_MISMATCH, "assign: the vector's size must equal the number of row indices");
    Map Cm = load(C, false), U = load(u), Mm; if (mask) Mm = load(mask);
    region_update(Cm, C->type->code, U, u->type->code, ri, std::vector<uint64_t>{j}, accum, mask_view(Mm, mask, dv), dv.replace,
                  false, false, true, j);
    store(C, Cm);
  });
}

}  // namespace grb

extern "C" {

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
  const auto ri = expand_index_list(I, ni, C->nrows, "assign"), ci = expand_index_list(J, nj, C->ncols, "assign");
  Map Cm = load(C, false), Am, Mm; if (Mask) Mm = load(Mask, false);
  for (size_t a = 0; a < ri.size(); a++) for (size_t b = 0; b < ci.size(); b++) Am[{a, b}] = v;
  region_update(Cm, ccode, Am, xcode, ri, ci, accum, mask_view(Mm, Mask, dv), dv.replace, true, false, false, 0);
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
  const auto idx = expand_index_list(I, ni, w->n, "assign");
  Map C = load(w), U, Mm; if (mask) Mm = load(mask);
  for (size_t a = 0; a < idx.size(); a++) U[{a, 0}] = v;
  region_update(C, wcode, U, xcode, idx, std::vector<uint64_t>{0}, accum, mask_view(Mm, mask, dv), dv.replace, true, false, false, 0);
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
}  // extern "C"
