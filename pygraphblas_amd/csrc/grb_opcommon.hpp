// grb_opcommon.hpp — pieces every GraphBLAS operation driver shares: operator validation, operand
// typecasts into the operator's domain, the operator of an element-wise step (ElemOp), mask -> allow bytes and the
// vector operations' prelude, and the final C<M,replace> = accum(C, T) write-back for vectors.
#pragma once
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_semiring.hpp"
#include "grb_userop.hpp"
#include "grb_possr.hpp"
#include "grb_cmpsr.hpp"
#include "grb_lazy.hpp"
#include <initializer_list>
#include <vector>

namespace grb {

inline void not_implemented(const std::string& what) { fail(GrB_INVALID_VALUE, "not implemented in the MI355X backend: " + what); }

// built-in, same-type binary operator (x, y, z all one real type) or a comparison whose inputs share a type
// (a user-defined operator runs in apply / eWiseAdd / eWiseMult only — grb_userop.cpp; those entry points look for it before they come here)
inline void check_binop(GrB_BinaryOp op, const char* what) {
  if (!check_obj(op)) fail(GrB_UNINITIALIZED_OBJECT, std::string(what) + " operator is not initialised");
  if (is_user(op)) userop_refuse(op->name, what);
  // the multiplier of a positional semiring (an internal object, reached through GxB_Semiring_multiply): it runs inside its semiring in mxm / mxv / vxm only
  if (binop_is_positional(op->opcode)) fail(GrB_DOMAIN_MISMATCH, std::string("positional operator ") + op->name + " cannot be used as " + what + ": it is the multiplier of the positional semirings, which run in mxm, mxv and vxm only");
  if (op->opcode >= B_FIRSTI) not_implemented(std::string("positional / user-defined operator ") + op->name);
  if (op->xtype != op->ytype) not_implemented(std::string("mixed-type operator ") + op->name);
}

// The operator of an element-wise step — GrB_apply, GxB_apply_BinaryOp1st / 2nd — built-in or user-defined alike: what the drivers need of a GrB_UnaryOp, or
// of a GrB_BinaryOp with one operand bound.  mode: 0 unary, 1 z = f(s, x), 2 z = f(x, s) — the numbers of UK_APPLY / UK_BIND1ST / UK_BIND2ND.
struct ElemOp {
  int mode, opcode, xcode, zcode; const char* name; const char* defn;
  bool user() const { return opcode >= (mode == 0 ? (int)U_USER : (int)B_USER); }
};
inline ElemOp elem_op(GrB_UnaryOp op) { return {0, op->opcode, op->xtype->code, op->ztype->code, op->name, op->defn}; }      // (the entry points have checked the handle)
inline ElemOp elem_op(GrB_BinaryOp op, int mode) {
  if (!(check_obj(op) && is_user(op))) check_binop(op, "apply");
  return {mode, op->opcode, op->xtype->code, op->ztype->code, op->name, op->defn};
}
// z(i) = f(x(i)) | f(s, x(i)) | f(x(i), s) over n positions: x and the bound scalar s already in the operator's type, px / q the presence bytes of a bitmap
// (nullptr: every position holds an entry / no presence bytes wanted).  A built-in operator's ahead-of-time kernel, or a user-defined one's compiled kernel.
inline void elem_eval(const ElemOp& op, uint64_t n, const void* x, const uint8_t* px, const void* s, void* z, uint8_t* q) {
  if (op.user()) userop_run(op.mode, op.name, op.defn, op.xcode, n, x, px, nullptr, nullptr, nullptr, s, z, q);
  else vec_apply(op.xcode, n, x, px, op.mode, op.opcode, s, z, q);
}

// ONE rule for NaN under a floating-point MIN / MAX monoid, on every path: the operator is fmin / fmax (a NaN operand is omitted, as in
// SuiteSparse), and an entry all of whose products are NaN is NaN — what a reduction that starts from its first product gives
// (the oracle's rule).  Kernels that start their accumulators from the monoid's identity (push SpMSpV, hash tables, padding lanes
// of wave reductions) get the same answer when that identity is NaN instead of +-inf: fmin(NaN, x) = x, fmin(NaN, NaN) = NaN — NaN
// IS the identity of fmin / fmax.  (Round 2: +-inf there dropped such an entry's NaN on some paths and kept it on others.)
inline bool fp_minmax_identity(int zcode, int addop, uint8_t* identity) {
  if (!(addop == B_MIN || addop == B_MAX)) return false;
  if (zcode == T_FP32) { const float q = std::numeric_limits<float>::quiet_NaN(); memcpy(identity, &q, 4); return true; }
  if (zcode == T_FP64) { const double q = std::numeric_limits<double>::quiet_NaN(); memcpy(identity, &q, 8); return true; }
  return false;
}

inline SemiringDesc make_semiring_desc(GrB_Semiring s, bool swap_mult_args) {
  if (!check_obj(s)) fail(GrB_UNINITIALIZED_OBJECT, "semiring is not initialised");
  check_binop(s->mul, "multiply"); check_binop(s->add->op, "monoid");
  if (s->mul->xtype != s->mul->ztype) not_implemented(std::string("semiring with a comparison multiplier: ") + s->name);
  if (!semiring_op_supported(s->mul->opcode, s->mul->ztype->code)) not_implemented(std::string("semiring multiplier ") + s->mul->name + " (math-library and bit-index operators run only in apply / eWise)");
  if (!semiring_op_supported(s->add->op->opcode, s->add->op->ztype->code)) not_implemented(std::string("semiring monoid ") + s->add->op->name);
  SemiringDesc d{};
  d.zcode = s->add->op->ztype->code; d.addop = s->add->op->opcode; d.mulop = s->mul->opcode; d.flip = false;
  if (swap_mult_args) { int m; if (mirror_binop(d.mulop, &m)) d.mulop = m; else d.flip = true; }
  memcpy(d.identity, s->add->identity, 16); memcpy(d.terminal, s->add->terminal, 16); d.has_terminal = s->add->has_terminal;
  fp_minmax_identity(d.zcode, d.addop, d.identity);
  return d;
}

// An index list argument (I, ni) of extract / assign as explicit 64-bit indices, validated against `dim` BEFORE any
// narrowing: GrB_ALL, an explicit list, or SuiteSparse's GxB_RANGE / GxB_STRIDE / GxB_BACKWARDS encodings of ni
// (I = {begin, end[, stride]}, `end` inclusive).
constexpr uint64_t GXB_RANGE = 0x7FFFFFFFFFFFFFFFull, GXB_STRIDE = GXB_RANGE - 1, GXB_BACKWARDS = GXB_RANGE - 2;
inline std::vector<uint64_t> expand_index_list(const GrB_Index* I, GrB_Index ni, uint64_t dim, const char* what) {
  std::vector<uint64_t> out;
  // an explicit list of positions is only ever built for lists that fit in memory: GrB_ALL or an open-ended range over a
  // hypersparse dimension (2^60) is refused with an error instead of an allocation failure
  constexpr uint64_t LIST_MAX = 1ull << 28;
  auto too_many = [&](uint64_t k) { fail(GrB_INSUFFICIENT_SPACE, std::string(what) + ": an index list of " + std::to_string(k) + " positions (more than 2^28) is not materialised; slice hypersparse containers with explicit indices"); };
  if (I == GrB_ALL) { if (dim > LIST_MAX) too_many(dim); out.resize(dim); for (uint64_t i = 0; i < dim; i++) out[i] = i; return out; }
  if (!I) fail(GrB_NULL_POINTER, std::string(what) + ": index list is NULL");
  auto oob = [&]() { fail(GrB_INDEX_OUT_OF_BOUNDS, std::string(what) + ": index out of bounds"); };
  if (ni == GXB_RANGE || ni == GXB_STRIDE || ni == GXB_BACKWARDS) {
    const uint64_t b = I[0], e = I[1], st = ni == GXB_RANGE ? 1 : I[2];
    if (st == 0) return out;
    { const uint64_t lo = ni == GXB_BACKWARDS ? e : b, hi = ni == GXB_BACKWARDS ? b : e; if (hi >= lo && (hi - lo) / st >= LIST_MAX) too_many((hi - lo) / st + 1); }
    if (ni == GXB_BACKWARDS) { if (b >= dim && b >= e) oob(); for (uint64_t i = b; i + 1 > e; i -= st) { if (i >= dim) oob(); out.push_back(i); if (i < st) break; } }
    else for (uint64_t i = b; i <= e; i += st) { if (i >= dim) oob(); out.push_back(i); }
    return out;
  }
  if (ni > (1ull << 40)) fail(GrB_INVALID_VALUE, std::string(what) + ": index count is not plausible");
  out.assign(I, I + ni);
  for (uint64_t v : out) if (v >= dim) oob();
  return out;
}

// how many positions an index argument names (GrB_ALL, an explicit list, or a GxB_RANGE / GxB_STRIDE / GxB_BACKWARDS triple whose
// `ni` is a sentinel, not a count), without building the list
inline double index_count(const GrB_Index* I, GrB_Index ni, uint64_t dim) {
  if (I == GrB_ALL) return (double)dim;
  if (!I) return 0.0;
  if (ni == GXB_RANGE || ni == GXB_STRIDE || ni == GXB_BACKWARDS) {
    const uint64_t b = I[0], e = I[1], st = ni == GXB_RANGE ? 1 : I[2];
    if (st == 0) return 0.0;
    const uint64_t lo = ni == GXB_BACKWARDS ? e : b, hi0 = ni == GXB_BACKWARDS ? b : e;
    if (hi0 < lo) return 0.0;
    const uint64_t hi = hi0 >= dim && dim ? dim - 1 : hi0;          // (an end beyond the dimension is an error raised later; count what could exist)
    return hi < lo ? 0.0 : (double)((hi - lo) / st + 1);
  }
  return (double)ni;
}

// values of a device array in another type: returns `src` itself when no cast is needed, else fills `tmp`
inline const void* cast_values(int dst_code, int src_code, const void* src, uint64_t n, DevBuf& tmp) {
  if (dst_code == src_code || n == 0) return src;
  tmp.alloc(n * type_size(dst_code));
  vec_cast_values(dst_code, tmp.p, src_code, src, n);
  return tmp.p;
}

// Does any of these containers (nullptr: not given) lack an HBM layout?  `hyper`: a dimension or size beyond the device layout; `cplx`: complex entries.  The two
// flags user_needs_layout / possr_needs_layout take; a scalar's or a thunk's type is the caller's own extra term.
struct NoLayout { bool hyper = false, cplx = false; };
inline void no_layout_of(NoLayout& f, const GrB_Matrix_opaque* A) { if (A) { f.hyper = f.hyper || is_hyper(A); f.cplx = f.cplx || A->type->code >= T_FC32; } }
inline void no_layout_of(NoLayout& f, const GrB_Vector_opaque* v) { if (v) { f.hyper = f.hyper || is_hyper(v); f.cplx = f.cplx || v->type->code >= T_FC32; } }
template <class... C> NoLayout no_layout(const C*... containers) { NoLayout f; (no_layout_of(f, containers), ...); return f; }

// ---- a semiring that does not run through SemiringDesc ----------------------------------------------------------------------------------------------------
// Made once at the top of a product call (semiring_route).  A built-in semiring goes through make_semiring_desc and the SpMV / SpGEMM kernels.  The three off-table
// kinds — user-defined (GrBX_Semiring_new_user, grb_userop.hpp), positional (grb_possr.hpp) and comparison (a built-in semiring whose multiplier is GrB_<cmp>_<T>
// over a non-Boolean T, grb_cmpsr.hpp) — share ONE driver per product (off_table_mxv_like in grb_mxv.cpp,
// off_table_mxm in grb_matrix_ops.cpp): T comes from a small row kernel (mxv / vxm) or "pattern first, values second" (mxm), then the built-in write-back runs;
// such a call is never queued and completes deferred work first, and its accumulator is looked at before the dimensions.  Where the three differ is answered here.
// `product`: 0 mxv, 1 vxm, 2 mxm — the numbers of USK_*, of PK_* and of CK_*.
enum SemiringKind { SR_BUILTIN = 0, SR_USER, SR_POSITIONAL, SR_COMPARE };
static_assert((int)USK_MXV == (int)PK_MXV && (int)USK_VXM == (int)PK_VXM && (int)USK_MXM == (int)PK_MXM, "one numbering of the products");
static_assert((int)CK_MXV == (int)PK_MXV && (int)CK_VXM == (int)PK_VXM && (int)CK_MXM == (int)PK_MXM, "one numbering of the products");
struct SemiringRoute {
  int kind; GrB_Semiring s;
  bool off_table() const { return kind != SR_BUILTIN; }
  int zcode() const { return s->add->op->ztype->code; }      // the type of T (a comparison semiring: BOOL, its monoid's)
  int xcode() const { return s->mul->xtype->code; }          // the type a comparison semiring compares in
  // operand values as the kernels take them: cast into T's type (user-defined) or into the multiplier's argument type (comparison), or none at all (a positional
  // semiring reads no value)
  const void* operand_values(int code, const void* val, uint64_t n, DevBuf& tmp) const {
    return kind == SR_USER ? cast_values(zcode(), code, val, n, tmp) : kind == SR_COMPARE ? cast_values(xcode(), code, val, n, tmp) : nullptr;
  }
  // the head of the plan string: "usersr<add=...,mul=...,type=...,kind=...> " / "possr<...> " / "cmpsr<...> "
  std::string plan(int product) const { return kind == SR_USER ? usersr_plan(product, s->add->op, s->mul) : kind == SR_COMPARE ? cmpsr_plan(product, s) : possr_plan(product, s); }
  // its layout refusal names the semiring and needs initialised operands: the callers hand refuse_before_device their NoLayout
  bool refuses_layout_by_name() const { return kind == SR_POSITIONAL || kind == SR_COMPARE; }
  // Refused before a device is asked for: operators the compiled route cannot run (user-defined); containers without an HBM layout, naming the semiring
  // (positional, comparison — `nl`: nullptr while an operand is not initialised, which is an error of its own) and, for a comparison semiring, a user-defined
  // accumulator (refused by check_binop as everywhere else; `accum` may be nullptr).
  void refuse_before_device(const NoLayout* nl, GrB_BinaryOp accum = nullptr) const {
    if (kind == SR_USER) usersr_check(s->add->op, s->mul);
    if (kind == SR_POSITIONAL && nl) possr_needs_layout(s, nl->hyper, nl->cplx);
    if (kind == SR_COMPARE && nl) cmpsr_needs_layout(s, nl->hyper, nl->cplx);
    if (kind == SR_COMPARE && accum && check_obj(accum) && is_user(accum)) check_binop(accum, "accum");
  }
  // ... and after it, once the operands are known to be initialised: containers without an HBM layout, naming the operator (user-defined; `extent`: "dimension" of
  // a matrix, "dimension or size" where vectors take part)
  void refuse_after_device(const NoLayout& nl, const char* extent) const {
    if (kind == SR_USER) user_needs_layout(usersr_name(s->add->op, s->mul), extent, nl.hyper, nl.cplx);
  }
  // mxv / vxm: t(r) for every allowed row of R (usersr_rows / possr_rows); the plan string ends up as plan(product) + the kernel's name
  void rows(int product, const DevCSR& R, const void* aval, const void* uval, const uint8_t* upres, const uint8_t* allow, void* tval, uint8_t* tpres) const {
    if (kind == SR_USER) usersr_rows(product, s->add->op, s->mul, R, aval, uval, upres, allow, tval, tpres);
    else if (kind == SR_COMPARE) cmpsr_rows(s->add->op->opcode, xcode(), cmp_sel(s->mul->opcode, product), R, aval, uval, upres, allow, (uint8_t*)tval, tpres);
    else possr_rows(s->add->op->opcode, zcode(), pos_coord(s->mul->opcode, product), R, upres, allow, tval, tpres);
  }
  // mxm: the values of a T whose pattern exists (usersr_product_values / possr_product_values); appends the kernel's name to the plan string
  void product_values(const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T) const {
    if (kind == SR_USER) usersr_product_values(s->add->op, s->mul, A, aval, B, bval, T);
    else if (kind == SR_COMPARE) cmpsr_product_values(s->add->op->opcode, xcode(), cmp_sel(s->mul->opcode, CK_MXM), A, aval, B, bval, T);
    else possr_product_values(s->add->op->opcode, zcode(), pos_coord(s->mul->opcode, PK_MXM), A, B, T);
  }
};
// (a handle that is not initialised is nobody's: the built-in route reports it)
inline SemiringRoute semiring_route(GrB_Semiring s) {
  if (!check_obj(s) || !check_obj(s->add)) return {SR_BUILTIN, s};
  if (check_obj(s->mul) && is_positional_semiring(s)) return {SR_POSITIONAL, s};
  // a BUILT-IN semiring over a comparison of a non-Boolean type; the same two objects composed with GrB_Semiring_new stay on the table route ("not implemented")
  if (check_obj(s->mul) && check_obj(s->add->op) && is_compare_semiring(s)) return {SR_COMPARE, s};
  return {is_user_semiring(s) ? SR_USER : SR_BUILTIN, s};
}

// ---- GxB_eWiseUnion: what its matrix and vector entry points share ------------------------------------------------------------------------------------------
// The arguments, before a device is asked for and in this order: all there, all initialised, both scalars hold an entry (as GRB_SCALAR_OK of grb_apply_scalar.cpp).
#define GRB_UNION_ARGS(C, M, op, A, B, alpha, beta) \
  if (!(C) || !(op) || !(A) || !(B) || !(alpha) || !(beta)) return GrB_NULL_POINTER; \
  if (!check_obj(C) || !check_obj(op) || !check_obj(A) || !check_obj(B) || ((M) && !check_obj(M)) || !check_obj(alpha) || !check_obj(beta)) return GrB_UNINITIALIZED_OBJECT; \
  if (!(alpha)->has || !(beta)->has) return GrB_INVALID_VALUE
// ... then, before the dimensions are looked at: no complex container and no complex scalar
inline void union_refuse_complex(const NoLayout& nl, GxB_Scalar alpha, GxB_Scalar beta) {
  if (nl.cplx || alpha->type->code >= T_FC32 || beta->type->code >= T_FC32) fail(GrB_DOMAIN_MISMATCH, "eWiseUnion: complex containers and scalars are out of scope");
}
inline void EwiseMode::cast_fill(int xcode, int ycode, uint8_t* a16, uint8_t* b16) const {
  cast_scalar(xcode, a16, alpha->type->code, alpha->x); cast_scalar(ycode, b16, beta->type->code, beta->x);
}

// mask vector -> allow bytes.  Returns nullptr (= everything allowed) when there is no mask and no
// complement; sets *nothing when there is no mask but the complement flag is set.
inline const uint8_t* vector_allow(GrB_Vector mask, const DescView& dv, uint64_t n, DevBuf& tmp, bool* nothing) {
  *nothing = false;
  if (!mask) { if (dv.mask_comp) *nothing = true; return nullptr; }
  vec_to_device(mask);
  tmp.alloc(n ? n : 1);
  build_allow(n, mask->type->code, mask->dval.p, mask->dpres.as<uint8_t>(), dv.mask_struct, dv.mask_comp, tmp.as<uint8_t>());
  return tmp.as<uint8_t>();
}

// The prelude of a vector operation: w, the operands and the mask all have the size n (GrB_DIMENSION_MISMATCH with the caller's own `msg` otherwise);
// deferred work is completed when `flush` (a user-defined operator is never queued: it runs after everything before it); the mask becomes `allow`.
// True: nothing may be written (no mask + complement) — w has been cleared under replace, and the caller returns.
inline bool vector_prelude(GrB_Vector w, GrB_Vector mask, const DescView& dv, uint64_t n, std::initializer_list<GrB_Vector> operands, const char* msg, bool flush,
                           DevBuf& tmp, const uint8_t*& allow) {
  bool conform = w->n == n && (!mask || mask->n == n);
  for (GrB_Vector u : operands) conform = conform && u->n == n;
  if (!conform) fail(GrB_DIMENSION_MISMATCH, msg);
  if (flush) lazy_flush();
  bool nothing = false;
  allow = vector_allow(mask, dv, n, tmp, &nothing);
  if (nothing && dv.replace) GrB_Vector_clear(w);
  return nothing;
}

// Write T (bitmap tval/tpres of type tcode; buffers are consumed) into w under mask/accum/replace.
// `t_only_allowed`: T has no entries where the mask forbids writing (true for the kernels here).
// `t_nvals`: the entry count of T when the caller knows it (~0 otherwise) — carried into w where the result's count follows
// from it, so that the next product does not have to count on the device and wait for the answer.
inline void vector_write_back(GrB_Vector w, int tcode, DevBuf& tval, DevBuf& tpres, const uint8_t* allow, GrB_BinaryOp accum,
                              bool replace, bool t_only_allowed, uint64_t t_nvals = ~0ull) {
  const uint64_t n = w->n; const int wcode = w->type->code;
  const bool w_empty = w->lazy ? false : (w->host_valid ? (vec_nvals(w) == 0) : (w->facts.dnvals_known && w->facts.dnvals == 0));   // (deferred work pending on w: not known, and not worth completing for this)
  if (accum) check_binop(accum, "accum");
  if (!accum && (!allow || (t_only_allowed && (replace || w_empty)))) {
    // w becomes exactly T: adopt the buffers (typecast the values if the output type differs)
    if (tcode != wcode) { DevBuf c(n * w->type->size + 1); vec_cast_values(wcode, c.p, tcode, tval.p, n); tval = std::move(c); }
    vec_invalidate_host(w, t_nvals, t_nvals != ~0ull);
    w->dval = std::move(tval); w->dpres = std::move(tpres); w->dev_valid = true;
    return;
  }
  vec_to_device(w);
  // no mask + accum: the result is the union of w and T — still full when w or T was
  const bool stays_full = !allow && accum && ((w->facts.dnvals_known && w->facts.dnvals == n) || t_nvals == n);
  // the epilogue runs in the accumulator's domain (or w's type without one)
  const int ecode = accum ? accum->xtype->code : wcode;
  DevBuf tc, wc;
  const void* tv = cast_values(ecode, tcode, tval.p, n, tc);
  void* wv = w->dval.p;
  if (ecode != wcode) { wc.alloc(n * type_size(ecode) + 1); vec_cast_values(ecode, wc.p, wcode, w->dval.p, n); wv = wc.p; }
  vec_epilogue(ecode, n, wv, w->dpres.as<uint8_t>(), tv, tpres.as<uint8_t>(), allow, accum ? accum->opcode : -1, replace);
  if (ecode != wcode) vec_cast_values(wcode, w->dval.p, ecode, wv, n);
  vec_invalidate_host(w, n, stays_full);   // (entries may disappear: the edge bound goes too; temporaries return to the pool, reuse is stream-ordered)
}

}  // namespace grb
