// grb_matrix_ops.cpp — GrB_mxm and the matrix operations around it.
//
//   GrB_mxm                 <- lib.GrB_mxm, pygraphblas/matrix.py:2572-2583 (Matrix.mxm)       THE HOT PATH
//   GrB_transpose           <- Matrix.transpose                 (pygraphblas/matrix.py:1003-1062)
//   GrB_Matrix_eWiseAdd/Mult_* <- Matrix.eadd / emult           (pygraphblas/matrix.py:1103-1413)
//   GxB_Matrix_eWiseUnion   <- Matrix.eunion                    (SuiteSparse 6: the union with fill values; not in the reference package)
//   GrB_Matrix_apply, GxB_Matrix_apply_BinaryOp1st/2nd          (pygraphblas/matrix.py:1934-2040)
//   GxB_Matrix_select       <- Matrix.select / tril / triu      (pygraphblas/matrix.py:2042-2200)
//   GrB_Matrix_reduce_Monoid <- Matrix.reduce_vector            (pygraphblas/matrix.py:1861-1932)
//   GrB_Matrix_assign_<T>   <- Matrix.assign_scalar             (pygraphblas/matrix.py:3180-3230)
// Semantics: SURVEY.md Appendix A.  Every operation computes T into a fresh CSR and then performs
// the C<M,replace> = accum(C,T) write-back, so the output may alias any input.
#include "grb_opcommon.hpp"
#include "grb_matops.hpp"
#include "grb_assign_scalar.hpp"
#include "grb_lazy.hpp"
#include "grb_hostmap.hpp"      // kind_name: the plan's word for an index argument
#include "grb_spmm.hpp"
#include "grb_sddmm.hpp"
#include "grb_gemm.hpp"

using namespace grb;

namespace grb {
bool mxm_few_rows_wanted(const DevCSR& Ad, const DevCSR& Bd);
void mxm_few_rows(const DevCSR& Ad, GrB_Type atype, GrB_Matrix Mmask, const DescView& dv, GrB_Semiring semiring, GrB_Matrix B, int zcode, DevCSR& T);
bool few_long_rows(uint64_t nrows, uint64_t ncols, uint64_t nnz);
void ewise_few_rows(GrB_Matrix C, GrB_Matrix Mmask, const DescView& dv, GrB_BinaryOp accum, GrB_BinaryOp op, const DevCSR& Ad, GrB_Type atype, const DevCSR& Bd, GrB_Type btype, const EwiseMode& mode, DevCSR& T);
// round 6: the same batches as bitmaps, all rows in one kernel (grb_mxm_rows.cpp)
bool batch_wanted(GrB_Matrix C, uint64_t work);
void ewise_batch(GrB_Matrix C, GrB_Matrix Mmask, const DescView& dv, GrB_BinaryOp accum, GrB_BinaryOp op, GrB_Matrix A, GrB_Matrix B, const EwiseMode& mode);
void apply_batch(GrB_Matrix C, int mode, int opcode, int xcode, const uint8_t* scalar16, GrB_Matrix A);
bool mxm_batch(GrB_Matrix C, GrB_Matrix A, GrB_Matrix Mmask, const DescView& dv, GrB_BinaryOp accum, GrB_Semiring semiring, GrB_Matrix B, int zcode, DevCSR& T);
}

namespace {

struct CsrView { const DevCSR* m; DevBuf vals; const void* v; };

// device CSR of op(A) with values cast to `code` (or untouched when `need_vals` is false)
const DevCSR& operand(GrB_Matrix A, bool transpose) { mat_to_device(A); return transpose ? mat_csc(A) : A->csr; }

// the dimensions of op(A)
struct Dims { uint64_t r, c; };
Dims op_dims(GrB_Matrix A, bool transpose) { return transpose ? Dims{A->ncols, A->nrows} : Dims{A->nrows, A->ncols}; }
// C and the mask are d.r x d.c, or GrB_DIMENSION_MISMATCH with the caller's own message
void conform(GrB_Matrix C, GrB_Matrix M, Dims d, const char* msg) {
  if (C->nrows != d.r || C->ncols != d.c || (M && (M->nrows != d.r || M->ncols != d.c))) fail(GrB_DIMENSION_MISMATCH, msg);
}
// no mask + complement: nothing may be written (C is cleared under replace), and the caller returns
bool nothing_to_write(GrB_Matrix C, GrB_Matrix M, const DescView& dv) {
  if (M || !dv.mask_comp) return false;
  if (dv.replace) GrB_Matrix_clear(C);
  return true;
}
// T has S's pattern (row pointers and columns copied) and a fresh value array of `val_bytes` (+ 16: the kernels of user-defined operators store whole packs)
DevCSR pattern_copy(const DevCSR& S, size_t val_bytes) {
  DevCSR T; T.nrows = S.nrows; T.ncols = S.ncols; T.nnz = S.nnz;
  T.rowptr.alloc(((size_t)S.nrows + 1) * 4); T.col.alloc(S.nnz * 4 + 4); T.val.alloc(val_bytes + 16);
  GRB_HIP(hipMemcpyAsync(T.rowptr.p, S.rowptr.p, ((size_t)S.nrows + 1) * 4, hipMemcpyDeviceToDevice, stream()));
  if (S.nnz) GRB_HIP(hipMemcpyAsync(T.col.p, S.col.p, S.nnz * 4, hipMemcpyDeviceToDevice, stream()));
  T.valid = true;
  return T;
}

void adopt(GrB_Matrix C, DevCSR& T, int tcode) {
  // C becomes exactly T (cast values if the types differ)
  if (tcode != C->type->code && T.nnz) { DevBuf c(T.nnz * C->type->size); vec_cast_values(C->type->code, c.p, tcode, T.val.p, T.nnz); T.val = std::move(c); }
  C->csr = std::move(T); mat_invalidate_host(C);      // (the old image is freed by the move; what was derived from it, the caches, the host mirror and the edit queue go)
  if (!C->csr.val.p) C->csr.val.alloc(8);
  if (!C->csr.col.p) C->csr.col.alloc(8);
  C->csr.valid = true; C->dev_valid = true; C->host_valid = false;
}

}  // namespace
// C<M,replace> = accum(C, T).  `t_masked`: T already has no entry the mask forbids.  (Declared in grb_extract.hpp: the extract entry points of grb_extract_ops.cpp end in it too.)
void grb::matrix_write_back(GrB_Matrix C, DevCSR& T, int tcode, GrB_Matrix M, const DescView& dv, GrB_BinaryOp accum, bool t_masked) {
  if (accum) check_binop(accum, "accum");
  if (nothing_to_write(C, M, dv)) return;
  const bool c_empty = mat_nvals(C) == 0;
  if (!accum && (!M || (t_masked && (dv.replace || c_empty)))) { adopt(C, T, tcode); return; }
  if (!accum && M && (dv.replace || c_empty)) {
    // filter T by the mask, then adopt
    mat_to_device(M);
    DevBuf keep(T.nnz + 1); DevCSR F;
    mask_flags(T, M->csr, M->type->code, dv.mask_struct, dv.mask_comp, keep.as<uint8_t>());
    csr_compact(T, T.val.p, type_size(tcode), keep.as<uint8_t>(), F);
    adopt(C, F, tcode); return;
  }
  // general three-way merge in the accumulator's domain (or C's type)
  mat_to_device(C); if (M) mat_to_device(M);
  const int ccode = C->type->code, ecode = accum ? accum->xtype->code : ccode;
  DevBuf tc, cc; DevCSR Cv, Tv;     // views with cast values
  const void* tv = cast_values(ecode, tcode, T.val.p, T.nnz, tc);
  const void* cv = cast_values(ecode, ccode, C->csr.val.p, C->csr.nnz, cc);
  // build shallow views that share index arrays: done by temporarily wrapping pointers
  struct Shallow { DevCSR v; ~Shallow() { v.rowptr.p = nullptr; v.col.p = nullptr; v.val.p = nullptr; } } sc, st;
  sc.v.nrows = C->csr.nrows; sc.v.ncols = C->csr.ncols; sc.v.nnz = C->csr.nnz; sc.v.rowptr.p = C->csr.rowptr.p; sc.v.col.p = C->csr.col.p; sc.v.val.p = (void*)cv;
  st.v.nrows = T.nrows; st.v.ncols = T.ncols; st.v.nnz = T.nnz; st.v.rowptr.p = T.rowptr.p; st.v.col.p = T.col.p; st.v.val.p = (void*)tv;
  DevCSR out;
  csr_writeback(ecode, C->csr.nrows, sc.v, st.v, M ? &M->csr : nullptr, M ? M->type->code : 0, dv.mask_struct, dv.mask_comp, dv.replace,
                accum ? accum->opcode : -1, out);
  adopt(C, out, ecode);
}
namespace {

void check_mat(GrB_Matrix A, const char* what) { if (!check_obj(A)) fail(GrB_UNINITIALIZED_OBJECT, std::string(what) + ": uninitialised matrix"); }

void check_mxm_operands(GrB_Matrix M, GrB_Matrix A, GrB_Matrix B) { check_mat(A, "mxm"); check_mat(B, "mxm"); if (M) check_mat(M, "mxm"); }

// ---------------------------------------------------------------------------------------------------------------------
// A semiring that does not run through SemiringDesc — user-defined, positional or comparison (SemiringRoute, grb_opcommon.hpp) — in two steps, one driver for all three.  The
// pattern of T is the pattern of the ANY_PAIR product of the operands' patterns: the built-in routes with a BOOL ANY_PAIR semiring and no values — spgemm_masked
// under a plain mask (its rows are the mask's, in column order), spgemm_hash otherwise (a segmented sort, or the dense path's ordered walk, leaves every row in
// column order).  The route's kernel then fills the values (a user-defined semiring: every entry the left-to-right sum of its products in ascending k, over operand
// values cast into T's type; a positional one: the coordinates' monoid, no operand value read or cast; a comparison one: the BOOL monoid over the comparisons of
// operand values cast into the multiplier's argument type, one byte per entry).  What is refused before a device is asked for was refused by
// the caller; a user-defined semiring's layout refusal comes here, then the accumulator is looked at BEFORE the dimensions; never queued; none of the batch /
// few-rows routes.  The write-back is the built-in semirings' own.  A call that may write nothing (no mask + the complement flag) leaves the plan string empty.
void off_table_mxm(const SemiringRoute& route, GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GrB_Matrix A, GrB_Matrix B, GrB_Descriptor desc) {
  check_mxm_operands(M, A, B);
  route.refuse_after_device(no_layout(C, M, A, B), "dimension");
  if (accum) check_binop(accum, "accum");
  const DescView dv(desc);
  const Dims a = op_dims(A, dv.tran0), b = op_dims(B, dv.tran1);
  if (a.c != b.r) fail(GrB_DIMENSION_MISMATCH, "mxm: dimensions do not conform");
  conform(C, M, {a.r, b.c}, "mxm: dimensions do not conform");
  lazy_flush();
  g_last_plan.clear();
  if (nothing_to_write(C, M, dv)) return;
  const DevCSR& Ad = operand(A, dv.tran0); const DevCSR& Bd = operand(B, dv.tran1);
  SemiringDesc pd{}; pd.zcode = T_BOOL; pd.addop = B_ANY; pd.mulop = B_PAIR;      // (identity false, no terminal value, no flip)
  SpgemmCall call{}; call.A = &Ad; call.B = &Bd;
  DevCSR T; bool t_masked = false;
  if (M && !dv.mask_comp) {
    mat_to_device(M);
    call.M = &M->csr; call.mcode = M->type->code; call.mstruct = dv.mask_struct;
    spgemm_masked(call, pd, T); t_masked = true;
  } else spgemm_hash(call, pd, T);
  const int zc = route.zcode();
  const std::string pattern_plan = g_last_plan;
  g_last_plan = route.plan(PK_MXM);
  T.val.alloc(T.nnz * type_size(zc) + 16);
  DevBuf acast, bcast;
  const void* av = route.operand_values(A->type->code, Ad.val.p, Ad.nnz, acast);
  const void* bv = route.operand_values(B->type->code, Bd.val.p, Bd.nnz, bcast);
  route.product_values(Ad, av, Bd, bv, T);
  g_last_plan += "pattern: " + pattern_plan;
  matrix_write_back(C, T, zc, M, dv, accum, t_masked);
}

// ---- the spmm_full route: op(B) holds every position (judged on the image operand() returned: pending edits applied, the cached transpose of a full matrix is
// full).  GRB_MI355X_FULL (read per call: a test hook, and the yardstick of tools/spmm_probe.py): 0 never, 1 wherever legal.  By itself: no plain mask (the masked
// product computes the wanted entries only), at least two columns, and SPMM_FULL_MIN_PRODUCTS products (grb_route.hpp).
bool spmm_full_wanted(const DevCSR& Ad, const DevCSR& Bd, bool plain_mask) {
  if (!spmm_is_full(Bd.nrows, Bd.ncols, Bd.nnz)) return false;
  const int env = route_env("GRB_MI355X_FULL");
  if (env >= 0) return env == 1;
  return !plain_mask && Bd.ncols >= 2 && Ad.nnz * (uint64_t)Bd.ncols >= SPMM_FULL_MIN_PRODUCTS;
}
// false: T would not fit the 32-bit layout, the call goes on to the route it took before
bool spmm_full_route(const SpgemmCall& call, const SemiringDesc& sd, bool cast, DevCSR& T) {
  SpmmPlan p;
  if (!spmm_full(call, sd, T, p)) return false;
  g_last_plan = "spmm_full<k=" + std::to_string(p.k) + ",group=" + std::to_string(p.group) + ",slabs=" + std::to_string(p.slabs) + ",long=" + std::to_string(p.nlong) + ",cast=" + (cast ? "1" : "0") +
                "> k_spmm_rowflags k_full_pattern " + (p.nlong ? "k_spmm_long_tasks " : "") + (p.group ? "k_spmm_narrow " : "k_spmm_wide ") + (p.nlong ? "k_spmm_fold " : "");
  return true;
}

// ---- the sddmm route: a plain mask over the product of two FULL operands, S<M> = X (+).(x) Y' (attention and edge scores, link-prediction scores, the gradient of
// spmm_full with respect to A's values).  T's pattern is the mask's and every entry is the dot product of two contiguous rows (grb_sddmm.hpp): nnz(M) k products
// where the masked Gustavson route probes the mask's hash table m k n times.  GRB_MI355X_SDDMM (read per call: a test hook, and the yardstick of
// tools/sddmm_probe.py): 0 never, 1 wherever legal.  By itself: from SDDMM_MIN_WORK = m k n (grb_route.hpp).  Fullness is judged on the operands' OWN images with
// pending edits applied (a full matrix transposed is full), before any transpose is asked for: the kernel reads op(A) and op(B)' row-major, so a `desc = T1` call
// reads B's own image and never builds its transpose.
bool sddmm_wanted(uint64_t m, uint64_t k, uint64_t n) {
  const int env = route_env("GRB_MI355X_SDDMM");
  if (env >= 0) return env == 1;
  return sddmm_by_default(m, k, n, SDDMM_MIN_WORK);
}
bool sddmm_operand_full(GrB_Matrix A) {
  if (!dev_capable(A)) return false;
  mat_to_device(A);
  return spmm_is_full(A->csr.nrows, A->csr.ncols, A->csr.nnz);
}
// T = the product at every entry of M's pattern.  A structural mask has then been applied (t_masked); a valued one is left to the write-back's filter: T keeps the
// false entries, the filter drops them, and the result is the masked route's.
void sddmm_route(GrB_Matrix M, GrB_Matrix A, GrB_Matrix B, const DescView& dv, const SemiringDesc& sd, DevBuf& xcast, DevBuf& ycast, DevCSR& T) {
  const DevCSR& X = operand(A, dv.tran0); const DevCSR& Y = operand(B, !dv.tran1);      // op(A), m x k, and op(B)', n x k: both row-major value arrays
  mat_to_device(M);
  const bool uses_x = binop_uses_x(sd.mulop), uses_y = binop_uses_y(sd.mulop);
  const void* xv = uses_x ? cast_values(sd.zcode, A->type->code, X.val.p, X.nnz, xcast) : nullptr;
  const void* yv = uses_y ? cast_values(sd.zcode, B->type->code, Y.val.p, Y.nnz, ycast) : nullptr;
  const bool cast = (uses_x && A->type->code != sd.zcode) || (uses_y && B->type->code != sd.zcode);
  SddmmPlan p;
  sddmm_full(M->csr, xv, yv, X.ncols, sd, T, p);
  g_last_plan = "sddmm<k=" + std::to_string(p.k) + ",group=" + std::to_string(p.group) + ",entries=" + std::to_string(p.entries) + ",cast=" + (cast ? "1" : "0") + "> " + (p.entries ? "k_sddmm " : "");
}

// ---- the gemm_full route: op(A) AND op(B) hold every position (judged like the sddmm route's operands: on their own images, before any transpose is asked for) —
// the dense update H W of a GNN layer, a Gram matrix X X', all-pairs MIN_PLUS on a dense block.  T is full too: a closed-form pattern and one register-tiled
// kernel that stages both operands in LDS and reads a transposed operand where it lies (grb_gemm.hpp); any mask is applied by the write-back.  GRB_MI355X_GEMM
// (read per call: a test hook, and the yardstick of tools/gemm_probe.py): 0 never, 1 wherever legal, a plain mask included (the sddmm route then stands back).
// By itself: exactly the calls spmm_full took when its left operand happened to be full — no plain mask, at least two columns, GEMM_FULL_MIN_WORK = m k n
// (grb_route.hpp) — and none while GRB_MI355X_FULL is set: that hook keeps its meaning.
bool gemm_full_wanted(int env, uint64_t m, uint64_t k, uint64_t n, bool plain_mask) {
  if (env >= 0) return env == 1;
  if (route_env("GRB_MI355X_FULL") >= 0) return false;
  return gemm_by_default(m, k, n, plain_mask, GEMM_FULL_MIN_WORK);
}
void gemm_full_route(GrB_Matrix A, GrB_Matrix B, uint64_t m, uint64_t n, uint64_t k, const DescView& dv, const SemiringDesc& sd, DevBuf& acast, DevBuf& bcast, DevCSR& T) {
  const bool uses_a = binop_uses_x(sd.mulop), uses_b = binop_uses_y(sd.mulop);
  const void* av = uses_a ? cast_values(sd.zcode, A->type->code, A->csr.val.p, A->csr.nnz, acast) : nullptr;
  const void* bv = uses_b ? cast_values(sd.zcode, B->type->code, B->csr.val.p, B->csr.nnz, bcast) : nullptr;
  const bool cast = (uses_a && A->type->code != sd.zcode) || (uses_b && B->type->code != sd.zcode);
  GemmPlan p;
  gemm_full((uint32_t)m, (uint32_t)n, (uint32_t)k, av, dv.tran0, bv, dv.tran1, sd, T, p);
  g_last_plan = "gemm_full<m=" + std::to_string(p.m) + ",n=" + std::to_string(p.n) + ",k=" + std::to_string(p.k) + ",tile=" + std::to_string(p.tm) + "x" + std::to_string(p.tn) +
                ",layout=" + (p.ta ? "T" : "N") + (p.tb ? "T" : "N") + ",cast=" + (cast ? "1" : "0") + "> k_full_pattern k_gemm_full ";
}

void do_mxm(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GrB_Semiring semiring, GrB_Matrix A, GrB_Matrix B, GrB_Descriptor desc) {
  const SemiringRoute route = semiring_route(semiring);
  if (route.refuses_layout_by_name()) {      // (its layout refusal needs initialised operands, and comes before a device is asked for)
    check_mxm_operands(M, A, B);
    const NoLayout nl = no_layout(C, M, A, B);
    route.refuse_before_device(&nl, accum);
  } else route.refuse_before_device(nullptr);
  need_device();
  if (route.off_table()) { off_table_mxm(route, C, M, accum, A, B, desc); return; }
  if (is_hyper(C) || is_hyper(M) || is_hyper(A) || is_hyper(B)) { hyper_mxm(C, M, accum, semiring, A, B, desc); return; }   // dimensions beyond the device layouts
  check_mxm_operands(M, A, B);
  const DescView dv(desc);
  const Dims a = op_dims(A, dv.tran0), b = op_dims(B, dv.tran1);
  if (a.c != b.r) fail(GrB_DIMENSION_MISMATCH, "mxm: dimensions do not conform");
  conform(C, M, {a.r, b.c}, "mxm: dimensions do not conform");
  SemiringDesc sd = make_semiring_desc(semiring, false);
  g_last_plan.clear();
  if (nothing_to_write(C, M, dv)) return;
  // a batch of a few very long rows times a large matrix (the BC sweeps' frontier products): the rows of the batch's BITMAP through GrB_vxm, the result a bitmap
  if (!dv.tran0 && mat_batch_shape(A->nrows, A->ncols, A->type->code) && mat_batch_shape(C->nrows, C->ncols, C->type->code) && (!M || mat_batch_shape(M->nrows, M->ncols, M->type->code)) &&
      !is_hyper(B) && A != B && M != B) {
    const DevCSR& Bd0 = operand(B, false);
    const char* e = getenv("GRB_MI355X_BATCH");
    if (e ? atoi(e) != 0 : (Bd0.nnz >= (1u << 20) && Bd0.ncols >= 65536u)) {
      if (accum) check_binop(accum, "accum");
      DevCSR T;
      if (mxm_batch(C, A, M, dv, accum, semiring, B, sd.zcode, T)) return;
      matrix_write_back(C, T, sd.zcode, M, dv, accum, true); return;
    }
  }
  DevBuf acast, bcast;
  if (a.c >= 1 && sddmm_operand_full(A) && sddmm_operand_full(B)) {
    // two full operands: the routes in front decline first (they look at op(A)'s and op(B)'s shape and count only, known without a transpose)
    DevCSR ah, bh; ah.nrows = (uint32_t)a.r; ah.ncols = (uint32_t)a.c; ah.nnz = A->csr.nnz; bh.nrows = (uint32_t)b.r; bh.ncols = (uint32_t)b.c; bh.nnz = B->csr.nnz;
    if (!mxm_few_rows_wanted(ah, bh)) {
      const bool plain_mask = M && !dv.mask_comp;
      const int gemm_env = route_env("GRB_MI355X_GEMM");
      if (plain_mask && gemm_env != 1 && dev_capable(M) && !spmm_full_wanted(ah, bh, true) && sddmm_wanted(a.r, a.c, b.c)) {
        DevCSR T; sddmm_route(M, A, B, dv, sd, acast, bcast, T);
        matrix_write_back(C, T, sd.zcode, M, dv, accum, dv.mask_struct); return;
      }
      if (gemm_full_wanted(gemm_env, a.r, a.c, b.c, plain_mask) && !spmm_overflows(a.r, b.c)) {      // (T beyond the 32-bit layout: on to the route the call took before)
        DevCSR T; gemm_full_route(A, B, a.r, b.c, a.c, dv, sd, acast, bcast, T);
        matrix_write_back(C, T, sd.zcode, M, dv, accum, false); return;
      }
    }
  }
  const DevCSR& Ad = operand(A, dv.tran0); const DevCSR& Bd = operand(B, dv.tran1);
  const bool uses_a = binop_uses_x(sd.mulop), uses_b = binop_uses_y(sd.mulop);
  SpgemmCall call{};
  call.A = &Ad; call.B = &Bd;
  call.aval = uses_a ? cast_values(sd.zcode, A->type->code, Ad.val.p, Ad.nnz, acast) : nullptr;
  call.bval = uses_b ? cast_values(sd.zcode, B->type->code, Bd.val.p, Bd.nnz, bcast) : nullptr;
  DevCSR T; bool t_masked = false;
  {
    const bool fp = sd.zcode == T_FP32 || sd.zcode == T_FP64;
    call.ordered = fp && sd.addop != B_MIN && sd.addop != B_MAX && (deterministic_env() || dv.axb == GxB_AxB_GUSTAVSON);      // (MIN / MAX: the same bits in any order)
  }
  if (mxm_few_rows_wanted(Ad, Bd)) {            // a handful of output rows (batched BC frontiers): one vxm per row, see grb_mxm_rows.cpp
    mxm_few_rows(Ad, A->type, M, dv, semiring, B, sd.zcode, T); t_masked = true;
  } else if (spmm_full_wanted(Ad, Bd, M && !dv.mask_comp) && spmm_full_route(call, sd, (uses_a && A->type->code != sd.zcode) || (uses_b && B->type->code != sd.zcode), T)) {
    // a full right operand (feature propagation, k seeds at once): T's pattern is known in advance, one pass (grb_spmm.hpp); a plain mask is applied by the write-back
  } else if (M && !dv.mask_comp) {
    mat_to_device(M);
    call.M = &M->csr; call.mcode = M->type->code; call.mstruct = dv.mask_struct;
    spgemm_masked(call, sd, T); t_masked = true;
  } else {
    // no mask, or a complemented one (applied by the write-back): the two-pass LDS-hash Gustavson; expand / sort / compress on
    // request (it forms floating-point sums in a fixed order): GRB_MI355X_SPGEMM=esc or the descriptor's AxB method GxB_AxB_DOT
    // Deterministic mode (round 5): GRB_MI355X_DETERMINISTIC=1 or the descriptor's GxB_AxB_GUSTAVSON — the two-pass product with its dense path's ordered
    // walk (floating-point sums bit-reproducible from run to run at ~1.15 x the time, grb_spgemm_hash.hpp); results too wide for that path (> 2^20 columns)
    // take expand / sort / compress.  Integer / Boolean monoids are exact in any order: nothing changes for them.
    const char* e = getenv("GRB_MI355X_SPGEMM");
    if ((e && !strcmp(e, "esc")) || dv.axb == GxB_AxB_DOT || (call.ordered && Bd.ncols > (1u << 20))) spgemm_esc(call, sd, T); else spgemm_hash(call, sd, T);
  }
  matrix_write_back(C, T, sd.zcode, M, dv, accum, t_masked);
}

void do_transpose(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GrB_Matrix A, GrB_Descriptor desc) {
  need_device(); check_mat(A, "transpose"); if (M) check_mat(M, "transpose");
  const DescView dv(desc);
  // desc.INP0 = TRAN transposes the input first: the result is then A itself
  const bool tr = !dv.tran0;
  conform(C, M, op_dims(A, tr), "transpose: dimensions do not conform");
  const DevCSR& S = operand(A, tr);
  const size_t ts = A->type->size;
  DevCSR T = pattern_copy(S, S.nnz * ts);
  if (S.nnz) GRB_HIP(hipMemcpyAsync(T.val.p, S.val.p, S.nnz * ts, hipMemcpyDeviceToDevice, stream()));
  matrix_write_back(C, T, A->type->code, M, dv, accum, false);
}

// eWiseAdd / eWiseMult.  A user-defined operator (grb_userop.cpp) has no HBM-less route — hypersparse and complex containers are refused, naming it — and no
// batch routes: the merge of the two patterns moves both operands' values to the output's positions (csr_ewise_aligned) and its compiled kernel streams over
// them, where a built-in operator's csr_ewise merges and computes in one pass.
// GxB_eWiseUnion (mode.fills()) takes every route of eWiseAdd with its two scalars beside the operator: the fill kernels call the operator where eWiseAdd copies.
// Its plan string names it: "ewise_union<on=matrix,op=...> k_merge_fill<union> ", or "union" inside the batch routes' and the user operator's own strings.
void do_ewise(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GrB_BinaryOp op, GrB_Matrix A, GrB_Matrix B, GrB_Descriptor desc, const EwiseMode& mode) {
  need_device(); check_mat(A, "eWise"); check_mat(B, "eWise"); if (M) check_mat(M, "eWise");
  const bool user = check_obj(op) && is_user(op);
  if (user) {
    const NoLayout nl = no_layout(C, M, A, B);
    user_needs_layout(op->name, "dimension", nl.hyper, nl.cplx);
    if (accum) check_binop(accum, "accum");
  } else {
    check_binop(op, "eWise");
    if (is_hyper(C) || is_hyper(M) || is_hyper(A) || is_hyper(B)) { hyper_mat_ewise(C, M, accum, op, A, B, desc, mode); return; }
  }
  const DescView dv(desc);
  const Dims a = op_dims(A, dv.tran0), b = op_dims(B, dv.tran1);
  if (a.r != b.r || a.c != b.c) fail(GrB_DIMENSION_MISMATCH, "eWise: dimensions do not conform");
  conform(C, M, a, "eWise: dimensions do not conform");
  if (mode.fills()) g_last_plan.clear();
  if (nothing_to_write(C, M, dv)) return;
  if (!user && !dv.tran0 && !dv.tran1 && batch_wanted(C, mat_nvals(A) + mat_nvals(B)) && A->type->code < T_FC32 && B->type->code < T_FC32 && (!M || M->type->code < T_FC32)) {
    if (accum) check_binop(accum, "accum");
    ewise_batch(C, M, dv, accum, op, A, B, mode); return;      // a batch of a few very long rows (BC sweeps): its bitmap as ONE vector through the vector kernel
  }
  const DevCSR& Ad = operand(A, dv.tran0); const DevCSR& Bd = operand(B, dv.tran1);
  if (!user && few_long_rows(C->nrows, C->ncols, Ad.nnz + Bd.nnz)) {          // a batch of a few very long rows (BC sweeps): row by row through the vector kernels
    DevCSR T; ewise_few_rows(C, M, dv, accum, op, Ad, A->type, Bd, B->type, mode, T);
    adopt(C, T, C->type->code); return;
  }
  const int xc = op->xtype->code;
  uint8_t alpha[16] = {0}, beta[16] = {0}; if (mode.fills()) mode.cast_fill(xc, op->ytype->code, alpha, beta);
  DevBuf acast, bcast;
  const void* av = cast_values(xc, A->type->code, Ad.val.p, Ad.nnz, acast);
  const void* bv = cast_values(xc, B->type->code, Bd.val.p, Bd.nnz, bcast);
  DevCSR T;
  if (user) {
    DevBuf xv, yv, both;
    csr_ewise_aligned(xc, Ad, av, Bd, bv, mode.kind, T, xv, yv, both, alpha, beta);
    // (a union: the aligned values are (a, beta) / (alpha, b) where one operand alone has the entry — the compiled kernel calls the operator on every entry)
    if (mode.fills()) userop_run(UK_EUNION, op->name, op->defn, xc, T.nnz, xv.p, nullptr, yv.p, nullptr, nullptr, alpha, T.val.p, nullptr, beta);
    else userop_run(mode.whole() ? UK_EADD : UK_EMULT, op->name, op->defn, xc, T.nnz, xv.p, nullptr, yv.p, nullptr, mode.whole() ? both.as<uint8_t>() : nullptr, nullptr, T.val.p, nullptr);
  } else {
    csr_ewise(xc, Ad, av, Bd, bv, op->opcode, mode.kind, T, alpha, beta);
    if (mode.fills()) g_last_plan = std::string("ewise_union<on=matrix,op=") + op->name + "> k_merge_fill<union> ";
  }
  matrix_write_back(C, T, xc, M, dv, accum, false);
}

// apply, and apply with a bound scalar (the ElemOp's mode).  A user-defined operator is refused on containers without an HBM layout and has its accumulator
// looked at first; the positional operators and the bitmap batch route exist for built-in operators only.
void do_apply(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, const ElemOp& op, const void* scalar, int scode, GrB_Matrix A, GrB_Descriptor desc) {
  need_device(); check_mat(A, "apply"); if (M) check_mat(M, "apply");
  if (op.user()) {
    const NoLayout nl = no_layout(C, M, A);
    user_needs_layout(op.name, "dimension", nl.hyper, nl.cplx || scode >= T_FC32);
    if (accum) check_binop(accum, "accum");
  }
  const DescView dv(desc);
  conform(C, M, op_dims(A, dv.tran0), "apply: dimensions do not conform");
  const bool positional = !op.user() && op.mode == 0 && op.opcode >= U_POSITIONI && op.opcode <= U_POSITIONJ1;
  if ((op.user() || positional) && nothing_to_write(C, M, dv)) return;      // (every other built-in operator: the write-back finds it, after the accumulator)
  if (positional) {      // T has op(A)'s pattern, the values are the entries' row / column indices in the operator's type
    const DevCSR& S = operand(A, dv.tran0);
    DevCSR T = pattern_copy(S, S.nnz * type_size(op.xcode));
    csr_position_values(op.xcode, S, op.opcode - U_POSITIONI, T.val.p);
    matrix_write_back(C, T, op.xcode, M, dv, accum, false);
    return;
  }
  uint8_t s[16] = {0}; if (scalar) cast_scalar(op.xcode, s, scode, scalar);
  if (!op.user() && !M && !accum && !dv.mask_comp && !dv.tran0 && A->bm.valid && !A->host_valid && batch_wanted(C, mat_nvals(A)) && A->type->code < T_FC32) {      // a batch that lives as a bitmap stays one
    apply_batch(C, op.mode, op.opcode, op.xcode, s, A); return;
  }
  const DevCSR& S = operand(A, dv.tran0);
  DevCSR T = pattern_copy(S, S.nnz * type_size(op.xcode));
  DevBuf ac; const void* av = cast_values(op.xcode, A->type->code, S.val.p, S.nnz, ac);
  elem_eval(op, S.nnz, av, nullptr, s, T.val.p, nullptr);
  matrix_write_back(C, T, op.xcode, M, dv, accum, false);
}

// select: the keep bytes over op(A)'s entries, then the compaction (T keeps A's own values and type) and the write-back.  A built-in operator makes the keep bytes
// from the positions or the values; a user-defined one with its compiled kernel, over the entries' row indices expanded and the values cast into the operator's
// type FOR THE PREDICATE ONLY — it is refused on containers without an HBM layout, has its accumulator looked at first and is never queued.
void do_select(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GxB_SelectOp op, GrB_Matrix A, GxB_Scalar thunk, GrB_Descriptor desc) {
  need_device(); check_mat(A, "select"); if (M) check_mat(M, "select");
  if (!check_obj(op)) fail(GrB_UNINITIALIZED_OBJECT, "select: operator");
  const bool user = is_user(op), has_thunk = thunk && check_obj(thunk) && thunk->has;
  if (user) {
    const NoLayout nl = no_layout(C, M, A);
    user_needs_layout(op->name, "dimension", nl.hyper, nl.cplx || (has_thunk && thunk->type->code >= T_FC32));
    if (accum) check_binop(accum, "accum");
  }
  const DescView dv(desc);
  conform(C, M, op_dims(A, dv.tran0), "select: dimensions do not conform");
  if (user) { lazy_flush(); if (nothing_to_write(C, M, dv)) return; }
  const DevCSR& S = operand(A, dv.tran0);           // (a transposed input: i and j are those of the transposed matrix)
  const int acode = A->type->code;
  DevBuf keep(S.nnz + 16); DevCSR T;
  int64_t k = 0; uint8_t th[16] = {0};      // the thunk as a diagonal, and in the type it is compared in (no thunk, or an empty one: zero)
  if (user) {
    const int xc = op->xtype->code, kc = op->ttype->code;
    DevBuf rowidx(S.nnz * 4 + 16), xcast;
    csr_row_indices(S, rowidx.as<uint32_t>());
    const void* xv = cast_values(xc, acode, S.val.p, S.nnz, xcast);
    if (has_thunk) cast_scalar(kc, th, thunk->type->code, thunk->x);
    userselect_run(op->name, op->defn, xc, kc, false, S.nnz, rowidx.as<uint32_t>(), S.col.as<uint32_t>(), xv, nullptr, th, keep.as<uint8_t>());
  } else {
    if (has_thunk) { cast_scalar(T_INT64, &k, thunk->type->code, thunk->x); cast_scalar(acode, th, thunk->type->code, thunk->x); }
    if (op->opcode <= SEL_OFFDIAG) select_positional_flags(S, op->opcode, k, keep.as<uint8_t>());
    else select_value_flags(acode, S.nnz, S.val.p, nullptr, op->opcode, th, keep.as<uint8_t>());
  }
  csr_compact(S, S.val.p, A->type->size, keep.as<uint8_t>(), T);
  matrix_write_back(C, T, acode, M, dv, accum, false);
}

void do_reduce_vector(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Monoid monoid, GrB_Matrix A, GrB_Descriptor desc) {
  if (check_obj(monoid) && check_obj(monoid->op) && is_user_monoid(monoid)) usersr_check(monoid->op, nullptr);      // (refused before a device is asked for)
  need_device(); check_mat(A, "reduce");
  if (!check_obj(monoid)) fail(GrB_UNINITIALIZED_OBJECT, "reduce: monoid");
  if (mask && !check_obj(mask)) fail(GrB_UNINITIALIZED_OBJECT, "reduce: mask");
  if (check_obj(monoid->op) && is_user_monoid(monoid)) {
    // a user-defined monoid (GrBX_Monoid_new_user): the row kernel of grb_usersr.cpp with the matrix value as the product; refused on containers without an HBM
    // layout, the accumulator looked at before the dimensions, never queued
    const NoLayout nl = no_layout(A, w, mask);
    user_needs_layout(monoid->op->name, "dimension or size", nl.hyper, nl.cplx);
    if (accum) check_binop(accum, "accum");
    const DescView udv(desc);
    const uint64_t ur = op_dims(A, udv.tran0).r;
    DevBuf uallow_buf; const uint8_t* uallow;
    if (vector_prelude(w, mask, udv, ur, {}, "reduce: dimensions do not conform", true, uallow_buf, uallow)) return;
    vec_gate(w);
    const int uc = monoid->op->ztype->code;
    const DevCSR& S = operand(A, udv.tran0);
    DevBuf ac, tval(ur * type_size(uc) + 16), tpres(ur + 16);
    const void* av = cast_values(uc, A->type->code, S.val.p, S.nnz, ac);
    usersr_rows(USK_REDUCE_ROWS, monoid->op, nullptr, S, av, nullptr, nullptr, nullptr, tval.p, tpres.as<uint8_t>());
    vector_write_back(w, uc, tval, tpres, uallow, accum, udv.replace, false);
    return;
  }
  check_binop(monoid->op, "monoid");
  const DescView dv(desc);
  const uint64_t r = op_dims(A, dv.tran0).r;
  DevBuf allow_buf; const uint8_t* allow;
  if (vector_prelude(w, mask, dv, r, {}, "reduce: dimensions do not conform", false, allow_buf, allow)) return;
  const int mc = monoid->op->ztype->code;
  DevBuf ac, tval(r * type_size(mc) + 8), tpres(r + 1);
  // the columns of a large matrix whose transpose is not at hand (desc T0 on a by-row matrix): no transpose is built for this, every
  // entry combines into its column's accumulator.  (Small matrices keep the row-wise reduction of the transpose: its fixed order
  // is what the reference's docstring values were computed with.)
  bool done = false;
  if (dv.tran0) {
    mat_to_device(A);
    // (only where the order the entries land in cannot show: integer / Boolean monoids and MIN / MAX.  A floating-point PLUS or TIMES keeps
    //  ONE fixed-order algorithm — the row reduction of the transpose — whatever the cache holds: the same call must not return different
    //  bits depending on whether an earlier operation happened to build the transpose)
    const int rop = monoid->op->opcode;
    const bool order_free = !(mc == T_FP32 || mc == T_FP64) || rop == B_MIN || rop == B_MAX || rop == B_ANY;
    // (taken WHETHER OR NOT a cached transpose exists: its row reduction adds in another order, and the same call must not return other bits because an
    //  earlier product happened to build the transpose)
    if (A->csr.nnz >= (1u << 20) && !order_free && A->csr.nrows <= 64) {      // a few long rows (a batch of the BC sweeps): row after row, no atomics, fixed order
      const void* av = cast_values(mc, A->type->code, A->csr.val.p, A->csr.nnz, ac);
      done = csr_reduce_cols_few_rows(mc, A->csr, av, rop, tval.p, tpres.as<uint8_t>());
    }
    if (!done && !A->csc.valid && A->csr.nnz >= (1u << 20) && order_free) {
      const void* av = cast_values(mc, A->type->code, A->csr.val.p, A->csr.nnz, ac);
      uint8_t id[16]; memcpy(id, monoid->identity, 16);
      fp_minmax_identity(mc, monoid->op->opcode, id);          // FP MIN / MAX start from NaN = from the column's first value (the one NaN rule, grb_opcommon.hpp)
      done = csr_reduce_cols(mc, A->csr, av, monoid->op->opcode, id, tval.p, tpres.as<uint8_t>());
    }
  }
  if (!done) {
    const DevCSR& S = operand(A, dv.tran0);
    const void* av = cast_values(mc, A->type->code, S.val.p, S.nnz, ac);
    csr_reduce_rows(mc, S, av, monoid->op->opcode, tval.p, tpres.as<uint8_t>());
  }
  vector_write_back(w, mc, tval, tpres, allow, accum, dv.replace, false);
}

// ---- C<M>(I,J) = accum(C(I,J), x): a T that holds the scalar wherever the write-back may read it, then assign semantics ----------------------------
// The device routes (grb_assign_scalar.hip) build T in HBM from the index arguments as they are — GrB_ALL and ranges never expanded, explicit lists uploaded once
// and inverted by assign_inverse:
//   mask=pattern       a mask object without GrB_COMP: T = M's true entries inside I x J.  The write-back reads T only where M allows a write, so this T and the
//                      full block give the same C — at O(nnz(M) + nnz(C)) whatever |I| |J| is, and with no limit on the region.
//   mask=none | comp   T = all of I x J in closed form; |I| |J| <= SCALAR_REGION_MAX as ever.
// A list that names an index twice, a list over more than ASSIGN_TABLE_MAX_DIM positions, a complex valued mask and GRB_MI355X_ASSIGN_SCALAR=0 (read per
// call: a test hook, and the yardstick of tools/assign_scalar_probe.py) keep the host-built block below.  There is no size threshold: measured from 1e2 positions
// up, the device block never loses to the host-built one by more than the spread between runs.
// the write-back of every route: assign keeps the entries of C outside the region, and inside it T's replace C's — that is accum = SECOND on the union of
// the patterns when the caller gave no accumulator
void scalar_write_back(GrB_Matrix C, DevCSR& T, GrB_Matrix M, const DescView& dv, GrB_BinaryOp accum, bool t_masked) {
  GrB_BinaryOp_opaque second{GRB_MAGIC, B_SECOND, C->type, C->type, C->type, "assign_second", nullptr};
  matrix_write_back(C, T, C->type->code, M, dv, accum ? accum : &second, t_masked);
}

// false: nothing was written and the caller takes the host-built block (which raises the same errors in the same order)
bool assign_scalar_device(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, const DescView& dv) {
  const char* e = getenv("GRB_MI355X_ASSIGN_SCALAR");
  if (e && *e && atoi(e) == 0) return false;
  const bool pattern = M && !dv.mask_comp;
  if (pattern && !dv.mask_struct && M->type->code >= T_FC32) return false;
  ExIdx ri, ci; extract_parse(ri, I, ni, C->nrows, "assign (rows)"); extract_parse(ci, J, nj, C->ncols, "assign (columns)");
  if (!pattern && !scalar_region_fits(ri.n, ci.n)) fail(GrB_OUT_OF_MEMORY, "assign: region too large");
  DevBuf keep_i, keep_j, inv_i, inv_j; extract_upload(ri, keep_i); extract_upload(ci, keep_j);
  if (!assign_inverse(ri, C->nrows, inv_i) || !assign_inverse(ci, C->ncols, inv_j)) return false;
  const int ccode = C->type->code; const size_t ts = C->type->size;
  uint8_t s[16]; cast_scalar(ccode, s, xcode, x);
  DevCSR T;
  if (pattern) { mat_to_device(M); scalar_from_mask(M->csr, M->type->code, dv.mask_struct, ri, inv_i, ci, inv_j, s, ts, T); }      // (M may be C itself: T is complete before the write-back starts)
  else scalar_block((uint32_t)C->nrows, (uint32_t)C->ncols, ri, inv_i, ci, inv_j, s, ts, T);
  g_last_plan = std::string("assign_scalar<rows=") + hostmap::kind_name(ri) + ",cols=" + hostmap::kind_name(ci) + ",mask=" + (pattern ? "pattern" : dv.mask_comp ? "comp" : "none") + ",accum=" + (accum ? accum->name : "none") + "> " +
                (pattern ? "k_assign_scalar_flags csr_compact k_assign_scalar_fill<values> " : "k_assign_scalar_rowflag k_assign_scalar_rowptr k_assign_scalar_fill<block> ") + "entries=" + std::to_string(T.nnz) + " ";
  scalar_write_back(C, T, M, dv, accum, pattern);
  return true;
}

void do_assign_scalar(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, GrB_Descriptor desc) {
  // no HBM layout for this container (hypersparse dimensions, or complex entries): bookkeeping on the host mirror
  if (C->nrows > GRB_DIM_DEVICE_MAX || C->ncols > GRB_DIM_DEVICE_MAX || C->type->code >= T_FC32) { host_assign_scalar(C, M, accum, x, xcode, I, ni, J, nj, desc); return; }
  need_device(); if (M) check_mat(M, "assign");
  const DescView dv(desc);
  conform(C, M, {C->nrows, C->ncols}, "assign: mask dimensions");
  if (I == GrB_ALL && J == GrB_ALL && !M && !accum && !dv.mask_comp && C->nrows * C->ncols <= 0xFFFFFFF0ull && C->nrows * C->ncols > 0) {
    // every position of C: the full one-valued matrix, written by one kernel (`Matrix.dense`, `M[:, :] = x`)
    uint8_t s0[16]; cast_scalar(C->type->code, s0, xcode, x);
    DevCSR T; csr_dense_fill((uint32_t)C->nrows, (uint32_t)C->ncols, s0, C->type->size, T);
    adopt(C, T, C->type->code);
    return;
  }
  if (assign_scalar_device(C, M, accum, x, xcode, I, ni, J, nj, dv)) return;
  // ---- the host-built block: the fallback, and the yardstick ----
  // (indices are validated as 64-bit values before they are narrowed to the device layout's 32 bits)
  const std::vector<uint64_t> rows64 = expand_index_list(I, ni, C->nrows, "assign (rows)"), cols64 = expand_index_list(J, nj, C->ncols, "assign (columns)");
  std::vector<uint32_t> rows(rows64.begin(), rows64.end()), cols(cols64.begin(), cols64.end());
  std::sort(cols.begin(), cols.end()); cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
  std::vector<uint8_t> inrow(C->nrows ? C->nrows : 1, 0); for (auto r : rows) inrow[r] = 1;
  uint64_t nsel = 0; for (uint64_t i = 0; i < C->nrows; i++) nsel += inrow[i];
  if (nsel * cols.size() > 0xFFFFFFF0ull) fail(GrB_OUT_OF_MEMORY, "assign: region too large");
  // the scalar block T (host-built CSR, uploaded)
  const int ccode = C->type->code; const size_t ts = C->type->size;
  uint8_t s[16]; cast_scalar(ccode, s, xcode, x);
  std::vector<uint32_t> rp(C->nrows + 1, 0), cc; std::vector<uint8_t> vv;
  cc.reserve(nsel * cols.size()); vv.reserve(nsel * cols.size() * ts);
  for (uint64_t i = 0; i < C->nrows; i++) {
    if (inrow[i]) { cc.insert(cc.end(), cols.begin(), cols.end()); for (size_t q = 0; q < cols.size(); q++) vv.insert(vv.end(), s, s + ts); }
    rp[i + 1] = (uint32_t)cc.size();
  }
  DevCSR T; T.nrows = (uint32_t)C->nrows; T.ncols = (uint32_t)C->ncols; T.nnz = cc.size();
  T.rowptr.alloc(rp.size() * 4); T.col.alloc(cc.size() * 4 + 4); T.val.alloc(vv.size() + 8);
  GRB_HIP(hipMemcpyAsync(T.rowptr.p, rp.data(), rp.size() * 4, hipMemcpyHostToDevice, stream()));
  if (!cc.empty()) { GRB_HIP(hipMemcpyAsync(T.col.p, cc.data(), cc.size() * 4, hipMemcpyHostToDevice, stream()));
                     GRB_HIP(hipMemcpyAsync(T.val.p, vv.data(), vv.size(), hipMemcpyHostToDevice, stream())); }
  GRB_HIP(hipStreamSynchronize(stream())); T.valid = true;
  scalar_write_back(C, T, M, dv, accum, false);
}

}  // namespace

#define MAT_GUARD(C) if (!(C)) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT

extern "C" {

GrB_Info GrB_mxm(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Semiring semiring, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!A || !B || !semiring) return GrB_NULL_POINTER;
  return guarded(C, [&] { do_mxm(C, Mask, accum, semiring, A, B, desc); });
}
GrB_Info GrB_transpose(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!A) return GrB_NULL_POINTER; return guarded(C, [&] { do_transpose(C, Mask, accum, A, desc); });
}
GrB_Info GrB_Matrix_eWiseAdd_BinaryOp(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A || !B) return GrB_NULL_POINTER; return guarded(C, [&] { do_ewise(C, M, accum, op, A, B, desc, {EW_ADD}); }); }
GrB_Info GrB_Matrix_eWiseAdd_Monoid(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A || !B) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT; return guarded(C, [&] { do_ewise(C, M, accum, op->op, A, B, desc, {EW_ADD}); }); }
GrB_Info GrB_Matrix_eWiseAdd_Semiring(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A || !B) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT; return guarded(C, [&] { possr_refuse_elementwise(op, "eWiseAdd"); do_ewise(C, M, accum, op->add->op, A, B, desc, {EW_ADD}); }); }
GrB_Info GrB_Matrix_eWiseMult_BinaryOp(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A || !B) return GrB_NULL_POINTER; return guarded(C, [&] { do_ewise(C, M, accum, op, A, B, desc, {EW_MULT}); }); }
GrB_Info GrB_Matrix_eWiseMult_Monoid(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A || !B) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT; return guarded(C, [&] { do_ewise(C, M, accum, op->op, A, B, desc, {EW_MULT}); }); }
GrB_Info GrB_Matrix_eWiseMult_Semiring(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A || !B) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT; return guarded(C, [&] { possr_refuse_elementwise(op, "eWiseMult"); do_ewise(C, M, accum, op->mul, A, B, desc, {EW_MULT}); }); }
GrB_Info GxB_Matrix_eWiseUnion(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GxB_Scalar alpha, const GrB_Matrix B, const GxB_Scalar beta,
                               const GrB_Descriptor desc) {
  GRB_UNION_ARGS(C, M, op, A, B, alpha, beta);
  return guarded(C, [&] { union_refuse_complex(no_layout(C, M, A, B), alpha, beta); do_ewise(C, M, accum, op, A, B, desc, {EW_UNION, alpha, beta}); });
}
GrB_Info GrB_Matrix_apply(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_UnaryOp op, const GrB_Matrix A, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A) return GrB_NULL_POINTER; if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] { do_apply(C, M, accum, elem_op(op), nullptr, 0, A, desc); });
}
GrB_Info GxB_Matrix_select(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GxB_SelectOp op, const GrB_Matrix A, const GxB_Scalar thunk, const GrB_Descriptor desc) {
  MAT_GUARD(C); if (!op || !A) return GrB_NULL_POINTER; return guarded(C, [&] { do_select(C, M, accum, op, A, thunk, desc); });
}
GrB_Info GrB_Matrix_reduce_Monoid(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Monoid monoid, const GrB_Matrix A, const GrB_Descriptor desc) {
  if (!w || !A || !monoid) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] { do_reduce_vector(w, mask, accum, monoid, A, desc); });
}

#define GRB_TYPED_MATOPS(SUF, CT, CODE) \
  GrB_Info GrB_Matrix_assign_##SUF(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, CT x, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, const GrB_Descriptor desc) { \
    MAT_GUARD(C); return guarded(C, [&] { do_assign_scalar(C, M, accum, &x, CODE, I, ni, J, nj, desc); }); } \
  GrB_Info GxB_Matrix_apply_BinaryOp1st_##SUF(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, CT x, const GrB_Matrix A, const GrB_Descriptor desc) { \
    MAT_GUARD(C); if (!op || !A) return GrB_NULL_POINTER; return guarded(C, [&] { do_apply(C, M, accum, elem_op(op, 1), &x, CODE, A, desc); }); } \
  GrB_Info GxB_Matrix_apply_BinaryOp2nd_##SUF(GrB_Matrix C, const GrB_Matrix M, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, CT y, const GrB_Descriptor desc) { \
    MAT_GUARD(C); if (!op || !A) return GrB_NULL_POINTER; return guarded(C, [&] { do_apply(C, M, accum, elem_op(op, 2), &y, CODE, A, desc); }); }
GRB_TYPED_MATOPS(BOOL, bool, T_BOOL) GRB_TYPED_MATOPS(INT8, int8_t, T_INT8) GRB_TYPED_MATOPS(UINT8, uint8_t, T_UINT8)
GRB_TYPED_MATOPS(INT16, int16_t, T_INT16) GRB_TYPED_MATOPS(UINT16, uint16_t, T_UINT16) GRB_TYPED_MATOPS(INT32, int32_t, T_INT32)
GRB_TYPED_MATOPS(UINT32, uint32_t, T_UINT32) GRB_TYPED_MATOPS(INT64, int64_t, T_INT64) GRB_TYPED_MATOPS(UINT64, uint64_t, T_UINT64)
GRB_TYPED_MATOPS(FP32, float, T_FP32) GRB_TYPED_MATOPS(FP64, double, T_FP64)

}  // extern "C"
