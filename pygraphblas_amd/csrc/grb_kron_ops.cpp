// grb_kron_ops.cpp — the Kronecker product, both routes.
//
//   GrB_Matrix_kronecker_BinaryOp / _Monoid / _Semiring, GxB_kron <- Matrix.kronecker, Matrix.kronpow (pygraphblas/matrix.py:2739-2805, 1732-1757)
//
// The host route works on the host mirror (grb_hostmap.hpp: one map insertion per product entry); the kernels of the device route are in grb_kron.hip — a
// product of two 8 000-entry matrices is 6.4e7 entries, one streaming store pass in HBM, out of reach for the map-based host route.
//
// Route (the rule and KRON_DEVICE_MIN_ENTRIES: grb_route.hpp): hook GRB_MI355X_KRON; legal when C, both operands and the mask have an HBM layout (mat_capable)
// and, kronecker's own, neither operand is the output, a mask object accompanies a complemented mask and the product fits the 32-bit device layout (ar br and
// ac bc follow from C's own shape; nnz(A) nnz(B) <= KRON_MAX_ENTRIES); by size when C or an operand lives in HBM only, or on nnz(A) nnz(B).  The 3 x 3
// docstring examples keep the host route.
// GRB_MI355X_KRON_TIME=1 puts HIP events around the fill kernel; GrBX_kron_fill_ms returns what they measured (tools/kron_probe.py).
#include "grb_hostmap.hpp"
#include "grb_kron.hpp"
#include "grb_matops.hpp"

using namespace grb;
using namespace grb::hostmap;

namespace {

thread_local float g_kron_fill_ms = 0.0f;

bool kron_on_device(GrB_Matrix C, GrB_Matrix Mask, GrB_Matrix A, GrB_Matrix B, const DescView& dv) {
  const RouteStep s = route_first(route_env("GRB_MI355X_KRON"), device_ok(), mat_capable(C) && mat_capable(A) && mat_capable(B) && mat_capable(Mask), false);
  if (s == ROUTE_HOST) return false;
  if (A == C || B == C || (!Mask && dv.mask_comp)) return false;
  if (C->nrows > GRB_DIM_DEVICE_MAX || C->ncols > GRB_DIM_DEVICE_MAX) return false;
  const uint64_t na = entries_of(A), nb = entries_of(B);
  if (na > KRON_MAX_ENTRIES || nb > KRON_MAX_ENTRIES || na * nb > KRON_MAX_ENTRIES) return false;      // (each factor < 2^32: the product cannot wrap)
  return s == ROUTE_DEVICE || route_by_size(hbm_only(C) || hbm_only(A) || hbm_only(B), true, na * nb, KRON_DEVICE_MIN_ENTRIES);
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

extern "C" {

GrB_Info GrB_Matrix_kronecker_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
  if (!C || !A || !B || !op) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_m(A, "kronecker"); check_m(B, "kronecker"); if (Mask) check_m(Mask, "kronecker"); check_binop(op, "kronecker");
    const DescView dv(desc);
    const uint64_t ar = dv.tran0 ? A->ncols : A->nrows, ac = dv.tran0 ? A->nrows : A->ncols, br = dv.tran1 ? B->ncols : B->nrows, bc = dv.tran1 ? B->nrows : B->ncols;
    if (C->nrows != ar * br || C->ncols != ac * bc || (Mask && (Mask->nrows != C->nrows || Mask->ncols != C->ncols))) fail(GrB_DIMENSION_MISMATCH, "kronecker: dimensions do not conform");
    if (kron_on_device(C, Mask, A, B, dv)) { kron_device(C, Mask, accum, op, A, B, dv); return; }
    Map Am = load(A, dv.tran0), Bm = load(B, dv.tran1), T, Cm = load(C, false), Mm; if (Mask) Mm = load(Mask, false);
    const int oc = op->xtype->code;
    for (auto& a : Am) for (auto& b : Bm) {
      Val x = cast(oc, A->type->code, a.second), y = cast(oc, B->type->code, b.second), z{};
      dispatch_type(oc, [&]<class T>() { T p, q; memcpy(&p, x.data(), sizeof(T)); memcpy(&q, y.data(), sizeof(T)); T r = apply_binop<T>(op->opcode, p, q); memcpy(z.data(), &r, sizeof(T)); });
      T[{a.first.first * br + b.first.first, a.first.second * bc + b.first.second}] = z;
    }
    write_back(Cm, C->type->code, T, oc, mask_view(Mm, Mask, dv), dv.replace, accum, everywhere);
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

}  // extern "C"
