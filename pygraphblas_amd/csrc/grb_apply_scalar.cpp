// grb_apply_scalar.cpp — apply with the bound operand in a GxB_Scalar: forwarded to the typed entry point of the scalar's type.
//
//   GxB_{Matrix,Vector}_apply_BinaryOp1st/2nd                   <- apply_first / apply_second with a Scalar (pygraphblas/matrix.py:1999-2004, 2034-2039)
//
// No kernels and no route of its own: the typed entry points are in grb_matrix_ops.cpp / grb_vector_ops.cpp.
#include "grb_api.hpp"
#include <string.h>

using namespace grb;

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
}  // extern "C"
