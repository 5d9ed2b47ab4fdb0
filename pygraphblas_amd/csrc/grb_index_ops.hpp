// grb_index_ops.hpp — the seven index-list operations, each once for both kinds of list: GrB_<name> passes a host list (or GrB_ALL, or a range triple),
// GrBX_<name>_at with location 1 and the GrBX_*_Vector entry points (grb_index_ops.cpp) pass a list that lies in HBM (IdxArg, grb_extract.hpp).
// Defined in grb_extract_ops.cpp and grb_assign_ops.cpp.
#pragma once
#include "grb_extract.hpp"

namespace grb {

GrB_Info vector_extract_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, const GrB_Descriptor desc);
GrB_Info col_extract_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, GrB_Index j, const GrB_Descriptor desc);
GrB_Info matrix_extract_any(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const GrB_Descriptor desc);
GrB_Info vector_assign_any(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, const GrB_Descriptor desc);
GrB_Info matrix_assign_any(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const IdxArg& ia, const IdxArg& ja, const GrB_Descriptor desc);
GrB_Info row_assign_any(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const IdxArg& ja, const GrB_Descriptor desc);
GrB_Info col_assign_any(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const IdxArg& ia, GrB_Index j, const GrB_Descriptor desc);

}  // namespace grb
