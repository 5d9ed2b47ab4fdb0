// grb_cmpsr.hpp — the comparison semirings GxB_{LOR,LAND,LXOR,EQ,ANY}_{EQ,NE,GT,LT,GE,LE}_{INT8..UINT64,FP32,FP64} in mxm / mxv / vxm (kernels and launches:
// grb_cmpsr.hip; the drivers: off_table_mxm in grb_matrix_ops.cpp and off_table_mxv_like in grb_mxv.cpp, shared with the user-defined and the positional
// semirings through a SemiringRoute, grb_opcommon.hpp).
//
// The multiplier is the built-in comparison GrB_<cmp>_<T>: T x T -> BOOL; the monoid is a BOOL one.  Both operands are cast into T (the C cast of every
// write-back), the terms are compared in T — NaN compares false except under NE, -0.0 == 0.0, unsigned values compare as unsigned — and T, the product, is BOOL:
// one byte per entry.  mxv and mxm call cmp(A(i,k), B(k,j)); vxm calls cmp(u(k), A(k,j)) on the rows of the CSR of A', so its kernel gets GT <-> LT and
// GE <-> LE mirrored (cmp_sel) — a kernel argument, never a flip of values.  An entry of the result exists iff at least one term exists; the monoid's identity
// is never combined in.  Only the BUILT-IN handles take this route: a semiring composed with GrB_Semiring_new from the same two objects keeps the operator
// table's "not implemented".  Hypersparse and complex containers are refused, naming the semiring.
#pragma once
#include "grb_internal.hpp"

namespace grb {

enum CmpKind { CK_MXV = 0, CK_VXM, CK_MXM };      // the numbers of PK_* / USK_*
// A comparison as three bits over the outcomes of one ordered pair — (a == b, a < b, a > b), all false when an operand is NaN — and a final negation:
// EQ {1,0,0,0}  NE {1,0,0,1}  LT {0,1,0,0}  GT {0,0,1,0}  LE {1,1,0,0}  GE {1,0,1,0}.  Passed to the kernels by value.
struct CmpSel { uint32_t eq, lt, gt, inv; };

inline bool is_compare_semiring(const GrB_Semiring_opaque* s) { return s->builtin && s->mul && s->add && s->add->op && s->mul->xtype != s->mul->ztype; }

// the multiplier `mulop` (B_EQ .. B_LE) in an operation of `kind`, in the kernels' orientation cmp(matrix value, operand value): vxm swaps the roles of < and >
CmpSel cmp_sel(int mulop, int kind);
// GrB_DOMAIN_MISMATCH naming the semiring: a hypersparse or a complex container
void cmpsr_needs_layout(const GrB_Semiring_opaque* s, bool hyper, bool cplx);
// "cmpsr<add=LOR,mul=EQ,type=INT64,kind=mxv> "
std::string cmpsr_plan(int kind, const GrB_Semiring_opaque* s);

// t(r) for every row r of R whose allow byte is not 0 (allow == nullptr: every row): the BOOL monoid `addop` (B_LOR, B_LAND, B_LXOR, B_LXNOR, B_ANY) over
// cmp(aval[p], uval[k]) of the entries p = (r, k) of R with upres[k] != 0 (upres == nullptr: every k); aval (R.nnz values) and uval in the type `xcode`.  uval[k]
// is not read where upres[k] == 0.  A skipped row and a row without a term get presence 0.  Appends to the kernel plan.
void cmpsr_rows(int addop, int xcode, CmpSel c, const DevCSR& R, const void* aval, const void* uval, const uint8_t* upres, const uint8_t* allow, uint8_t* tval, uint8_t* tpres);
// T.val (allocated, one byte per entry) over T's pattern — that of the ANY_PAIR product of A's and B's patterns or a subset of it, columns ascending in every row.
void cmpsr_product_values(int addop, int xcode, CmpSel c, const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T);

}  // namespace grb
