// grb_possr.hpp — the positional semirings GxB_{MIN,MAX,ANY,PLUS,TIMES}_{FIRSTI,FIRSTI1,FIRSTJ,FIRSTJ1,SECONDI,SECONDI1,SECONDJ,SECONDJ1}_{INT32,INT64} in
// mxm / mxv / vxm (kernels and launches: grb_possr.hip; the drivers: off_table_mxm in grb_matrix_ops.cpp and off_table_mxv_like in grb_mxv.cpp, which a
// positional semiring shares with the user-defined ones through a SemiringRoute, grb_opcommon.hpp).
//
// The multiplier ignores the operands' values and yields a coordinate of the product term, cast to the semiring's type (INT32 wraps), + 1 for the ...1 forms.
// With the indices of the operands AFTER the descriptor's transposes:
//                mxm  A(i,k) B(k,j)     mxv  A(i,k) u(k)     vxm  u(k) A(k,j)
//   FIRSTI       i                      i                    0
//   FIRSTJ       k                      k                    k
//   SECONDI      k                      k                    k
//   SECONDJ      j                      0                    j
// (u is an n x 1 column in mxv and u' a 1 x n row in vxm.)  An entry of the result exists iff at least one term exists; the monoid's identity is never combined in.
// The operands may have any real type: their values are never read.  Hypersparse and complex containers are refused, naming the semiring.
// The multipliers are internal objects of the registry (GxB_Semiring_multiply returns them, the printers name them); no binary-operator handle is exported, and
// every other place a binary operator can go refuses them (check_binop, grb_opcommon.hpp).
#pragma once
#include "grb_internal.hpp"

namespace grb {

enum PosSel { PS_ROW = 0, PS_K, PS_COL, PS_ZERO };       // which coordinate of the term (i, k, j) a product is: the kernels' row, the contraction index, T's column, none
enum PosKind { PK_MXV = 0, PK_VXM, PK_MXM };
struct PosCoord { int sel; int plus1; };                 // passed to the kernels by value

inline bool is_positional_semiring(const GrB_Semiring_opaque* s) { return s->mul && binop_is_positional(s->mul->opcode); }

// the multiplier in an operation of `kind`, in the kernels' orientation (mxv / vxm: a row of the kernel's CSR is an output position, its columns are k)
inline PosCoord pos_coord(int mulop, int kind) {
  const int base = (mulop - B_FIRSTI) >> 1, plus1 = (mulop - B_FIRSTI) & 1;      // 0 FIRSTI, 1 FIRSTJ, 2 SECONDI, 3 SECONDJ
  int sel = PS_K;
  if (base == 0) sel = kind == PK_VXM ? PS_ZERO : PS_ROW;
  else if (base == 3) sel = kind == PK_MXV ? PS_ZERO : kind == PK_VXM ? PS_ROW : PS_COL;
  return {sel, plus1};
}

// GrB_DOMAIN_MISMATCH naming the semiring: a hypersparse operand (grb_hyper.cpp relabels indices: the coordinates would be the relabelled ones) or a complex one
void possr_needs_layout(const GrB_Semiring_opaque* s, bool hyper, bool cplx);
// ... and the semiring handed to an operation that takes a semiring for one of its operators (eWiseAdd, eWiseMult, kronecker)
void possr_refuse_elementwise(const GrB_Semiring_opaque* s, const char* where);
// "possr<add=MIN,mul=SECONDI,type=INT64,kind=vxm> "
std::string possr_plan(int kind, const GrB_Semiring_opaque* s);

// t(r) for every row r of R whose allow byte is not 0 (allow == nullptr: every row): the monoid `addop` of type `zcode` (INT32 / INT64) over coord(r, k) of the
// entries (r, k) of R with upres[k] != 0 (upres == nullptr: every k).  A skipped row and a row without a term get presence 0.  Appends to the kernel plan.
void possr_rows(int addop, int zcode, PosCoord c, const DevCSR& R, const uint8_t* upres, const uint8_t* allow, void* tval, uint8_t* tpres);
// T.val (allocated, `zcode`) over T's pattern — that of the ANY_PAIR product of A's and B's patterns or a subset of it, columns ascending in every row.
void possr_product_values(int addop, int zcode, PosCoord c, const DevCSR& A, const DevCSR& B, DevCSR& T);

}  // namespace grb
