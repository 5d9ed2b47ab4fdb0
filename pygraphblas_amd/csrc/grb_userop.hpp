// grb_userop.hpp — user-defined unary / binary / select operators handed over as C source (GxB_UnaryOp_new / GxB_BinaryOp_new / GxB_SelectOp_new) and compiled for the device (grb_userop.cpp).
#pragma once
#include "grb_internal.hpp"

namespace grb {

enum UserKind { UK_APPLY = 0, UK_BIND1ST, UK_BIND2ND, UK_EADD, UK_EMULT, UK_EUNION };

inline bool is_user(const GrB_BinaryOp_opaque* op) { return op->opcode >= B_USER; }
inline bool is_user(const GrB_UnaryOp_opaque* op) { return op->opcode >= U_USER; }
inline bool is_user(const GxB_SelectOp_opaque* op) { return op->opcode >= SEL_USER; }

// GrB_DOMAIN_MISMATCH: the operator `opname` cannot be used as `where` (an accumulator, a monoid, a multiplier, ...)
[[noreturn]] void userop_refuse(const char* opname, const char* where);
// A user-defined operator runs on containers with an HBM layout only: GrB_DOMAIN_MISMATCH naming the operator for a hypersparse container (`extent`: what of
// it is beyond the device layout — "dimension" of a matrix, "size" of a vector) or a complex one.
void user_needs_layout(const char* opname, const char* extent, bool hyper, bool cplx);

// Evaluate the operator (`name`, `defn`, all of its types `tcode`) over n positions with its compiled kernel; sets the kernel plan.
//   x / y        operand values of type tcode (y: nullptr for UK_APPLY / UK_BIND*)
//   px / py      presence bytes of a bitmap operand, nullptr = every position holds an entry
//   both         UK_EADD over aligned CSR values: 1 where both operands have the entry (else the value in x is copied); nullptr: decided by px / py
//   scalar       the bound operand of UK_BIND1ST / UK_BIND2ND, already in tcode; UK_EUNION: alpha, what stands in for x where only y has the entry
//   scalar2      UK_EUNION: beta, what stands in for y where only x has the entry (px == py == nullptr, aligned CSR values: neither is ever used)
//   z / q        result values and (when not nullptr) result presence bytes
// Throws GrbError when hipRTC is missing or the definition does not compile (the message carries the operator's name and the compiler's log).
void userop_run(int kind, const char* name, const char* defn, int tcode, uint64_t n, const void* x, const uint8_t* px, const void* y, const uint8_t* py,
                const uint8_t* both, const void* scalar, void* z, uint8_t* q, const void* scalar2 = nullptr);

// keep[p] = present(p) && NAME(i, j, &x[p], &thunk) over n entries with the select operator's compiled kernel (`name`, `defn`, value type xcode, thunk type
// tcode); sets the kernel plan.
//   rowidx / col entries' row and column indices of a matrix (on_vector: ignored — i is the position p, j is 0)
//   x            the entries' values, already in xcode
//   pres         presence bytes of a bitmap, nullptr = every position holds an entry
//   thunk        the thunk, already in tcode
// Throws like userop_run.
void userselect_run(const char* name, const char* defn, int xcode, int tcode, bool on_vector, uint64_t n, const uint32_t* rowidx, const uint32_t* col, const void* x,
                    const uint8_t* pres, const void* thunk, uint8_t* keep);

// ---- what the kernels of user-defined semirings (grb_usersr.cpp) share with the ones above: one table of compiled texts, one set of counters ----
// The compiled kernel `entry` of the text `src` (code objects on disk: `prefix`-<hash>.co) for the operator(s) `name`: compiled at first use outside the table's
// lock, a second process reads the code object.  Throws GrbError (GrB_PANIC without hipRTC, GrB_INVALID_VALUE with the compiler's log).
hipFunction_t userop_kernel_of(const std::string& src, const char* name, const char* entry, const char* prefix);
const char* userop_c_type(int code);      // the C type of a real built-in type, nullptr for every other
const char* userop_prelude();             // what a definition may assume (the fixed-width integer names, INFINITY, NAN)
void userop_count_launch();               // GrBX_userop_stats' `launched`

}  // namespace grb

// ---- user-defined monoids and semirings (GrBX_Monoid_new_user / GrBX_Semiring_new_user, grb_usersr.cpp) ----------------------------------------------------
// A monoid or semiring made by those two entry points: its operators are user-defined or built-ins the generated text can express, its types ONE real built-in
// type.  Every such object — also one made of built-ins only, and a semiring over such a monoid — takes this route.  It runs in mxm / mxv / vxm (the off-table
// drivers off_table_mxm / off_table_mxv_like, through a SemiringRoute: grb_opcommon.hpp) and the matrix-to-vector reduction (a block of do_reduce_vector)
// through two compiled kernels:
//   rows      t(r) = (+)_p mul(a(p), u(col(p))) over the CSR rows of one operand (mxv, vxm), or (+)_p a(p) (reduce_rows): a wave per row
//   product   the values of T = A (+).(x) B on a pattern that is already there: a wave per row of T
// The monoid's identity is never combined into a result (an entry starts from its first product), and the multiplier's argument order is a constant of the text.
namespace grb {

enum UserSrKind { USK_MXV = 0, USK_VXM, USK_MXM, USK_REDUCE_ROWS };

inline bool is_user_monoid(const GrB_Monoid_opaque* m) { return m->op && (m->usersr || is_user(m->op)); }
inline bool is_user_semiring(const GrB_Semiring_opaque* s) { return s->add && s->mul && (s->usersr || s->add->usersr || is_user(s->mul) || (s->add->op && is_user(s->add->op))); }
// the name a refusal or a plan string speaks of: the user-defined one of the two operators (the monoid's when both are)
inline const char* usersr_name(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul) { return is_user(add) || !mul ? add->name : mul->name; }

// Can these operators run on the compiled route?  Each is user-defined or a built-in the text expresses, all types are one real built-in type (mul: nullptr for
// a reduction).  GrB_DOMAIN_MISMATCH naming the operator otherwise — a GrB_Semiring_new semiring over a GrBX_Monoid_new_user monoid may carry any built-in
// multiplier, and it is refused here, at the top of the drivers, before a device is asked for and before anything is written.
void usersr_check(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul);

// t(r) for every row r of R whose allow byte is not 0 (allow == nullptr: every row); sets the kernel plan.  aval / uval: already in the semiring's type.
//   kind       USK_MXV: mul(a, u); USK_VXM: mul(u, a); USK_REDUCE_ROWS: the product is a itself (mul, uval, upres unused)
//   upres      presence bytes of u, nullptr = every position holds an entry
//   tval/tpres one value and one presence byte per row; a skipped row gets presence 0
void usersr_rows(int kind, const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul, const DevCSR& R, const void* aval, const void* uval, const uint8_t* upres,
                 const uint8_t* allow, void* tval, uint8_t* tpres);
// T.val (allocated, the semiring's type) over T's pattern — that of the ANY_PAIR product of A's and B's patterns, or a subset of it (a product whose column is not
// in T's row is dropped): every entry the left-to-right sum of its products in ascending k.  Appends to the kernel plan.
void usersr_product_values(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul, const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T);
// "usersr<add=...,mul=...,type=...,kind=...> "
std::string usersr_plan(int kind, const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul);

}  // namespace grb
