// grb_userop.hpp — user-defined unary / binary / select operators handed over as C source (GxB_UnaryOp_new / GxB_BinaryOp_new / GxB_SelectOp_new) and compiled for the device (grb_userop.cpp).
#pragma once
#include "grb_internal.hpp"

namespace grb {

enum UserKind { UK_APPLY = 0, UK_BIND1ST, UK_BIND2ND, UK_EADD, UK_EMULT };

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
//   scalar       the bound operand of UK_BIND1ST / UK_BIND2ND, already in tcode
//   z / q        result values and (when not nullptr) result presence bytes
// Throws GrbError when hipRTC is missing or the definition does not compile (the message carries the operator's name and the compiler's log).
void userop_run(int kind, const char* name, const char* defn, int tcode, uint64_t n, const void* x, const uint8_t* px, const void* y, const uint8_t* py,
                const uint8_t* both, const void* scalar, void* z, uint8_t* q);

// keep[p] = present(p) && NAME(i, j, &x[p], &thunk) over n entries with the select operator's compiled kernel (`name`, `defn`, value type xcode, thunk type
// tcode); sets the kernel plan.
//   rowidx / col entries' row and column indices of a matrix (on_vector: ignored — i is the position p, j is 0)
//   x            the entries' values, already in xcode
//   pres         presence bytes of a bitmap, nullptr = every position holds an entry
//   thunk        the thunk, already in tcode
// Throws like userop_run.
void userselect_run(const char* name, const char* defn, int xcode, int tcode, bool on_vector, uint64_t n, const uint32_t* rowidx, const uint32_t* col, const void* x,
                    const uint8_t* pres, const void* thunk, uint8_t* keep);

}  // namespace grb
