// grb_gemv.hpp — host interface of a FULL matrix times a vector (grb_gemv.hip; the integer geometry is grb_gemv_geom.hpp): t = M (+).(x) u for M = A or A', A full —
// nnz == rows cols, so its value array IS the row-major dense array — and u a bitmap vector with or without holes.  Both layouts read A's own image: no transpose
// of a full matrix is built, no SpMV plan, no column word is read.  t has an entry at every position when u holds at least one entry, and none otherwise.  One
// more producer of (tval, tpres) for the write-back of GrB_mxv / GrB_vxm (grb_mxv.cpp, the `gemv_full` route).
//
// THE ORDER GUARANTEE: the fold order of an output is a function of the inner length k, the layout, the value size and u's pattern ALONE — not of the output's
// position, the outer length, the grid, the alignment of A's rows or the run; no atomics.  Absent u(l) contribute nothing and every fold starts from its first
// existing product.
//   N, k <= 64   lane g holds product g; p_g = p_g (+) p_(g + s) for s = G / 2 ... 1, G = pow2ceil(k), among the lanes that hold a product.
//   N, k > 64    per chunk of GEMV_N_CHUNK: lane g folds its packets (V = min(16 / size, 4) consecutive l each) g, g + 64, ... left to right, then the butterfly over 64
//                lanes; the chunks in ascending order.
//   T            per chunk of gemv_t_chunk(k) rows: four consecutive pieces each folded in ascending l, then the pieces in ascending order; the chunks in
//                ascending order.
// The oracle's plain left-to-right order: N for k <= 2, T for k <= gemv_t_piece(k) + 1 (64 rows up to k = 65 536).
#pragma once
#include "grb_matops.hpp"
#include "grb_gemv_geom.hpp"

namespace grb {

// what the route reports in the plan string
struct GemvPlan { uint64_t m = 0, k = 0, chunks = 0; int layout = GEMV_N; bool holes = false; const char* kernel = ""; };

// t(o) = (+)_l M(o, l) (x) u(l) for o < m: layout GEMV_N reads aval as m x k row-major, GEMV_T as k x m.  aval / uval: values already in the semiring's type,
// nullptr when the multiplier ignores that side (nothing is loaded from it); upres: u's presence bytes, nullptr when every position holds an entry — otherwise at
// least one byte is set (the caller has counted).  tval: m values; every one is written.
void gemv_full(int layout, uint64_t m, uint64_t k, const void* aval, const void* uval, const uint8_t* upres, const SemiringDesc& d, void* tval, GemvPlan& plan);

// ---- between the driver (grb_gemv.hip) and the kernels (grb_gemv_kernels.hpp, one instantiation per value type: grb_gemv_inst.hip) ----
struct GemvValuesCall { int layout; uint64_t m, k, chunks; const void* aval; const void* uval; const uint8_t* upres; void* tval; void* part; uint8_t* flag; };
template <class T> void run_gemv_values(const GemvValuesCall& c, const SemiringDesc& d);

}  // namespace grb
