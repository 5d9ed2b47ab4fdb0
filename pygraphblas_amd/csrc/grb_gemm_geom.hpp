// grb_gemm_geom.hpp — the integer side of the product of two FULL matrices (grb_gemm.hpp, the gemm_full route of GrB_mxm): the constants of the kernel's shape
// and the integer functions host code and the kernel share.  Plain integers only — no HIP types, no containers — so that a stand-alone program can check it
// under the sanitizers (tests/gemm_geometry_check.cpp).  Every function is constexpr: host code and the kernel call the same text.
//
// THE SHAPE (T(i, j) = (+)_l op(A)(i, l) (x) op(B)(l, j); op(A) m x k and op(B) k x n full; T m x n full and row-major)
//   tile     a TM x TN block of T.  Two shapes: wide, GEMM_TM_WIDE x GEMM_TN_WIDE, for n > GEMM_TALL_MAX_N, and tall, GEMM_TM_TALL x GEMM_TN_TALL, for narrower
//            results (a classifier layer's width): both hold GEMM_WAVES * 64 register blocks of GEMM_RM x GEMM_RN outputs, one per thread.  Tiles are numbered
//            row-major — tile t covers rows gemm_tile_i0(t, n) ... and columns gemm_tile_j0(t, n) ... — and a workgroup of GEMM_WAVES waves takes tiles blockIdx,
//            blockIdx + grid, ... (a grid capped at GEMM_GRID_CAP workgroups).
//   k steps  the inner dimension is walked in gemm_ksteps(k) steps of GEMM_KT; the last one holds gemm_step_len(k, s) <= GEMM_KT products.  A step stages a
//            TM x KT piece of op(A) and a KT x TN piece of op(B) in LDS as [l][i] and [l][j], each row GEMM_PAD elements longer than the tile.
//   fold     every thread folds the products of its 16 outputs in ascending l, across the steps and inside them, starting from the product l = 0.
// Neither the tile shapes nor GEMM_KT have been swept (DESIGN.md "Product of two full matrices").
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint32_t GEMM_TM_WIDE = 64, GEMM_TN_WIDE = 64;       // the wide tile
constexpr uint32_t GEMM_TM_TALL = 256, GEMM_TN_TALL = 16;      // the tall tile: results of at most GEMM_TALL_MAX_N columns
constexpr uint32_t GEMM_TALL_MAX_N = 16;                       // the widest result the tall tile takes
constexpr uint32_t GEMM_KT = 16;                               // products per step: the FP64 tall tile stages 35 KB of LDS, four workgroups a compute unit (32: 71 KB, two)
constexpr uint32_t GEMM_WAVES = 4;                             // waves per workgroup
constexpr uint32_t GEMM_RM = 4, GEMM_RN = 4;                   // the register block of one thread
constexpr uint32_t GEMM_PAD = 4;                               // elements behind each staged row: consecutive l fall into different LDS banks, rows stay 16-byte aligned
constexpr uint32_t GEMM_GRID_CAP = 2048;                       // workgroups: eight per compute unit, a loop past it
constexpr uint32_t GEMM_MIN_TILES = 16;                        // the default rule: tiles of T below which a few workgroups walk k alone — measured: the only sweep points the route lost (4 and 8 tall tiles, k = 256) lie below, every point from 16 tiles won

static_assert(GEMM_TM_WIDE * GEMM_TN_WIDE == GEMM_WAVES * 64 * GEMM_RM * GEMM_RN && GEMM_TM_TALL * GEMM_TN_TALL == GEMM_WAVES * 64 * GEMM_RM * GEMM_RN, "a tile is one register block per thread");
static_assert(GEMM_TM_WIDE % GEMM_RM == 0 && GEMM_TN_WIDE % GEMM_RN == 0 && GEMM_TM_TALL % GEMM_RM == 0 && GEMM_TN_TALL % GEMM_RN == 0, "a tile is whole register blocks");
static_assert(GEMM_TALL_MAX_N <= GEMM_TN_TALL && GEMM_PAD % 4 == 0, "one tall tile spans a narrow result; padded rows keep their alignment");

// the tile shape for a result of n columns
constexpr bool gemm_tall(uint64_t n) { return n <= GEMM_TALL_MAX_N; }
constexpr uint32_t gemm_tm(uint64_t n) { return gemm_tall(n) ? GEMM_TM_TALL : GEMM_TM_WIDE; }
constexpr uint32_t gemm_tn(uint64_t n) { return gemm_tall(n) ? GEMM_TN_TALL : GEMM_TN_WIDE; }
// tiles down, across and in all (no m + TM: m may be nearly 2^32 ... or 2^64 in a check)
constexpr uint64_t gemm_tiles_m(uint64_t m, uint64_t n) { return m / gemm_tm(n) + (m % gemm_tm(n) != 0); }
constexpr uint64_t gemm_tiles_n(uint64_t n) { return n / gemm_tn(n) + (n % gemm_tn(n) != 0); }
constexpr uint64_t gemm_tiles(uint64_t m, uint64_t n) { return gemm_tiles_m(m, n) * gemm_tiles_n(n); }      // (m n < 2^32: no overflow)
// the first row and column of tile t, for t < gemm_tiles(m, n) and n >= 1
constexpr uint64_t gemm_tile_i0(uint64_t t, uint64_t n) { return t / gemm_tiles_n(n) * gemm_tm(n); }
constexpr uint64_t gemm_tile_j0(uint64_t t, uint64_t n) { return t % gemm_tiles_n(n) * gemm_tn(n); }
constexpr uint32_t gemm_grid(uint64_t m, uint64_t n) { const uint64_t t = gemm_tiles(m, n); return t < 1 ? 1u : t > GEMM_GRID_CAP ? GEMM_GRID_CAP : (uint32_t)t; }
// the steps of the inner dimension, and the products [s KT, s KT + gemm_step_len) of step s < gemm_ksteps(k)
constexpr uint64_t gemm_ksteps(uint64_t k) { return k / GEMM_KT + (k % GEMM_KT != 0); }
constexpr uint32_t gemm_step_len(uint64_t k, uint64_t s) { return k - s * GEMM_KT > GEMM_KT ? GEMM_KT : (uint32_t)(k - s * GEMM_KT); }

// (Whether T, m x n with every position an entry, fits the 32-bit layout is spmm_overflows(m, n) of grb_spmm_geom.hpp: the route's one guard, shared with spmm_full.)

// The default rule's work count, m k n multiply-adds, saturating (three factors below 2^32 can pass 2^64)
constexpr uint64_t gemm_work(uint64_t m, uint64_t k, uint64_t n) {
  const uint64_t top = ~0ull;
  if (m == 0 || k == 0 || n == 0) return 0;
  if (m > top / k) return top;
  const uint64_t mk = m * k;
  return mk > top / n ? top : mk * n;
}
// T has at least `least` tiles (tile counts of a check may be near 2^64: no product unless both factors are small)
constexpr bool gemm_has_tiles(uint64_t m, uint64_t n, uint64_t least) {
  const uint64_t a = gemm_tiles_m(m, n), b = gemm_tiles_n(n);
  return a >= least || b >= least || a * b >= least;
}
// by itself: no plain mask (that is the sddmm route's), at least two columns, min_work multiply-adds, and GEMM_MIN_TILES tiles of T
constexpr bool gemm_by_default(uint64_t m, uint64_t k, uint64_t n, bool plain_mask, uint64_t min_work) {
  return !plain_mask && n >= 2 && gemm_work(m, k, n) >= min_work && gemm_has_tiles(m, n, GEMM_MIN_TILES);
}

}  // namespace grb
