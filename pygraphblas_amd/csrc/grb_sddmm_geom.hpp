// grb_sddmm_geom.hpp — the integer side of the masked product of two FULL matrices (grb_sddmm.hpp, the sddmm route of GrB_mxm): the constants of the kernel's
// shape and the integer functions host code and the kernel share.  Plain integers only — no HIP types, no containers — so that a stand-alone program can check
// it under the sanitizers (tests/sddmm_geometry_check.cpp).  Every function is constexpr: host code and the kernel call the same text.
//
// THE SHAPE (T(i, j) = (+)_l X(i, l) (x) Y(j, l) for the entries (i, j) of a mask; X m x k and Y n x k full and row-major; the mask's entries numbered 0 .. E - 1
// in CSR order)
//   tile     SDDMM_TILE consecutive ENTRIES of the mask, whatever rows they lie in: a hub row spreads over many tiles, an empty row belongs to none.  A workgroup
//            of SDDMM_WAVES waves takes tiles blockIdx, blockIdx + grid, ... (a grid capped at SDDMM_GRID_CAP workgroups).  The rows of a tile's first and last
//            entry are found by bisecting the row pointer once per tile; an entry's own row by bisecting between those two (no step when the tile lies in one row).
//   group    G = sddmm_group(k) = pow2ceil(min(k, 64)) lanes serve one entry, 64 / G entries per wave, SDDMM_WAVES * 64 / G per workgroup and pass; a tile takes
//            sddmm_passes() passes.  Lane g of the group owns l = g, g + G, g + 2 G, ... < k: sddmm_trips(k, g) products.
//   fold     lane g folds its products left to right in ascending l, starting from the first one; then for s = G / 2 ... 1: p_g = p_g (+) p_{g + s} where
//            sddmm_takes_part(g, s, k).  Lane 0 holds the entry's value.  The order is a function of k alone.
// None of the constants has been swept (DESIGN.md "Masked product of two full matrices").
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint32_t SDDMM_TILE = 256;            // mask entries per tile: one per thread at G = 1
constexpr uint32_t SDDMM_WAVES = 4;             // waves per workgroup
constexpr uint32_t SDDMM_GRID_CAP = 2048;       // workgroups: eight per compute unit, a loop past it
constexpr uint32_t SDDMM_GROUP_MAX = 64;        // the widest group: one wave

static_assert(SDDMM_TILE % (SDDMM_WAVES * 64) == 0, "a tile is a whole number of passes at G = 1");

// lanes that serve one entry: the power of two >= min(k, 64), for k >= 1
constexpr uint32_t sddmm_group(uint64_t k) { uint32_t g = 1; while (g < SDDMM_GROUP_MAX && g < k) g <<= 1; return g; }
constexpr uint32_t sddmm_gshift(uint64_t k) { uint32_t s = 0; while ((1u << s) < sddmm_group(k)) s++; return s; }
// lanes of a group that hold a product: min(k, G)
constexpr uint32_t sddmm_live(uint64_t k) { return k < sddmm_group(k) ? (uint32_t)k : sddmm_group(k); }
// products lane g of a group folds: the l = g, g + G, ... below k
constexpr uint64_t sddmm_trips(uint64_t k, uint32_t g) { return g < k ? (k - g - 1) / sddmm_group(k) + 1 : 0; }
// butterfly step s (a power of two below G): lane g combines with lane g + s when that lane holds a partial
constexpr bool sddmm_takes_part(uint32_t g, uint32_t s, uint64_t k) { return g + s < sddmm_live(k); }

// entries a workgroup serves in one pass, and the passes of a tile of `count` entries
constexpr uint32_t sddmm_entries_per_pass(uint64_t k) { return SDDMM_WAVES * 64u / sddmm_group(k); }
constexpr uint32_t sddmm_passes(uint32_t count, uint64_t k) { return (count + sddmm_entries_per_pass(k) - 1) / sddmm_entries_per_pass(k); }
// tiles of E entries, and the entries [begin, end) of tile t
constexpr uint64_t sddmm_tiles(uint64_t entries) { return entries / SDDMM_TILE + (entries % SDDMM_TILE != 0); }      // (no entries + TILE: E may be nearly 2^32 ... or 2^64 in a check)
constexpr uint64_t sddmm_tile_begin(uint64_t t) { return t * SDDMM_TILE; }
constexpr uint64_t sddmm_tile_end(uint64_t t, uint64_t entries) { return entries - t * SDDMM_TILE > SDDMM_TILE ? (t + 1) * SDDMM_TILE : entries; }      // for t < sddmm_tiles(entries)
constexpr uint32_t sddmm_grid(uint64_t entries) { const uint64_t t = sddmm_tiles(entries); return t < 1 ? 1u : t > SDDMM_GRID_CAP ? SDDMM_GRID_CAP : (uint32_t)t; }

// The row of entry e: the largest i in [lo, hi] with rowptr[i] <= e, given rowptr[lo] <= e < rowptr[hi + 1].  Empty rows (rowptr[i] == rowptr[i + 1]) are
// stepped over: the answer is the row that holds e.  At most ceil(log2(hi - lo + 1)) reads, none when lo == hi.
template <class RP> constexpr uint32_t sddmm_row_of(const RP& rowptr, uint32_t lo, uint32_t hi, uint64_t e) {
  while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (rowptr[mid] <= e) lo = mid; else hi = mid - 1; }
  return lo;
}

// The default rule: the work the masked Gustavson route would do, m k n probes, saturating (three factors below 2^32 can pass 2^64)
constexpr uint64_t sddmm_masked_work(uint64_t m, uint64_t k, uint64_t n) {
  const uint64_t top = ~0ull;
  if (m == 0 || k == 0 || n == 0) return 0;
  if (m > top / k) return top;
  const uint64_t mk = m * k;
  return mk > top / n ? top : mk * n;
}
constexpr bool sddmm_by_default(uint64_t m, uint64_t k, uint64_t n, uint64_t min_work) { return sddmm_masked_work(m, k, n) >= min_work; }

}  // namespace grb
