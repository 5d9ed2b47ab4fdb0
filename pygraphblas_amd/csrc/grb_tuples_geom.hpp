// grb_tuples_geom.hpp — the integer side of extractTuples in HBM (grb_tuples.hip, GrBX_*_extractTuples_at in grb_tuples_ops.cpp): the tile sizes, the grid, which
// entries and positions a tile holds, the row of an entry by bisection of the row pointer, and the 16-byte alignment test of the output streams.  Plain integers
// only — no HIP types, no containers — so that a stand-alone program can check it under the sanitizers (tests/tuples_geometry_check.cpp).  Every function is
// constexpr: host code and the kernels call the same text.
//
// THE SHAPES
//   matrix   the entries 0 .. nnz of the CSR are cut into tiles of TUPLES_TILE consecutive ENTRIES (never rows: one R-MAT row holds 10^5 entries, and runs of
//            rows hold none).  A workgroup of 256 threads takes tile t, t + grid, ...; the grid is capped at TUPLES_GRID_CAP workgroups.  The workgroup brackets
//            its tile's rows once — the row of the tile's first entry by bisection of the whole row pointer, the row of its last entry by a gallop from there —
//            and every lane bisects inside the bracket.  A lane holds two neighbouring entries (one 16-byte store into I and into J) when the outputs are
//            16-byte aligned, else one entry per round (8-byte stores, still one contiguous run per wave).
//   vector   the positions 0 .. n are cut into tiles of TUPLES_VEC_TILE; each of the workgroup's four waves takes a quarter (TUPLES_VEC_WAVE positions, four
//            rounds of 64) and owns one count word, so that no pass needs LDS or a barrier.
// Neither constant has been swept: 1 024 entries amortise the bracket's ~30 dependent loads over 37 KiB of traffic (FP64), and keep the test sizes small.
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint32_t TUPLES_THREADS = 256;
constexpr uint32_t TUPLES_TILE = 1024;                       // entries per tile of the matrix kernel
constexpr uint32_t TUPLES_VEC_WAVE = 256;                    // positions one wave counts and scatters: four rounds of 64
constexpr uint32_t TUPLES_VEC_TILE = 4 * TUPLES_VEC_WAVE;    // positions per tile (workgroup) of the vector kernels
constexpr uint32_t TUPLES_GRID_CAP = 4096;                   // workgroups, as grid_1d caps the other O(nnz) kernels

static_assert(TUPLES_TILE % (2 * TUPLES_THREADS) == 0, "a tile is a whole number of rounds in both lane shapes");

constexpr uint64_t tuples_tiles(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }
constexpr uint32_t tuples_grid(uint64_t ntiles) { return ntiles < 1 ? 1u : ntiles > TUPLES_GRID_CAP ? TUPLES_GRID_CAP : (uint32_t)ntiles; }
// entries (or positions) of tile t: [t * tile, min((t + 1) * tile, n)) — empty for t >= tuples_tiles(n, tile)
constexpr uint64_t tuples_tile_begin(uint64_t t, uint32_t tile) { return t * tile; }
constexpr uint64_t tuples_tile_end(uint64_t t, uint32_t tile, uint64_t n) { return (t + 1) * tile < n ? (t + 1) * tile : n; }

// The row of entry e: the r in [lo, hi] with rowptr[r] <= e < rowptr[r + 1].  Requires rowptr[lo] <= e < rowptr[hi + 1] (so the row exists, and it is not
// empty); reads rowptr[lo + 1 .. hi] only.  Empty rows before it share its first word and are passed over: the LAST r with rowptr[r] <= e is taken.
constexpr uint32_t tuples_row_of(const uint32_t* rowptr, uint32_t lo, uint32_t hi, uint32_t e) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);           // in (lo, hi]
    if (rowptr[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// The same for an entry known to lie in row `lo` or later (rowptr[lo] <= e < rowptr[last + 1]): doubling steps from lo, then the bisection between the last
// two probes.  A tile's last entry is a few rows behind its first unless a run of empty rows lies between, which costs its logarithm.
constexpr uint32_t tuples_row_from(const uint32_t* rowptr, uint32_t lo, uint32_t last, uint32_t e) {
  uint32_t hi = last; uint64_t step = 1;
  for (uint32_t at = lo; at < last;) {
    const uint32_t nxt = (uint64_t)(last - at) > step ? (uint32_t)(at + step) : last;
    if (rowptr[nxt] <= e) { lo = at = nxt; step <<= 1; } else { hi = nxt - 1; break; }
  }
  return tuples_row_of(rowptr, lo, hi, e);
}

// a stream takes 16-byte stores when its first byte is 16-byte aligned (NULL: the stream is not written, and does not stand in the way)
constexpr bool tuples_aligned16(uint64_t address) { return (address & 15u) == 0; }

}  // namespace grb
