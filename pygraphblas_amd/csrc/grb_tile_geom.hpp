// grb_tile_geom.hpp — the integer side of GxB_Matrix_concat / GxB_Matrix_split (grb_tile_ops.cpp, grb_tile.hip): the bounds of a tile grid as prefix sums of
// its sizes, the verdict on the arguments of both calls, which tile-row / column block an index lies in, where a tile's counts stand in split's flat count
// buffer, and the cut of the entries into chunks.  Plain integers only — no HIP types, no containers — so that a stand-alone program can check it under the
// sanitizers (tests/tile_geometry_check.cpp).  Every function is constexpr: host code and the kernels call the same text.
//
// THE SHAPES
//   grid     m x n tiles, row-major: tile (a, b) is number a n + b.  rowb[0 .. m] / colb[0 .. n] are the prefix sums of the tile-rows' heights / the column
//            blocks' widths: tile (a, b) covers rows rowb[a] .. rowb[a + 1] and columns colb[b] .. colb[b + 1] of the whole matrix.
//   entries  both fill kernels cut the ENTRIES 0 .. nnz of the whole matrix (C of concat, A of split) into chunks of TILE_CHUNK consecutive entries — never
//            rows: one R-MAT row holds 10^5 entries — a workgroup of TILE_THREADS takes chunk c, c + grid, ...; the grid is capped at TILE_GRID_CAP.
//   counts   split counts per (row of A, column block) into ONE flat buffer ordered tile by tile: the nr_a counts of tile (a, b) begin at
//            tile_count_base(...) = n rowb[a] + b nr_a.  One exclusive scan S over it holds every tile's row pointer: rowptr_t[lr] = S[base + lr] - S[base],
//            and base of the next tile = base + nr_a, so a tile's total is S[next base] - S[base].
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint32_t TILE_THREADS = 256;
constexpr uint32_t TILE_CHUNK = 1024;          // entries per chunk of the two fill kernels
constexpr uint32_t TILE_EPL = 4;               // consecutive entries of C one lane of the concat fill stores: 16 bytes of columns
constexpr uint32_t TILE_GRID_CAP = 4096;       // workgroups, as grid_1d caps the other O(nnz) kernels
constexpr uint64_t TILE_DIM_MAX = 0xFFFFFFF0ull;        // = GRB_DIM_DEVICE_MAX: dimensions of the 32-bit device layout
constexpr uint64_t TILE_MAX_ENTRIES = 0xFFFFFFF0ull;    // = KRON_MAX_ENTRIES: entries of the 32-bit device layout

static_assert(TILE_CHUNK % (TILE_THREADS * TILE_EPL) == 0, "a chunk is a whole number of rounds of the concat fill");

constexpr uint64_t tile_chunks(uint64_t nnz) { return (nnz + TILE_CHUNK - 1) / TILE_CHUNK; }
constexpr uint32_t tile_grid(uint64_t nchunks) { return nchunks < 1 ? 1u : nchunks > TILE_GRID_CAP ? TILE_GRID_CAP : (uint32_t)nchunks; }
// entries of chunk c: [c * TILE_CHUNK, min((c + 1) * TILE_CHUNK, nnz)) — empty for c >= tile_chunks(nnz)
constexpr uint64_t tile_chunk_begin(uint64_t c) { return c * TILE_CHUNK; }
constexpr uint64_t tile_chunk_end(uint64_t c, uint64_t nnz) { return (c + 1) * TILE_CHUNK < nnz ? (c + 1) * TILE_CHUNK : nnz; }

// bounds[0 .. k] = prefix sums of sizes[0 .. k); false when a sum passes 2^64 (bounds is then not to be used)
constexpr bool tile_bounds(const uint64_t* sizes, uint64_t k, uint64_t* bounds) {
  uint64_t s = 0; bounds[0] = 0;
  for (uint64_t i = 0; i < k; i++) { if (sizes[i] > ~s) return false; s += sizes[i]; bounds[i + 1] = s; }
  return true;
}

// the verdicts, in the order the checks are made; the entry points map them to GrB_Info
enum TileVerdict { TILE_OK = 0, TILE_NULL, TILE_INVALID, TILE_MISMATCH };

// GxB_Matrix_split: the grid and the size arrays against A's shape.  A size of 0 is refused (TILE_INVALID); sums that differ from (or wrap past) the shape
// are TILE_MISMATCH.  On TILE_OK rowb[0 .. m] and colb[0 .. n] hold the bounds.
constexpr TileVerdict tile_check_split(uint64_t m, uint64_t n, const uint64_t* tile_nrows, const uint64_t* tile_ncols, uint64_t nrows, uint64_t ncols, uint64_t* rowb, uint64_t* colb) {
  if (!tile_nrows || !tile_ncols || !rowb || !colb) return TILE_NULL;
  if (m == 0 || n == 0) return TILE_INVALID;
  for (uint64_t a = 0; a < m; a++) if (tile_nrows[a] == 0) return TILE_INVALID;
  for (uint64_t b = 0; b < n; b++) if (tile_ncols[b] == 0) return TILE_INVALID;
  if (!tile_bounds(tile_nrows, m, rowb) || !tile_bounds(tile_ncols, n, colb)) return TILE_MISMATCH;
  return (rowb[m] == nrows && colb[n] == ncols) ? TILE_OK : TILE_MISMATCH;
}
// GxB_Matrix_concat: the shapes of the m n tiles (shape_rows[t], shape_cols[t], row-major) against each other and against C's shape.  Tiles of a tile-row
// share their height, tiles of a column block their width (the first tile of each names it), the sums are C's shape.  On TILE_OK the bounds are filled.
constexpr TileVerdict tile_check_concat(uint64_t m, uint64_t n, const uint64_t* shape_rows, const uint64_t* shape_cols, uint64_t nrows, uint64_t ncols, uint64_t* rowb, uint64_t* colb) {
  if (!shape_rows || !shape_cols || !rowb || !colb) return TILE_NULL;
  if (m == 0 || n == 0) return TILE_INVALID;
  for (uint64_t a = 0; a < m; a++) for (uint64_t b = 0; b < n; b++)
    if (shape_rows[a * n + b] != shape_rows[a * n] || shape_cols[a * n + b] != shape_cols[b]) return TILE_MISMATCH;
  uint64_t s = 0; rowb[0] = 0;
  for (uint64_t a = 0; a < m; a++) { const uint64_t h = shape_rows[a * n]; if (h > ~s) return TILE_MISMATCH; s += h; rowb[a + 1] = s; }
  s = 0; colb[0] = 0;
  for (uint64_t b = 0; b < n; b++) { const uint64_t w = shape_cols[b]; if (w > ~s) return TILE_MISMATCH; s += w; colb[b + 1] = s; }
  return (rowb[m] == nrows && colb[n] == ncols) ? TILE_OK : TILE_MISMATCH;
}

// The block of index x: the LAST k in [0, nb) with bounds[k] <= x.  Requires bounds[0] <= x < bounds[nb] and nb >= 1; reads bounds[1 .. nb - 1] only.  An
// empty block (bounds[k] == bounds[k + 1], concat only) is passed over: the block taken is the one that holds x.
template <class W> constexpr uint32_t tile_block_of(const W* bounds, uint32_t nb, W x) {
  uint32_t lo = 0, hi = nb - 1;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if (bounds[mid] <= x) lo = mid; else hi = mid - 1; }
  return lo;
}

// split's flat count buffer: where the counts of tile (a, b) begin (nr_a of them), and the tile-row of a flat position (by the bounds scaled by n)
constexpr uint64_t tile_count_base(const uint32_t* rowb, uint32_t n, uint32_t a, uint32_t b) { return (uint64_t)n * rowb[a] + (uint64_t)b * (rowb[a + 1] - rowb[a]); }
constexpr uint32_t tile_count_row_of(const uint32_t* rowb, uint32_t m, uint32_t n, uint64_t pos) {      // requires pos < n rowb[m], non-empty tile-rows
  uint32_t lo = 0, hi = m - 1;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if ((uint64_t)n * rowb[mid] <= pos) lo = mid; else hi = mid - 1; }
  return lo;
}

// The first position p in [lo, hi) of a sorted run of columns with col[p] >= x, or hi: how split cuts a row at a block boundary, and how its scatter finds
// where an entry's block begins inside the row.
constexpr uint32_t tile_lower_bound(const uint32_t* col, uint32_t lo, uint32_t hi, uint32_t x) {
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (col[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

// Where entry k (counted from the row's first) of row lr of a concatenated tile-row comes from: walking the row's n tiles with their lengths len[b], the tile
// that holds it and its position inside that tile's row.  `len_of(b)` returns the length of the row in tile b; requires k < the sum of the lengths.
struct TileSeg { uint32_t b, at, left; };      // column block, position in that tile's row, entries of that row from `at` on (>= 1)
template <class LenOf> constexpr TileSeg tile_segment(uint32_t n, uint32_t k, LenOf len_of) {
  uint32_t b = 0, len = len_of(0u);
  while (k >= len && b + 1 < n) { k -= len; b++; len = len_of(b); }
  return TileSeg{b, k, len - k};
}

}  // namespace grb
