// grb_tile.hpp — host interface of the concat / split kernels (grb_tile.hip): a grid of CSR tiles into one CSR, one CSR into a grid of CSR tiles.
#pragma once
#include "grb_internal.hpp"
#include "grb_tile_geom.hpp"
#include <vector>

namespace grb {

// The descriptor table of one call, one record per tile (row-major), uploaded in one copy with the two bounds arrays behind it:
//   [TileDesc x m n][rowb u32 x (m + 1)][colb u32 x (n + 1)]
// concat reads through the three pointers, split writes through them.
struct TileDesc { uint32_t* rowptr; uint32_t* col; uint8_t* val; uint32_t row0, col0; uint64_t eprefix; };      // eprefix: entries of the tiles before this one
static_assert(sizeof(TileDesc) == 40, "the bounds arrays behind the table stay 4-byte aligned");

// a grid whose bounds fit the 32-bit device layout (the entry points checked it: rowb[m], colb[n] <= GRB_DIM_DEVICE_MAX)
struct TileGrid { uint32_t m = 0, n = 0; std::vector<uint32_t> rowb, colb; };
// a tile of concat: its CSR image and its values already in C's type (the image's own array, or a cast copy)
struct TileSrc { const DevCSR* csr; const void* val; };

// T = the tiles put together: T's row r of tile-row a is the rows r - rowb[a] of tiles (a, 0 .. n - 1) one after the other, columns + colb[b]; values of `ts`
// bytes moved untouched.  The tiles have sorted rows; so has T.  Requires (checked by the caller, grb_tile_ops.cpp): the tiles' shapes conform to the grid
// and the sum of their entries is <= TILE_MAX_ENTRIES.  Launches: count, scan, fill — whatever m n is.
void concat_csr(size_t ts, const TileGrid& g, const std::vector<TileSrc>& tiles, DevCSR& T);
// out[a n + b] = A(rowb[a] .. rowb[a + 1], colb[b] .. colb[b + 1]) with the origin subtracted, for every tile; values of `ts` bytes moved untouched.  A is only
// read.  Requires: rowb[m] == A.nrows, colb[n] == A.ncols, no empty block, n A.nrows <= TILE_MAX_ENTRIES.  Launches: count, scan, totals, row pointers,
// scatter, and one read-back of the m n totals that size the outputs — whatever m n is.
void split_csr(size_t ts, const TileGrid& g, const DevCSR& A, std::vector<DevCSR>& out);

}  // namespace grb
