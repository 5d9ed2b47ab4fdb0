// tuples_geometry_check.cpp — grb_tuples_geom.hpp on its own (plain integers, host code only): the tile and grid counts at their edges, the tiles covering the
// entries exactly once, the row of an entry by bisection and by gallop against a linear walk over row pointers with long rows, single-entry rows and runs of empty
// rows at the start, in the middle and at the end, every probe inside the row pointer (the arrays are heap blocks of exactly nrows + 1 words: the address
// sanitizer sees a probe outside), and the alignment test.  Built with the address and undefined-behaviour sanitizers by tests/test_tuples_host.py; prints
// "tuples geometry ok".
#include "grb_tuples_geom.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// rows given by their lengths; every entry's row by both searches, from every legal bracket start, against the walk
static void check_rows(const std::vector<uint32_t>& len) {
  const uint32_t nrows = (uint32_t)len.size();
  uint32_t* rowptr = (uint32_t*)malloc(((size_t)nrows + 1) * 4);      // exactly nrows + 1 words
  rowptr[0] = 0; for (uint32_t r = 0; r < nrows; r++) rowptr[r + 1] = rowptr[r] + len[r];
  const uint32_t nnz = rowptr[nrows];
  uint32_t row = 0;
  for (uint32_t e = 0; e < nnz; e++) {
    while (rowptr[row + 1] <= e) row++;                                // the model: walk forward
    CHECK(tuples_row_of(rowptr, 0, nrows - 1, e) == row);
    CHECK(tuples_row_from(rowptr, 0, nrows - 1, e) == row);
    CHECK(tuples_row_of(rowptr, row, row, e) == row);
    CHECK(tuples_row_from(rowptr, row, nrows - 1, e) == row);
    CHECK(tuples_row_from(rowptr, row, row, e) == row);
    // a tile's bracket: the rows of its first and last entry, and a lane's search inside it
    const uint64_t t = e / TUPLES_TILE, base = tuples_tile_begin(t, TUPLES_TILE), end = tuples_tile_end(t, TUPLES_TILE, nnz);
    const uint32_t rlo = tuples_row_of(rowptr, 0, nrows - 1, (uint32_t)base), rhi = tuples_row_from(rowptr, rlo, nrows - 1, (uint32_t)(end - 1));
    CHECK(rlo <= row && row <= rhi && tuples_row_of(rowptr, rlo, rhi, e) == row);
    if (e + 1 < end && rowptr[row + 1] <= e + 1) { CHECK(row < rhi); CHECK(rowptr[tuples_row_of(rowptr, row + 1, rhi, e + 1)] <= e + 1); }      // the second entry of a lane's pair
  }
  free(rowptr);
}

int main() {
  const uint32_t T = TUPLES_TILE, V = TUPLES_VEC_TILE, W = TUPLES_VEC_WAVE;
  CHECK(T % 512 == 0 && V == 4 * W && W % 64 == 0 && TUPLES_THREADS == 256 && TUPLES_GRID_CAP >= 1);
  // tiles and grid
  CHECK(tuples_tiles(0, T) == 0 && tuples_tiles(1, T) == 1 && tuples_tiles(T - 1, T) == 1 && tuples_tiles(T, T) == 1 && tuples_tiles(T + 1, T) == 2);
  CHECK(tuples_tiles(0xFFFFFFF0ull, T) == (0xFFFFFFF0ull + T - 1) / T && tuples_tiles(0xFFFFFFF0ull, W) * W >= 0xFFFFFFF0ull);
  CHECK(tuples_grid(0) == 1 && tuples_grid(1) == 1 && tuples_grid(TUPLES_GRID_CAP) == TUPLES_GRID_CAP && tuples_grid(TUPLES_GRID_CAP + 1ull) == TUPLES_GRID_CAP && tuples_grid(1ull << 40) == TUPLES_GRID_CAP);
  const uint64_t G = (uint64_t)TUPLES_GRID_CAP * T;
  CHECK(tuples_tiles(G, T) == TUPLES_GRID_CAP && tuples_tiles(G + 1, T) == TUPLES_GRID_CAP + 1ull);      // G + 1 entries: one workgroup makes a second round
  // the tiles cover [0, n) once, in order
  for (uint64_t n : {(uint64_t)1, (uint64_t)T - 1, (uint64_t)T, (uint64_t)T + 1, (uint64_t)3 * T + 1, (uint64_t)0xFFFFFFF0u}) {
    const uint64_t nt = tuples_tiles(n, T);
    CHECK(tuples_tile_begin(0, T) == 0 && tuples_tile_end(nt - 1, T, n) == n && tuples_tile_begin(nt - 1, T) < n);
    for (uint64_t t : {(uint64_t)0, nt / 2, nt - 1}) { CHECK(tuples_tile_begin(t, T) < tuples_tile_end(t, T, n) && tuples_tile_end(t, T, n) - tuples_tile_begin(t, T) <= T); if (t + 1 < nt) CHECK(tuples_tile_end(t, T, n) == tuples_tile_begin(t + 1, T)); }
    CHECK((tuples_tile_begin(nt - 1, T) * 8) % 16 == 0);                                                   // a tile begins on a 16-byte boundary of every stream
  }
  // rows
  check_rows({1});
  check_rows({5});
  check_rows({1, 1, 1, 1});
  check_rows({1, 3 * T + 1, 1});                                         // one long row between single-entry rows: its tiles' bracket is that one row
  { std::vector<uint32_t> len(2 * T + 3 + 4, 0); len[0] = 2; len[1] = 1; len[len.size() - 2] = 1; len[len.size() - 1] = T + 5; check_rows(len); }      // empty rows in the middle
  { std::vector<uint32_t> len(2 * T + 3 + 2, 0); len[len.size() - 2] = 3; len[len.size() - 1] = 1; check_rows(len); }                                    // ... at the start
  { std::vector<uint32_t> len(2 * T + 3 + 2, 0); len[0] = T; len[1] = 1; check_rows(len); }                                                             // ... at the end
  { std::vector<uint32_t> len(3000); for (size_t r = 0; r < len.size(); r++) len[r] = ((uint32_t)(r * 2654435761u) >> 29) * (r % 3 == 0 ? 0u : 1u); len[1500] = 2 * T; check_rows(len); }
  // the extreme words: a row pointer whose entries reach the device limit is searched without overflow (two rows, the second one holds the last entry)
  { uint32_t rp[3] = {0, 0xFFFFFFEFu, 0xFFFFFFF0u}; CHECK(tuples_row_of(rp, 0, 1, 0xFFFFFFEFu) == 1 && tuples_row_of(rp, 0, 1, 0xFFFFFFEEu) == 0 && tuples_row_from(rp, 0, 1, 0xFFFFFFEFu) == 1); }
  // alignment
  CHECK(tuples_aligned16(0) && tuples_aligned16(16) && tuples_aligned16(0x7f0000001000ull) && !tuples_aligned16(8) && !tuples_aligned16(0x7f0000001008ull) && !tuples_aligned16(1));
  printf("tuples geometry ok\n");
  return 0;
}
