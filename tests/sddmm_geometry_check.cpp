// sddmm_geometry_check.cpp — grb_sddmm_geom.hpp on its own (plain integers, host code only): the group width, the live lanes and every lane's loop trips for k
// from 1 to 300 (the lanes' products cover l = 0 .. k - 1 exactly once, each lane's in ascending order); the lanes that take part in each butterfly step, by
// simulating the fold on SETS of l and asking that lane 0 ends with every l exactly once; tiles to entry ranges for counts around the tile size and the grid cap
// (the tiles cover the entries once, in order, and a workgroup's passes cover a tile once); the row bisection against a linear walk for row pointers with empty
// rows in front, in the middle and at the end and a hub row longer than two tiles; the overflow guards of the tile arithmetic and of the default rule's m k n.
// Built with the address and undefined-behaviour sanitizers by tests/test_sddmm_host.py; prints "sddmm geometry ok".
#include "grb_sddmm_geom.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// the fold of one entry for k products, on multisets of l: count[g][l] = how often product l is inside lane g's partial
static void check_fold(uint32_t k) {
  const uint32_t G = sddmm_group(k), live = sddmm_live(k);
  CHECK(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && 64 % G == 0 && (1u << sddmm_gshift(k)) == G);
  CHECK(k > 64 ? G == 64 : (G >= k && (G == 1 || G / 2 < k)));
  CHECK(live == (k < G ? k : G) && live >= 1);
  std::vector<std::vector<uint32_t>> part(G, std::vector<uint32_t>(k, 0));
  uint64_t total = 0;
  for (uint32_t g = 0; g < G; g++) {
    const uint64_t trips = sddmm_trips(k, g);
    CHECK((trips != 0) == (g < live));
    uint64_t n = 0; for (uint64_t l = g; l < k; l += G) { part[g][l]++; n++; }      // the kernel's loop
    CHECK(n == trips); total += trips;
  }
  CHECK(total == k);
  uint32_t steps = 0;
  for (uint32_t s = G >> 1; s; s >>= 1, steps++) {
    std::vector<std::vector<uint32_t>> next = part;                                   // every lane reads its partner's partial of BEFORE the step
    for (uint32_t g = 0; g < G; g++) {
      const bool in = sddmm_takes_part(g, s, k);
      CHECK(in == (g + s < live));
      if (!in) continue;
      CHECK(g + s < G && sddmm_trips(k, g + s) != 0 && sddmm_trips(k, g) != 0);     // both lanes hold a partial: no identity is ever needed
      for (uint32_t l = 0; l < k; l++) next[g][l] = part[g][l] + part[g + s][l];
    }
    part.swap(next);
  }
  CHECK((1u << steps) == G);
  for (uint32_t l = 0; l < k; l++) CHECK(part[0][l] == 1);                            // lane 0: every product exactly once
}

// tiles over E entries: in order, disjoint, covering; passes cover a tile
static void check_tiles(uint64_t E) {
  const uint64_t nt = sddmm_tiles(E);
  CHECK(nt == (E + SDDMM_TILE - 1) / SDDMM_TILE);
  uint64_t at = 0;
  for (uint64_t t = 0; t < nt; t++) {
    const uint64_t b = sddmm_tile_begin(t), e = sddmm_tile_end(t, E);
    CHECK(b == at && e > b && e - b <= SDDMM_TILE && e <= E && ((t + 1 == nt) == (e == E)));
    at = e;
    for (uint32_t k : {1u, 2u, 3u, 17u, 64u, 300u}) {
      const uint32_t per = sddmm_entries_per_pass(k), passes = sddmm_passes((uint32_t)(e - b), k);
      CHECK(per * sddmm_group(k) == SDDMM_WAVES * 64 && (uint64_t)passes * per >= e - b && (uint64_t)(passes - 1) * per < e - b);
    }
  }
  CHECK(at == E);
  const uint32_t grid = sddmm_grid(E);
  CHECK(grid >= 1 && grid <= SDDMM_GRID_CAP && (nt == 0 ? grid == 1 : grid == (nt < SDDMM_GRID_CAP ? nt : SDDMM_GRID_CAP)));
}

// the row of every entry, by bisection between the tile's end rows, against a linear walk
static void check_rows(const std::vector<uint32_t>& len) {
  const uint32_t m = (uint32_t)len.size();
  uint32_t* rowptr = (uint32_t*)calloc(m + 1, 4);                                   // exactly m + 1 words: the address sanitizer sees a read outside
  for (uint32_t r = 0; r < m; r++) rowptr[r + 1] = rowptr[r] + len[r];
  const uint64_t E = rowptr[m];
  std::vector<uint32_t> row; for (uint32_t r = 0; r < m; r++) for (uint32_t x = 0; x < len[r]; x++) row.push_back(r);
  for (uint64_t t = 0; t < sddmm_tiles(E); t++) {
    const uint64_t t0 = sddmm_tile_begin(t), t1 = sddmm_tile_end(t, E);
    const uint32_t rlo = sddmm_row_of(rowptr, 0u, m - 1, t0), rhi = sddmm_row_of(rowptr, rlo, m - 1, t1 - 1);
    CHECK(rlo == row[t0] && rhi == row[t1 - 1]);
    for (uint64_t e = t0; e < t1; e++) CHECK(sddmm_row_of(rowptr, rlo, rhi, e) == row[e]);
  }
  free(rowptr);
}

int main() {
  const uint32_t T = SDDMM_TILE, CAP = SDDMM_GRID_CAP;
  CHECK(T % (SDDMM_WAVES * 64) == 0 && SDDMM_WAVES >= 1 && SDDMM_WAVES <= 16 && CAP >= 1 && SDDMM_GROUP_MAX == 64);
  for (uint32_t k = 1; k <= 300; k++) check_fold(k);
  CHECK(sddmm_group(1) == 1 && sddmm_group(2) == 2 && sddmm_group(3) == 4 && sddmm_group(33) == 64 && sddmm_group(64) == 64 && sddmm_group(65) == 64 && sddmm_group(~0ull) == 64);
  CHECK(sddmm_trips(257, 0) == 5 && sddmm_trips(257, 1) == 4 && sddmm_trips(64, 63) == 1 && sddmm_trips(65, 0) == 2 && sddmm_trips(3, 3) == 0 && sddmm_trips(0xFFFFFFFFull, 0) == (1u << 26));
  // k = 3: G = 4, lanes 0, 1, 2 live; step 2 combines lane 0 with lane 2 only, step 1 lane 0 with lane 1 (and lane 1 with lane 2, whose result nobody reads)
  CHECK(sddmm_takes_part(0, 2, 3) && !sddmm_takes_part(1, 2, 3) && sddmm_takes_part(0, 1, 3) && sddmm_takes_part(1, 1, 3) && !sddmm_takes_part(2, 1, 3));
  // tiles around the tile size and the grid cap
  const uint64_t T64 = T, full_round = (uint64_t)CAP * T;
  for (uint64_t E : std::vector<uint64_t>{0, 1, T64 - 1, T64, T64 + 1, 2 * T64, 2 * T64 + 1, full_round - 1, full_round, full_round + 1}) check_tiles(E);
  CHECK(sddmm_grid((uint64_t)CAP * T + 1) == CAP && sddmm_tiles((uint64_t)CAP * T + 1) == CAP + 1);
  // the overflow guards: counts at the device layout's limit and at the 64-bit limit
  CHECK(sddmm_tiles(0xFFFFFFF0ull) == 0xFFFFFFF0ull / T + 1 && sddmm_tile_end(0xFFFFFFF0ull / T, 0xFFFFFFF0ull) == 0xFFFFFFF0ull && sddmm_tile_end(0xFFFFFFF0ull / T - 1, 0xFFFFFFF0ull) == 0xFFFFFFF0ull / T * T);
  CHECK(sddmm_tiles(~0ull) == ~0ull / T + 1 && sddmm_tile_end(~0ull / T, ~0ull) == ~0ull && sddmm_grid(~0ull) == CAP);
  // rows
  check_rows({1});
  check_rows({0, 0, 3, 0, 0, 5, 1, 0});
  check_rows({0, 0, 0, T - 1, 0, 1, 0, 0, 1, T, 0});
  check_rows({2, 2 * T + 7, 0, 1, 3});
  check_rows({T, T, 0, T});                                                           // row boundaries on tile boundaries
  { std::vector<uint32_t> len; for (uint32_t r = 0; r < 700; r++) len.push_back(r % 7 == 3 ? 0 : r % 5); check_rows(len); }
  // the default rule's work count saturates
  CHECK(sddmm_masked_work(64, 64, 64) == (1ull << 18) && sddmm_masked_work(0, 5, 5) == 0 && sddmm_masked_work(5, 0, 5) == 0);
  CHECK(sddmm_masked_work(1ull << 31, 1ull << 31, 1ull << 31) == ~0ull && sddmm_masked_work(1ull << 32, 1ull << 31, 1) == (1ull << 63) && sddmm_masked_work(1ull << 32, 1ull << 32, 1) == ~0ull);
  CHECK(sddmm_by_default(64, 64, 64, 1ull << 18) && !sddmm_by_default(64, 64, 63, 1ull << 18) && sddmm_by_default(~0ull, ~0ull, ~0ull, ~0ull));
  printf("sddmm geometry ok\n");
  return 0;
}
