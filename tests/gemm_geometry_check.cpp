// gemm_geometry_check.cpp — grb_gemm_geom.hpp on its own (plain integers, host code only): the tile maps for m and n around 1, the tile sizes and the switch
// between the tall and the wide shape (the tiles cover [0, m) x [0, n) exactly once, counted cell by cell, each thread's 4 x 4 block inside its tile); the
// grid-stride walk under the cap (every tile once); the k steps for k = 1 .. 3 KT + 1 (they cover [0, k) once, in ascending order, only the last one ragged); the
// staging loops' index maps (every LDS word of a step once); the route's overflow guard (spmm_overflows, grb_spmm_geom.hpp) at m n = 2^32 -/+ 1 and at the device
// layout's limit; the default rule.  Built with the address and undefined-behaviour sanitizers by tests/test_gemm_full_host.py; prints "gemm geometry ok".
// With arguments `m k n plain_mask` it prints instead what the library's rule says of that call: "rule <0|1> min_work <GEMM_FULL_MIN_WORK>".
#include "grb_gemm_geom.hpp"
#include "grb_spmm_geom.hpp"      // spmm_overflows: the guard the route tests T with
#include "grb_route.hpp"          // GEMM_FULL_MIN_WORK
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// every cell of an m x n result is written by exactly one (tile, thread, register), walking the tiles as the grid does
static void check_cover(uint64_t m, uint64_t n) {
  const uint32_t tm = gemm_tm(n), tn = gemm_tn(n), threads = GEMM_WAVES * 64;
  CHECK((tm == GEMM_TM_TALL && tn == GEMM_TN_TALL) == (n <= GEMM_TALL_MAX_N) && (tm == GEMM_TM_WIDE && tn == GEMM_TN_WIDE) == (n > GEMM_TALL_MAX_N));
  const uint64_t nt = gemm_tiles(m, n);
  CHECK(gemm_tiles_m(m, n) == (m + tm - 1) / tm && gemm_tiles_n(n) == (n + tn - 1) / tn && nt == gemm_tiles_m(m, n) * gemm_tiles_n(n));
  const uint32_t grid = gemm_grid(m, n);
  CHECK(grid >= 1 && grid <= GEMM_GRID_CAP && grid == (nt < 1 ? 1 : nt < GEMM_GRID_CAP ? nt : GEMM_GRID_CAP));
  uint8_t* hit = (uint8_t*)calloc(m * n ? m * n : 1, 1);                     // exactly m n bytes: the address sanitizer sees a store outside
  std::vector<uint8_t> tile_seen(nt, 0);
  const uint32_t tx_n = tn / GEMM_RN;
  for (uint32_t b = 0; b < grid; b++)
    for (uint64_t t = b; t < nt; t += grid) {
      CHECK(!tile_seen[t]); tile_seen[t] = 1;
      const uint64_t i0 = gemm_tile_i0(t, n), j0 = gemm_tile_j0(t, n);
      CHECK(i0 < m && j0 < n && i0 % tm == 0 && j0 % tn == 0);
      for (uint32_t th = 0; th < threads; th++) {
        const uint32_t ri = th / tx_n * GEMM_RM, cj = th % tx_n * GEMM_RN;      // the kernel's thread map
        CHECK(ri + GEMM_RM <= tm && cj + GEMM_RN <= tn);
        for (uint32_t r = 0; r < GEMM_RM; r++) for (uint32_t c = 0; c < GEMM_RN; c++) {
          const uint64_t i = i0 + ri + r, j = j0 + cj + c;
          if (i < m && j < n) { CHECK(hit[i * n + j] == 0); hit[i * n + j] = 1; }
        }
      }
    }
  for (uint64_t t = 0; t < nt; t++) CHECK(tile_seen[t]);
  for (uint64_t e = 0; e < m * n; e++) CHECK(hit[e] == 1);
  free(hit);
}

// the steps of k products: in order, disjoint, covering, only the last one short
static void check_steps(uint64_t k) {
  const uint64_t ns = gemm_ksteps(k);
  CHECK(ns == (k + GEMM_KT - 1) / GEMM_KT);
  uint64_t at = 0, walked = 0;
  for (uint64_t l0 = 0; l0 < k; l0 += GEMM_KT, walked++) {                    // the kernel's loop
    const uint32_t len = gemm_step_len(k, l0 / GEMM_KT);
    CHECK(l0 == at && len >= 1 && len <= GEMM_KT && (len == GEMM_KT || walked + 1 == ns));
    at += len;
  }
  CHECK(at == k && walked == ns);
}

// the staging loops: R rows (or columns) of a tile side times KT products, both index maps; every word of dst[l][r] once, inside the padded row
static void check_stage(uint32_t R) {
  const uint32_t threads = GEMM_WAVES * 64;
  CHECK((R * GEMM_KT) % threads == 0);
  for (int along_l = 0; along_l < 2; along_l++) {
    uint8_t* lds = (uint8_t*)calloc((size_t)GEMM_KT * (R + GEMM_PAD), 1);
    for (uint32_t th = 0; th < threads; th++)
      for (uint32_t e = th; e < R * GEMM_KT; e += threads) {
        const uint32_t l = along_l ? e % GEMM_KT : e / R, r = along_l ? e / GEMM_KT : e % R;
        CHECK(l < GEMM_KT && r < R);
        uint8_t& w = lds[(size_t)l * (R + GEMM_PAD) + r]; CHECK(w == 0); w = 1;
      }
    for (uint32_t l = 0; l < GEMM_KT; l++) for (uint32_t r = 0; r < R + GEMM_PAD; r++) CHECK(lds[(size_t)l * (R + GEMM_PAD) + r] == (r < R));
    free(lds);
  }
}

int main(int argc, char** argv) {
  if (argc == 5) {                                                             // the default rule as the library compiles it, for the host test
    printf("rule %d min_work %llu\n", (int)gemm_by_default(strtoull(argv[1], 0, 10), strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10), atoi(argv[4]) != 0, GEMM_FULL_MIN_WORK),
           (unsigned long long)GEMM_FULL_MIN_WORK);
    return 0;
  }
  const uint64_t TM = GEMM_TM_WIDE, TN = GEMM_TN_WIDE, TTM = GEMM_TM_TALL, TTN = GEMM_TN_TALL, CAP = GEMM_GRID_CAP, KT = GEMM_KT, NSW = GEMM_TALL_MAX_N;
  CHECK(TM * TN == GEMM_WAVES * 64 * 16 && TTM * TTN == GEMM_WAVES * 64 * 16 && GEMM_RM == 4 && GEMM_RN == 4 && (KT == 16 || KT == 32) && NSW <= TTN && NSW == 16);
  for (uint64_t m : std::vector<uint64_t>{1, 2, TM - 1, TM, TM + 1, 2 * TM + 1, TTM - 1, TTM, TTM + 1})
    for (uint64_t n : std::vector<uint64_t>{1, 2, 3, NSW - 1, NSW, NSW + 1, TN - 1, TN, TN + 1, 2 * TN + 1}) check_cover(m, n);
  // past one grid round: one tile more than the cap, wide and tall, and a two-dimensional tiling beyond it
  check_cover((CAP + 1) * TM, TN); check_cover((CAP + 1) * TTM, 3); check_cover(47 * TM + 5, 45 * TN + 7);
  CHECK(gemm_tiles((CAP + 1) * TM, TN) == CAP + 1 && gemm_grid((CAP + 1) * TM, TN) == CAP && gemm_grid(0, 5) == 1);
  CHECK(gemm_tile_i0(CAP, TN) == CAP * TM && gemm_tile_j0(CAP, TN) == 0 && gemm_tile_i0(5, 2 * TN + 1) == TM && gemm_tile_j0(5, 2 * TN + 1) == 2 * TN);
  for (uint64_t k = 1; k <= 3 * KT + 1; k++) check_steps(k);
  CHECK(gemm_ksteps(257) == (257 + KT - 1) / KT && gemm_step_len(257, gemm_ksteps(257) - 1) == 257 - (gemm_ksteps(257) - 1) * KT);
  CHECK(gemm_ksteps(0xFFFFFFEFull) == 0xFFFFFFEFull / KT + 1 && gemm_step_len(0xFFFFFFEFull, 0xFFFFFFEFull / KT) == 0xFFFFFFEFull % KT);
  CHECK((uint64_t)(uint32_t)(0xFFFFFFEFull / KT * KT + KT) == 0xFFFFFFEFull / KT * KT + KT);      // the kernel's 32-bit l0 + KT does not wrap for the largest k
  for (uint32_t R : {GEMM_TM_WIDE, GEMM_TN_WIDE, GEMM_TM_TALL, GEMM_TN_TALL}) check_stage(R);
  // the overflow guards: m n at 2^32 -/+ 1 is refused, the device layout's limit 2^32 - 16 is the first refused count
  CHECK(spmm_overflows(0xFFFFFFFFull, 1) && spmm_overflows(1, 0xFFFFFFFFull) && spmm_overflows(0x100000001ull, 1) && spmm_overflows(1, 0x100000001ull));
  CHECK(spmm_overflows(65537, 65535) && spmm_overflows(65535, 65537) && spmm_overflows(641, 6700417) && spmm_overflows(1ull << 16, 1ull << 16));      // 2^32 - 1, 2^32 + 1 = 641 * 6700417, 2^32
  CHECK(spmm_overflows(SPMM_ENTRY_MAX, 1) && !spmm_overflows(SPMM_ENTRY_MAX - 1, 1) && !spmm_overflows(1, SPMM_ENTRY_MAX - 1) && spmm_overflows(~0ull, ~0ull) && !spmm_overflows(~0ull, 0));
  CHECK(!spmm_overflows(65535, 65535) && !spmm_overflows(1ull << 20, 64) && gemm_tiles(65535, 65535) == 1024ull * 1024);
  CHECK(gemm_tiles(SPMM_ENTRY_MAX - 1, 1) == (SPMM_ENTRY_MAX - 1) / TTM + 1 && gemm_tiles_m(~0ull, 17) == ~0ull / TM + 1);
  // the default rule: its work count saturates; no plain mask, two columns
  CHECK(gemm_work(64, 64, 64) == (1ull << 18) && gemm_work(0, 5, 5) == 0 && gemm_work(5, 0, 5) == 0 && gemm_work(5, 5, 0) == 0);
  CHECK(gemm_work(1ull << 31, 1ull << 31, 1ull << 31) == ~0ull && gemm_work(1ull << 32, 1ull << 31, 1) == (1ull << 63) && gemm_work(1ull << 32, 1ull << 32, 1) == ~0ull);
  CHECK(gemm_by_default(1024, 4, 64, false, 1ull << 18) && !gemm_by_default(1024, 4, 63, false, 1ull << 18) && !gemm_by_default(1024, 4, 64, true, 1ull << 18));
  CHECK(!gemm_by_default(1ull << 18, 4, 1, false, 1ull << 18) && gemm_by_default(1ull << 18, 4, 2, false, 1ull << 18) && gemm_by_default(~0ull, ~0ull, ~0ull, false, ~0ull));
  CHECK(gemm_by_default(256, 4, 256, false, 1ull << 18) && !gemm_by_default(255, 4, 255, false, 1ull << 18));
  // ... and GEMM_MIN_TILES tiles of T: 16 wide tiles or 16 tall ones are in, one fewer is out whatever the work
  const uint64_t MT = GEMM_MIN_TILES;
  CHECK(gemm_has_tiles(MT * TM, TN, MT) && !gemm_has_tiles((MT - 1) * TM, TN, MT) && gemm_has_tiles((MT - 1) * TM + 1, TN, MT) && gemm_has_tiles(TM, MT * TN, MT) && !gemm_has_tiles(TM, (MT - 1) * TN, MT));
  CHECK(gemm_has_tiles(MT * TTM, 2, MT) && !gemm_has_tiles(MT * TTM - TTM, NSW, MT) && gemm_has_tiles(4 * TM, 4 * TN, 16) && !gemm_has_tiles(4 * TM, 3 * TN, 16) && gemm_has_tiles(~0ull, ~0ull, MT) && gemm_has_tiles(~0ull, 2, MT));
  CHECK(!gemm_by_default(1024, 256, 16, false, 1ull << 18) && !gemm_by_default(2048, 256, 16, false, 1ull << 18) && gemm_by_default(4096, 256, 16, false, 1ull << 18));      // the measured losses and the first win beside them
  CHECK(!gemm_by_default(64, 64, 64, false, 1ull << 18) && !gemm_by_default(TTM, 64, 16, false, 1ull << 18) && gemm_by_default(1024, 256, 64, false, 1ull << 18));
  printf("gemm geometry ok\n");
  return 0;
}
