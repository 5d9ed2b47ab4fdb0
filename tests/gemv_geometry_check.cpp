// gemv_geometry_check.cpp — grb_gemv_geom.hpp on its own (plain integers, host code only): the kernels' index maps replayed on the host.  Layout N: the groups of
// the short-row kernel and the (row, chunk) units, lanes and packets of the wave kernel cover [0, m) x [0, k) exactly once, for every value size; layout T: the
// (slab, chunk) units, the waves' pieces and the lanes' columns do; the scratch slots of either layout never overlap and fill [0, m chunks); the grid-stride walks
// under the cap visit every unit once; the work counts saturate near 2^64; the default rule.  Built with the address and undefined-behaviour sanitizers by
// tests/test_gemv_full_host.py; prints "gemv geometry ok".  With arguments `rows cols transposed` it prints instead what the library's rule says of that matrix:
// "rule <0|1> min_work <GEMV_FULL_MIN_WORK>".
#include "grb_gemv_geom.hpp"
#include "grb_route.hpp"          // GEMV_FULL_MIN_WORK
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// exactly m k bytes (or m chunks): the address sanitizer sees a store outside
struct Cells {
  uint8_t* p; uint64_t n;
  explicit Cells(uint64_t n_) : p((uint8_t*)calloc(n_ ? n_ : 1, 1)), n(n_) {}
  ~Cells() { free(p); }
  void hit(uint64_t at) { CHECK(at < n); CHECK(p[at] == 0); p[at] = 1; }
  void all() const { for (uint64_t e = 0; e < n; e++) CHECK(p[e] == 1); }
};

// layout N, k <= GEMV_N_GROUP_MAX: the kernel's loop — workgroup b takes rows r0 = b per_wg, + grid per_wg ..., thread t row r0 + t / G and product t % G
static void check_n_short(uint64_t m, uint64_t k) {
  CHECK(gemv_n_short(k) && gemv_chunks(GEMV_N, k) == 1);
  const uint32_t G = gemv_group(k), per_wg = gemv_rows_per_workgroup(k), threads = GEMV_WAVES * 64;
  CHECK(G >= k && (G & (G - 1)) == 0 && (G == 1 || G / 2 < k) && G <= 64 && per_wg * G == threads && gemv_rows_per_wave(k) * G == 64);
  const uint32_t grid = gemv_grid(m, per_wg);
  CHECK(grid >= 1 && grid <= GEMV_GRID_CAP);
  Cells cell(m * k);
  for (uint32_t b = 0; b < grid; b++)
    for (uint64_t r0 = (uint64_t)b * per_wg; r0 < m; r0 += (uint64_t)grid * per_wg)
      for (uint32_t t = 0; t < threads; t++) {
        const uint64_t i = r0 + t / G; const uint32_t g = t % G;
        if (i < m && g < k) cell.hit(i * k + g);
      }
  cell.all();
}

// layout N, longer rows: a wave per unit, lane g the packets g, g + 64, ... of the chunk; slots
static void check_n_wave(uint64_t m, uint64_t k, uint32_t size) {
  CHECK(!gemv_n_short(k));
  const uint64_t chunks = gemv_chunks(GEMV_N, k), units = m * chunks, V = gemv_vec(size);
  CHECK(chunks == (k + GEMV_N_CHUNK - 1) / GEMV_N_CHUNK && V * size <= GEMV_LOAD_BYTES && V <= GEMV_MAX_PACK && (V == GEMV_MAX_PACK || V * size == GEMV_LOAD_BYTES));
  const uint32_t grid = gemv_grid(gemv_mul_sat(m, chunks), GEMV_WAVES);
  Cells cell(m * k), slot(units);
  for (uint32_t b = 0; b < grid; b++)
    for (uint32_t w = 0; w < GEMV_WAVES; w++)
      for (uint64_t unit = (uint64_t)b * GEMV_WAVES + w; unit < units; unit += (uint64_t)grid * GEMV_WAVES) {
        const uint64_t i = unit / chunks, c = unit % chunks, l0 = gemv_n_chunk_begin(c), l1 = gemv_n_chunk_end(k, c);
        CHECK(l0 < l1 && l1 <= k && l1 - l0 <= GEMV_N_CHUNK && (l1 == k || l1 - l0 == GEMV_N_CHUNK) && l0 % (64 * V) == 0);
        for (uint32_t lane = 0; lane < 64; lane++) {
          uint64_t l = l0 + lane * V;
          const uint64_t STEP = 64 * V;
          for (; l + (GEMV_N_UNROLL - 1) * STEP + V <= l1; l += GEMV_N_UNROLL * STEP)                 // the unrolled loop: whole packets only
            for (uint32_t r = 0; r < GEMV_N_UNROLL; r++) for (uint64_t e = 0; e < V; e++) cell.hit(i * k + l + r * STEP + e);
          for (; l < l1; l += STEP) { const uint64_t n = l1 - l < V ? l1 - l : V; for (uint64_t e = 0; e < n; e++) cell.hit(i * k + l + e); }
        }
        slot.hit(gemv_slot(GEMV_N, i, c, m, chunks));
      }
  cell.all(); slot.all();
}

// layout T: A is k x m; a workgroup per (slab, chunk) unit, wave w piece w of the chunk's rows, lane g the columns (64 slab + g) VT ...
static void check_t(uint64_t m, uint64_t k, uint32_t size) {
  const uint64_t chunks = gemv_chunks(GEMV_T, k), slabs = gemv_t_slabs(m, size), VT = gemv_t_vt(m, size), rt = gemv_t_chunk(k);
  CHECK((VT == 1 || (VT == gemv_vec(size) && m % VT == 0)) && gemv_t_slab(m, size) == 64 * VT && slabs == (m + 64 * VT - 1) / (64 * VT));
  CHECK(rt >= GEMV_T_CHUNK && (rt & (rt - 1)) == 0 && chunks == (k + rt - 1) / rt && chunks <= GEMV_T_MAX_CHUNKS && gemv_t_piece(k) * GEMV_WAVES == rt);
  const uint64_t units = slabs * chunks;
  const uint32_t grid = gemv_grid(gemv_mul_sat(slabs, chunks), 1);
  Cells cell(m * k), slot(m * chunks);
  for (uint32_t b = 0; b < grid; b++)
    for (uint64_t unit = b; unit < units; unit += grid) {
      const uint64_t c = unit / slabs, slab = unit % slabs;
      uint64_t at = c * rt < k ? c * rt : k;
      for (uint32_t w = 0; w < GEMV_WAVES; w++) {                                    // the pieces: consecutive, ascending, inside the chunk
        const uint64_t pb = gemv_t_piece_begin(k, c, w), pe = gemv_t_piece_end(k, c, w);
        CHECK(pb == at && pe >= pb && pe <= k && pe - pb <= gemv_t_piece(k)); at = pe;
        for (uint32_t lane = 0; lane < 64; lane++) {
          const uint64_t j0 = (slab * 64 + lane) * VT;
          if (j0 >= m) continue;
          CHECK(j0 + VT <= m);                                                       // a packet is whole
          for (uint64_t l = pb; l < pe; l++) for (uint64_t v = 0; v < VT; v++) cell.hit(l * m + j0 + v);
        }
      }
      CHECK(at == ((c + 1) * rt < k ? (c + 1) * rt : k));
      for (uint32_t lane = 0; lane < 64; lane++) { const uint64_t j0 = (slab * 64 + lane) * VT; if (j0 < m) for (uint64_t v = 0; v < VT; v++) slot.hit(gemv_slot(GEMV_T, j0 + v, c, m, chunks)); }
    }
  cell.all(); slot.all();
}

int main(int argc, char** argv) {
  if (argc == 4) {                                                                   // the default rule as the library compiles it, for the host test
    printf("rule %d min_work %llu\n", (int)gemv_by_default(strtoull(argv[1], 0, 10), strtoull(argv[2], 0, 10), atoi(argv[3]) != 0, GEMV_FULL_MIN_WORK), (unsigned long long)GEMV_FULL_MIN_WORK);
    return 0;
  }
  const uint64_t L = GEMV_N_CHUNK, GM = GEMV_N_GROUP_MAX, CAP = GEMV_GRID_CAP, RT = GEMV_T_CHUNK;
  CHECK(GEMV_LOAD_BYTES == 16 && GM == 64 && L % (64 * 16) == 0 && GEMV_WAVES >= 1 && GEMV_WAVES <= 16);
  // N, short rows: around every group size, around the rows of a wave and of a workgroup, and past one grid round
  for (uint64_t k : std::vector<uint64_t>{1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64})
    for (uint64_t m : std::vector<uint64_t>{1, 2, gemv_rows_per_wave(k) - 1 ? gemv_rows_per_wave(k) - 1 : 1, gemv_rows_per_wave(k), gemv_rows_per_wave(k) + 1, gemv_rows_per_workgroup(k) - 1,
                                            gemv_rows_per_workgroup(k), gemv_rows_per_workgroup(k) + 1, 3 * gemv_rows_per_workgroup(k) + 1}) check_n_short(m, k);
  check_n_short(CAP * gemv_rows_per_workgroup(1) + 1, 1); check_n_short(CAP * gemv_rows_per_workgroup(64) + 1, 64);
  CHECK(gemv_group(0) == 1 && gemv_group(1) == 1 && gemv_group(2) == 2 && gemv_group(3) == 4 && gemv_group(33) == 64 && gemv_group(64) == 64 && gemv_group(~0ull) == 64);
  // N, a wave per (row, chunk): every value size, around a packet, a wave's round of packets, the unrolled step and the chunk
  for (uint32_t size : {1u, 2u, 4u, 8u}) {
    const uint64_t V = gemv_vec(size), R = 64 * V, U = GEMV_N_UNROLL * R;
    for (uint64_t k : std::vector<uint64_t>{65, 66, R - 1, R, R + 1, R + V - 1, R + V, R + V + 1, U - 1, U, U + 1, 2 * U + V + 1, L - 1, L, L + 1, 2 * L + 1})
      if (k > GM) for (uint64_t m : std::vector<uint64_t>{1, 3, GEMV_WAVES + 1}) check_n_wave(m, k, size);
  }
  check_n_wave(CAP * GEMV_WAVES + 1, 65, 4); check_n_wave(CAP + 3, 2 * L + 1, 8);      // past one grid round
  CHECK(gemv_n_chunks(L) == 1 && gemv_n_chunks(L + 1) == 2 && gemv_n_chunks(~0ull) == ~0ull / L + 1 && gemv_n_chunk_end(~0ull, ~0ull / L) == ~0ull);
  // T: columns around the slab of either packet width, rows around the chunk and its pieces, longer chunks for long columns, more units than the cap
  for (uint32_t size : {1u, 4u, 8u}) {
    const uint64_t V = gemv_vec(size);
    for (uint64_t m : std::vector<uint64_t>{1, 2, 63, 64, 65, 64 * V - V, 64 * V, 64 * V + V, 64 * V + 1, 128 * V + 3})
      for (uint64_t k : std::vector<uint64_t>{1, 2, RT / GEMV_WAVES, RT / GEMV_WAVES + 1, RT - 1, RT, RT + 1, 2 * RT + 1}) check_t(m, k, size);
  }
  const uint64_t KM = (uint64_t)RT * GEMV_T_MAX_CHUNKS;                                // the longest column with the shortest chunks
  check_t(3, KM, 4); check_t(3, KM + 1, 4); check_t(2, 4 * KM + 5, 8);
  CHECK(gemv_t_chunk(KM) == RT && gemv_t_chunk(KM + 1) == 2 * RT && gemv_t_chunks(KM + 1) == GEMV_T_MAX_CHUNKS / 2 + 1 && gemv_t_chunk(1ull << 40) == (1ull << 40) / GEMV_T_MAX_CHUNKS);
  check_t(64 * (CAP + 1) + 1, 1, 8); check_t(65, (CAP / 2 + 1) * RT, 4);               // more (slab, chunk) units than the grid cap: CAP + 2 slabs; 2 slabs x CAP / 2 + 1 chunks
  CHECK(gemv_t_slabs(64 * (CAP + 1) + 1, 8) * gemv_t_chunks(1) > CAP && gemv_grid(gemv_t_slabs(64 * (CAP + 1) + 1, 8), 1) == CAP);
  CHECK(gemv_t_chunks(1ull << 63) == GEMV_T_MAX_CHUNKS && gemv_t_piece_end(1ull << 63, GEMV_T_MAX_CHUNKS - 1, GEMV_WAVES - 1) == 1ull << 63 && gemv_t_piece_end(~0ull, gemv_t_chunks(~0ull) - 1, GEMV_WAVES - 1) == ~0ull);
  // work counts near 2^64
  CHECK(gemv_mul_sat(1ull << 32, 1ull << 32) == ~0ull && gemv_mul_sat(1ull << 32, (1ull << 32) - 1) == ((1ull << 32) - 1) << 32 && gemv_mul_sat(~0ull, 1) == ~0ull && gemv_mul_sat(~0ull, 2) == ~0ull);
  CHECK(gemv_mul_sat(0, ~0ull) == 0 && gemv_mul_sat(~0ull, 0) == 0 && gemv_work(1ull << 63, 2) == ~0ull && gemv_work(3, 5) == 15);
  CHECK(gemv_grid(0, 4) == 1 && gemv_grid(~0ull, 4) == CAP && gemv_grid(~0ull, 1) == CAP && gemv_grid(4 * CAP, 4) == CAP && gemv_grid(4 * CAP - 4, 4) == CAP - 1 && gemv_ceil_div(~0ull, 1) == ~0ull);
  // the default rule: not transposed, rows of at least GEMV_DEFAULT_MIN_INNER values, rows cols >= min_work
  const uint64_t MI = GEMV_DEFAULT_MIN_INNER;
  CHECK(gemv_by_default(256, MI, false, 1ull << 24) && !gemv_by_default(255, MI, false, 1ull << 24) && !gemv_by_default(256, MI, true, 1ull << 24) && !gemv_by_default(1ull << 20, MI - 1, false, 1ull << 24));
  CHECK(!gemv_by_default(1ull << 20, 64, false, 1ull << 24) && !gemv_by_default(16, 1ull << 16, false, 1ull << 24) && gemv_by_default(16, 1ull << 20, false, 1ull << 24) && gemv_by_default(16, 1ull << 22, false, 1ull << 24));      // measured losses and wins
  CHECK(!gemv_by_default(0, ~0ull, false, 1) && !gemv_by_default(~0ull, 0, false, 1) && gemv_by_default(~0ull, ~0ull, false, ~0ull) && gemv_by_default(1ull << 40, 1ull << 40, false, ~0ull) && !gemv_by_default(1ull << 31, 1ull << 32, false, ~0ull));
  printf("gemv geometry ok\n");
  return 0;
}
