// tile_geometry_check.cpp — stand-alone host check of the integer geometry of GxB_Matrix_concat / GxB_Matrix_split (grb_tile_geom.hpp, with the row search of
// grb_tuples_geom.hpp the kernels share), meant to be built with the address and undefined-behaviour sanitizers (host code only) and run on the CPU
// (tests/test_tile_host.py does).  It checks the bounds as prefix sums (overflow included), the verdicts on both calls' arguments, the block search at every
// edge, split's flat count layout, and — by replaying the index arithmetic of the two fill kernels entry by entry on small grids — the map from a chunk of
// entries to its tile and row.  No device code runs.
#include "grb_tile_geom.hpp"
#include "grb_tuples_geom.hpp"
#include <stdio.h>
#include <vector>

using namespace grb;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)((rng_state >> 11) % n); }

static void check_bounds_and_verdicts() {
  uint64_t b[5];
  const uint64_t s1[3] = {3, 1, 5};
  CHECK(tile_bounds(s1, 3, b) && b[0] == 0 && b[1] == 3 && b[2] == 4 && b[3] == 9, "prefix sums");
  CHECK(tile_bounds(s1, 0, b) && b[0] == 0, "no blocks");
  const uint64_t big[2] = {~0ull, 1};
  CHECK(!tile_bounds(big, 2, b), "a sum past 2^64 is reported");
  const uint64_t edge[2] = {~0ull - 1, 1};
  CHECK(tile_bounds(edge, 2, b) && b[2] == ~0ull, "a sum of exactly 2^64 - 1 is not");

  uint64_t rb[4], cb[4];
  const uint64_t r2[2] = {2, 3}, c3[3] = {1, 4, 2}, z2[2] = {2, 0};
  CHECK(tile_check_split(2, 3, r2, c3, 5, 7, rb, cb) == TILE_OK && rb[2] == 5 && cb[3] == 7 && cb[1] == 1 && cb[2] == 5, "split ok");
  CHECK(tile_check_split(2, 3, nullptr, c3, 5, 7, rb, cb) == TILE_NULL && tile_check_split(2, 3, r2, nullptr, 5, 7, rb, cb) == TILE_NULL, "split NULL sizes");
  CHECK(tile_check_split(0, 3, r2, c3, 5, 7, rb, cb) == TILE_INVALID && tile_check_split(2, 0, r2, c3, 5, 7, rb, cb) == TILE_INVALID, "split empty grid");
  CHECK(tile_check_split(2, 3, z2, c3, 2, 7, rb, cb) == TILE_INVALID && tile_check_split(2, 2, r2, z2, 5, 2, rb, cb) == TILE_INVALID, "split size 0");
  CHECK(tile_check_split(2, 3, r2, c3, 6, 7, rb, cb) == TILE_MISMATCH && tile_check_split(2, 3, r2, c3, 5, 6, rb, cb) == TILE_MISMATCH, "split sums");
  CHECK(tile_check_split(2, 3, big, c3, 0, 7, rb, cb) == TILE_MISMATCH, "split sum that wraps to A's shape");

  // concat: 2 x 2 grid, shapes row-major
  const uint64_t sr[4] = {2, 2, 3, 3}, sc[4] = {4, 1, 4, 1};
  CHECK(tile_check_concat(2, 2, sr, sc, 5, 5, rb, cb) == TILE_OK && rb[1] == 2 && rb[2] == 5 && cb[1] == 4 && cb[2] == 5, "concat ok");
  CHECK(tile_check_concat(2, 2, sr, sc, 5, 6, rb, cb) == TILE_MISMATCH && tile_check_concat(2, 2, sr, sc, 4, 5, rb, cb) == TILE_MISMATCH, "concat sums");
  const uint64_t sr_bad[4] = {2, 3, 3, 3}, sc_bad[4] = {4, 1, 3, 1};
  CHECK(tile_check_concat(2, 2, sr_bad, sc, 5, 5, rb, cb) == TILE_MISMATCH, "a tile-row's heights differ");
  CHECK(tile_check_concat(2, 2, sr, sc_bad, 5, 5, rb, cb) == TILE_MISMATCH, "a column block's widths differ");
  CHECK(tile_check_concat(0, 2, sr, sc, 0, 5, rb, cb) == TILE_INVALID && tile_check_concat(2, 0, sr, sc, 5, 0, rb, cb) == TILE_INVALID, "concat empty grid");
  CHECK(tile_check_concat(2, 2, nullptr, sc, 5, 5, rb, cb) == TILE_NULL, "concat NULL");
  const uint64_t hr[2] = {~0ull, 1}, hc[2] = {1, 1};
  CHECK(tile_check_concat(2, 1, hr, hc, 0, 1, rb, cb) == TILE_MISMATCH, "concat heights that wrap");
  const uint64_t zr[2] = {0, 0}, zc[2] = {3, 0};
  CHECK(tile_check_concat(1, 2, zr, zc, 0, 3, rb, cb) == TILE_OK && cb[1] == 3 && cb[2] == 3, "concat accepts tiles without rows or columns");
}

static void check_block_search() {
  // every x of every small bounds array against a linear search; empty blocks (concat) are passed over
  for (int trial = 0; trial < 300; trial++) {
    const uint32_t nb = 1 + rnd(9);
    std::vector<uint32_t> bounds(nb + 1, 0);
    for (uint32_t k = 0; k < nb; k++) bounds[k + 1] = bounds[k] + (rnd(4) == 0 ? 0 : 1 + rnd(5));
    std::vector<uint64_t> wide(bounds.begin(), bounds.end());
    for (uint32_t x = 0; x < bounds[nb]; x++) {
      uint32_t want = 0; while (!(bounds[want] <= x && x < bounds[want + 1])) want++;
      CHECK(tile_block_of<uint32_t>(bounds.data(), nb, x) == want, "nb=%u x=%u", nb, x);
      CHECK(tile_block_of<uint64_t>(wide.data(), nb, (uint64_t)x) == want, "64-bit nb=%u x=%u", nb, x);
    }
  }
  const uint32_t top[3] = {0, 0xFFFFFFEFu, 0xFFFFFFF0u};
  CHECK(tile_block_of<uint32_t>(top, 2, 0xFFFFFFEEu) == 0 && tile_block_of<uint32_t>(top, 2, 0xFFFFFFEFu) == 1, "the last column of block 0 and the first of block 1 at the top of the range");
  for (int trial = 0; trial < 200; trial++) {
    const uint32_t len = rnd(12); std::vector<uint32_t> col(len + 1, 0); uint32_t c = 0;
    for (uint32_t k = 0; k < len; k++) { c += 1 + rnd(3); col[k] = c; }
    for (uint32_t lo = 0; lo <= len; lo++) for (uint32_t x = 0; x <= c + 2; x++) {
      uint32_t want = lo; while (want < len && col[want] < x) want++;
      CHECK(tile_lower_bound(col.data(), lo, len, x) == want, "lower bound len=%u lo=%u x=%u", len, lo, x);
    }
  }
}

static void check_chunks() {
  CHECK(tile_chunks(0) == 0 && tile_chunks(1) == 1 && tile_chunks(TILE_CHUNK) == 1 && tile_chunks(TILE_CHUNK + 1) == 2, "chunk count");
  CHECK(tile_grid(0) == 1 && tile_grid(1) == 1 && tile_grid(TILE_GRID_CAP) == TILE_GRID_CAP && tile_grid((uint64_t)TILE_GRID_CAP + 1) == TILE_GRID_CAP, "grid cap");
  const uint64_t nnzs[] = {1, TILE_CHUNK - 1, TILE_CHUNK, TILE_CHUNK + 1, 3ull * TILE_CHUNK + 5, TILE_MAX_ENTRIES};
  for (uint64_t nnz : nnzs) {
    const uint64_t nc = tile_chunks(nnz);
    CHECK(tile_chunk_begin(0) == 0 && tile_chunk_end(nc - 1, nnz) == nnz && tile_chunk_begin(nc - 1) < nnz, "nnz=%llu", (unsigned long long)nnz);
    if (nc > 1) CHECK(tile_chunk_end(0, nnz) == TILE_CHUNK && tile_chunk_begin(1) == TILE_CHUNK, "nnz=%llu", (unsigned long long)nnz);
    CHECK(tile_chunk_end(nc - 1, nnz) - tile_chunk_begin(nc - 1) <= TILE_CHUNK, "the last chunk");
  }
}

// a small CSR: rows of random length (many empty), sorted distinct columns
struct Csr { uint32_t nrows, ncols; std::vector<uint32_t> rp, col; };
static Csr random_csr(uint32_t nrows, uint32_t ncols, uint32_t one_in) {
  Csr A{nrows, ncols, {0}, {}};
  for (uint32_t r = 0; r < nrows; r++) {
    const bool empty = rnd(3) == 0;
    for (uint32_t c = 0; c < ncols && !empty; c++) if (rnd(one_in) == 0) A.col.push_back(c);
    A.rp.push_back((uint32_t)A.col.size());
  }
  return A;
}

// replay k_split_count / the scan / k_split_rowptr / k_split_scatter and then k_concat_count / the scan / k_concat_fill on the tiles: A must come back
static void check_round_trip(uint32_t m, uint32_t n, uint32_t one_in) {
  std::vector<uint32_t> rowb(m + 1, 0), colb(n + 1, 0);
  for (uint32_t a = 0; a < m; a++) rowb[a + 1] = rowb[a] + 1 + rnd(4);
  for (uint32_t b = 0; b < n; b++) colb[b + 1] = colb[b] + 1 + rnd(4);
  const Csr A = random_csr(rowb[m], colb[n], one_in);
  const uint32_t nnz = (uint32_t)A.col.size();
  // split: counts in the flat layout
  const uint64_t npos = (uint64_t)n * A.nrows;
  std::vector<uint32_t> counts(npos + 1, 0xDEADu), S(npos + 1, 0);
  std::vector<int> hit(npos, 0);
  for (uint32_t r = 0; r < A.nrows; r++) {
    const uint32_t a = tile_block_of<uint32_t>(rowb.data(), m, r), nr = rowb[a + 1] - rowb[a], lr = r - rowb[a];
    uint32_t lo = A.rp[r]; const uint32_t hi = A.rp[r + 1];
    for (uint32_t b = 0; b < n; b++) {
      const uint32_t cut = b + 1 < n ? tile_lower_bound(A.col.data(), lo, hi, colb[b + 1]) : hi;
      const uint64_t at = tile_count_base(rowb.data(), n, a, b) + lr;
      CHECK(at == (uint64_t)n * rowb[a] + (uint64_t)b * nr + lr && at < npos, "count position");
      if (at < npos) { hit[at]++; counts[at] = cut - lo; }
      lo = cut;
    }
  }
  for (uint64_t p = 0; p < npos; p++) CHECK(hit[p] == 1, "every flat position is written once (m=%u n=%u pos=%llu)", m, n, (unsigned long long)p);
  counts[npos] = 0;
  for (uint64_t p = 0; p < npos; p++) S[p + 1] = S[p] + counts[p];
  CHECK(S[npos] == nnz, "the counts add up to nnz");
  // the tiles' row pointers through the flat positions
  std::vector<Csr> tiles((size_t)m * n);
  for (uint32_t a = 0; a < m; a++) for (uint32_t b = 0; b < n; b++) {
    Csr& t = tiles[(size_t)a * n + b]; t.nrows = rowb[a + 1] - rowb[a]; t.ncols = colb[b + 1] - colb[b]; t.rp.assign(t.nrows + 1, 0xDEADu);
    const uint64_t base = tile_count_base(rowb.data(), n, a, b);
    t.col.assign(S[base + t.nrows] - S[base], 0xDEADu);
  }
  for (uint64_t pos = 0; pos < npos; pos++) {
    const uint32_t a = tile_count_row_of(rowb.data(), m, n, pos), nr = rowb[a + 1] - rowb[a];
    const uint64_t within = pos - (uint64_t)n * rowb[a];
    const uint32_t b = (uint32_t)(within / nr), lr = (uint32_t)(within - (uint64_t)b * nr);
    CHECK(a < m && b < n && lr < nr && pos - lr == tile_count_base(rowb.data(), n, a, b), "flat position %llu", (unsigned long long)pos);
    Csr& t = tiles[(size_t)a * n + b];
    t.rp[lr] = S[pos] - S[pos - lr];
    if (lr + 1 == nr) t.rp[nr] = S[pos + 1] - S[pos - lr];
  }
  // scatter, chunk by chunk as the kernel brackets its rows
  for (uint64_t c = 0; c < tile_chunks(nnz); c++) {
    const uint64_t base = tile_chunk_begin(c), end = tile_chunk_end(c, nnz);
    const uint32_t rlo = tuples_row_of(A.rp.data(), 0, A.nrows - 1, (uint32_t)base), rhi = tuples_row_from(A.rp.data(), rlo, A.nrows - 1, (uint32_t)(end - 1));
    for (uint32_t e = (uint32_t)base; e < end; e++) {
      const uint32_t r = tuples_row_of(A.rp.data(), rlo, rhi, e), col = A.col[e];
      CHECK(A.rp[r] <= e && e < A.rp[r + 1], "row of entry %u", e);
      const uint32_t b = tile_block_of<uint32_t>(colb.data(), n, col), a = tile_block_of<uint32_t>(rowb.data(), m, r);
      Csr& t = tiles[(size_t)a * n + b];
      const uint32_t first = tile_lower_bound(A.col.data(), A.rp[r], e, colb[b]);
      const uint32_t dst = t.rp[r - rowb[a]] + (e - first);
      CHECK(dst < t.col.size() && dst < t.rp[r - rowb[a] + 1], "scatter target inside its row");
      if (dst < t.col.size()) { CHECK(t.col[dst] == 0xDEADu, "written once"); t.col[dst] = col - colb[b]; }
    }
  }
  for (const Csr& t : tiles) {
    CHECK(t.rp[0] == 0 && t.rp[t.nrows] == t.col.size(), "a tile's row pointer closes");
    for (uint32_t r = 0; r < t.nrows; r++) for (uint32_t p = t.rp[r]; p < t.rp[r + 1]; p++) CHECK(t.col[p] < t.ncols && (p == t.rp[r] || t.col[p - 1] < t.col[p]), "a tile's row is sorted and inside the tile");
  }
  // concat of the tiles
  std::vector<uint32_t> crp(A.nrows + 1, 0);
  for (uint32_t r = 0; r < A.nrows; r++) {
    const uint32_t a = tile_block_of<uint32_t>(rowb.data(), m, r), lr = r - rowb[a]; uint32_t sum = 0;
    for (uint32_t b = 0; b < n; b++) { const Csr& t = tiles[(size_t)a * n + b]; sum += t.rp[lr + 1] - t.rp[lr]; }
    crp[r + 1] = crp[r] + sum;
  }
  CHECK(crp == A.rp, "concat's row pointer is A's");
  for (uint32_t q = 0; q < nnz; q++) {
    const uint32_t r = tuples_row_of(crp.data(), 0, A.nrows - 1, q), a = tile_block_of<uint32_t>(rowb.data(), m, r), lr = r - rowb[a];
    const TileSeg s = tile_segment(n, q - crp[r], [&](uint32_t b) { const Csr& t = tiles[(size_t)a * n + b]; return t.rp[lr + 1] - t.rp[lr]; });
    const Csr& t = tiles[(size_t)a * n + s.b];
    CHECK(s.b < n && s.left >= 1 && s.at + s.left == t.rp[lr + 1] - t.rp[lr], "segment of entry %u", q);
    CHECK(t.col[t.rp[lr] + s.at] + colb[s.b] == A.col[q], "entry %u comes back", q);
  }
}

int main() {
  check_bounds_and_verdicts();
  check_block_search();
  check_chunks();
  for (int trial = 0; trial < 40; trial++) check_round_trip(1 + rnd(4), 1 + rnd(6), 1 + rnd(3));
  check_round_trip(1, 1, 1); check_round_trip(1, 9, 2); check_round_trip(7, 1, 2);
  check_round_trip(40, 30, 1);                                               // several chunks: rows bracketed per chunk
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("tile geometry ok\n");
  return 0;
}
