// assign_scalar_geometry_check.cpp — stand-alone host check of the region arithmetic of grb_assign_scalar_geom.hpp (the size test of the block I x J against the
// device layout's limit, the count and the sorted form of a range triple, the column slot of a block entry), meant to be built with the address and
// undefined-behaviour sanitizers (host code only) and run on the CPU (tests/test_assign_scalar_model.py does).  Each value is compared with the same quantity
// computed in 128-bit integers or by enumeration.  No device code runs.
#include "grb_assign_scalar_geom.hpp"
#include <stdio.h>
#include <algorithm>
#include <vector>

typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_region(uint64_t nsel, uint64_t ncs) {
  const u128 prod = (u128)nsel * ncs;
  const bool fits = prod <= (u128)grb::SCALAR_REGION_MAX;
  CHECK(grb::scalar_region_fits(nsel, ncs) == fits, "nsel=%llu ncs=%llu", (unsigned long long)nsel, (unsigned long long)ncs);
  CHECK((u128)grb::scalar_region_entries(nsel, ncs) == (fits ? prod : (u128)0), "nsel=%llu ncs=%llu", (unsigned long long)nsel, (unsigned long long)ncs);
}

// a triple over a dimension small enough to enumerate: the indices it names, one by one
static void check_range(bool back, uint64_t b, uint64_t e, uint64_t st, uint64_t dim) {
  std::vector<uint64_t> named;
  if (st != 0) {
    if (back) { if (b >= e) for (uint64_t i = b;; i -= st) { named.push_back(i); if (i < e + st) break; } }
    else for (uint64_t i = b; i <= e; i += st) named.push_back(i);
  }
  const uint64_t n = grb::scalar_range_count(back, b, e, st);
  CHECK(n == named.size(), "back=%d %llu:%llu:%llu count %llu", (int)back, (unsigned long long)b, (unsigned long long)e, (unsigned long long)st, (unsigned long long)n);
  if (!n || n != named.size()) return;
  for (uint64_t i : named) CHECK(i < dim, "index outside the dimension");
  std::sort(named.begin(), named.end());
  CHECK(grb::scalar_range_first(back, b, st, n) == named[0], "back=%d %llu:%llu:%llu first", (int)back, (unsigned long long)b, (unsigned long long)e, (unsigned long long)st);
  for (uint64_t k = 0; k < n; k++)
    CHECK(grb::scalar_range_sorted_at(back, b, st, n, k) == named[k], "back=%d %llu:%llu:%llu sorted[%llu]", (int)back, (unsigned long long)b, (unsigned long long)e, (unsigned long long)st, (unsigned long long)k);
}

// the block of nsel x ncs entries: slot and row pointer against enumeration, the stepping the fill kernel does against the division
static void check_block(uint64_t nsel, uint64_t ncs) {
  if (!ncs) return;
  uint64_t p = 0;
  for (uint64_t r = 0; r < nsel; r++) {
    CHECK(grb::scalar_block_rowptr(r, ncs) == p, "rowptr nsel=%llu ncs=%llu r=%llu", (unsigned long long)nsel, (unsigned long long)ncs, (unsigned long long)r);
    for (uint64_t k = 0; k < ncs; k++, p++) CHECK(grb::scalar_block_slot(p, ncs) == k, "slot p=%llu ncs=%llu", (unsigned long long)p, (unsigned long long)ncs);
  }
  CHECK(grb::scalar_block_rowptr(nsel, ncs) == p, "rowptr end");
  const uint64_t total = nsel * ncs;
  for (uint64_t p0 = 0; p0 < total; p0 += 4) {                                // a lane's group of four: one division, three steps
    uint64_t k = grb::scalar_block_slot(p0, ncs);
    for (uint64_t j = 0; j < 4 && p0 + j < total; j++) { CHECK(k == (p0 + j) % ncs, "step p0=%llu j=%llu ncs=%llu", (unsigned long long)p0, (unsigned long long)j, (unsigned long long)ncs); k = grb::scalar_block_next_slot(k, ncs); }
  }
}

int main() {
  // the boundary products: 65 535^2 fits, 65 536^2 = 2^32 does not; the limit itself and the value after it, as one row, one column and as factorisations
  const uint64_t sides[] = {0, 1, 2, 3, 5, 16, 65535, 65536, 65537, 70000, 0xFFFFFFF0ull / 2, 0xFFFFFFF0ull / 2 + 1, 0xFFFFFFEFull, 0xFFFFFFF0ull, 0xFFFFFFF1ull, 0xFFFFFFFFull,
                            1ull << 32, 1ull << 33, 1ull << 60, UINT64_MAX / 2, UINT64_MAX - 1, UINT64_MAX};
  for (uint64_t a : sides) for (uint64_t b : sides) check_region(a, b);
  CHECK(grb::scalar_region_fits(65535, 65535) && !grb::scalar_region_fits(65536, 65536), "65535^2 / 65536^2");
  CHECK(grb::scalar_region_fits(0xFFFFFFF0ull, 1) && !grb::scalar_region_fits(0xFFFFFFF1ull, 1) && grb::scalar_region_fits(1, 0xFFFFFFF0ull) && !grb::scalar_region_fits(1, 0xFFFFFFF1ull), "the limit");
  CHECK(grb::scalar_region_fits(0x7FFFFFF8ull, 2) && !grb::scalar_region_fits(0x7FFFFFF9ull, 2), "half the limit, twice");
  CHECK(grb::scalar_region_fits(0, UINT64_MAX) && grb::scalar_region_fits(UINT64_MAX, 0) && grb::scalar_region_entries(0, UINT64_MAX) == 0, "an empty side");
  CHECK(!grb::scalar_region_fits(70000, 70000), "70 000^2");
  // ranges: every triple over small dimensions, step 0 and empty directions included
  for (uint64_t dim : {1ull, 2ull, 7ull, 12ull})
    for (uint64_t b = 0; b < dim; b++) for (uint64_t e = 0; e < dim; e++) for (uint64_t st = 0; st <= dim + 1; st++) { check_range(false, b, e, st, dim); check_range(true, b, e, st, dim); }
  CHECK(grb::scalar_range_count(false, 3, 9, 0) == 0 && grb::scalar_range_count(true, 9, 3, 0) == 0, "step 0 names nothing");
  CHECK(grb::scalar_range_count(false, 9, 3, 1) == 0 && grb::scalar_range_count(true, 3, 9, 1) == 0, "the empty directions");
  // ... and at the far end of 64 bits (a triple that names all 2^64 indices cannot pass extract_parse: its end is not below any dimension)
  CHECK(grb::scalar_range_count(false, 0, UINT64_MAX - 1, 1) == UINT64_MAX && grb::scalar_range_count(true, UINT64_MAX - 1, 0, 1) == UINT64_MAX, "the longest range");
  CHECK(grb::scalar_range_count(false, 0, UINT64_MAX, UINT64_MAX) == 2 && grb::scalar_range_count(true, UINT64_MAX, 0, UINT64_MAX) == 2 && grb::scalar_range_count(false, 5, UINT64_MAX, UINT64_MAX) == 1, "the longest step");
  CHECK(grb::scalar_range_first(true, 0xFFFFFFEFull, 3, 5) == 0xFFFFFFEFull - 12 && grb::scalar_range_first(false, 7, 3, 5) == 7 && grb::scalar_range_first(true, 9, 4, 0) == 9, "first");
  // blocks: empty lists, single entries, odd widths, widths around the lane group
  for (uint64_t nsel : {0ull, 1ull, 3ull, 5ull, 37ull}) for (uint64_t ncs : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, 7ull, 29ull, 301ull}) check_block(nsel, ncs);
  printf(failures ? "assign scalar geometry: %d checks failed\n" : "assign scalar geometry ok\n", failures);
  return failures ? 1 : 0;
}
