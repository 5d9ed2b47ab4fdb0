// spmm_geometry_check.cpp — grb_spmm_geom.hpp on its own (plain integers, host code only): the group width for every k from 1 to 130, the slab counts and the
// chunk counts at their edges, the chunks of a row covering its entries exactly once, the scratch slots of the long rows (consecutive per row, no two rows sharing
// one, all inside the allocation) for row pointers with long rows back to back, T's row pointer against a loop for patterns with the first, the last, all and no
// rows empty, the overflow test around 2^32 - 16 and the fullness test.  Built with the address and undefined-behaviour sanitizers by
// tests/test_spmm_full_host.py; prints "spmm geometry ok".
#include "grb_spmm_geom.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// rows given by their lengths: every long row's chunks cover its entries once and in order, and its slots are its own
static void check_slots(const std::vector<uint32_t>& len) {
  const uint32_t nrows = (uint32_t)len.size();
  std::vector<uint32_t> rowptr(nrows + 1, 0);
  for (uint32_t r = 0; r < nrows; r++) rowptr[r + 1] = rowptr[r] + len[r];
  uint64_t nlong = 0; for (uint32_t r = 0; r < nrows; r++) nlong += spmm_long(len[r]);
  const uint64_t nslots = spmm_slots(rowptr[nrows], nlong);
  CHECK((nslots == 0) == (nlong == 0));
  uint8_t* owner = (uint8_t*)calloc(nslots ? nslots : 1, 1);             // exactly nslots bytes: the address sanitizer sees a slot outside
  uint32_t q = 0; uint64_t last = 0; bool any = false;
  for (uint32_t r = 0; r < nrows; r++) {
    const uint32_t nch = spmm_chunks(len[r]);
    CHECK((nch != 0) == spmm_long(len[r]));
    if (!nch) continue;
    const uint32_t base = spmm_slot_base(rowptr[r], q);
    CHECK(!any || base > last);                                          // behind the previous long row's run
    uint32_t at = rowptr[r];
    for (uint32_t c = 0; c < nch; c++) {
      CHECK((uint64_t)base + c < nslots); CHECK(owner[base + c] == 0); owner[base + c] = 1;
      const uint32_t b = spmm_chunk_begin(rowptr[r], c), e = spmm_chunk_end(rowptr[r], rowptr[r + 1], c);
      CHECK(b == at && e > b && e - b <= SPMM_L && (c + 1 == nch) == (e == rowptr[r + 1]));
      at = e;
    }
    CHECK(at == rowptr[r + 1]);
    last = (uint64_t)base + nch - 1; any = true; q++;
  }
  CHECK(q == nlong);
  free(owner);
}

// T's row pointer: k times the non-empty rows in front, against a loop
static void check_rowptr(const std::vector<uint32_t>& len, uint32_t k) {
  uint64_t before = 0, walk = 0;
  for (size_t r = 0; r <= len.size(); r++) {
    CHECK(spmm_rowptr(before, k) == walk);
    if (r < len.size() && len[r]) { before++; walk += k; }
  }
  CHECK(spmm_overflows(before, k) == (walk >= 0xFFFFFFF0ull));
}

int main() {
  const uint32_t L = SPMM_L, S = SPMM_SLAB;
  CHECK(L >= 2 && S % 64 == 0 && SPMM_WAVES >= 1 && SPMM_GRID_CAP >= 1 && SPMM_NARROW_MAX == 64);
  // the group width: the power of two >= k, a divisor of the wave
  for (uint32_t k = 1; k <= 130; k++) {
    CHECK(spmm_narrow(k) == (k <= 64));
    if (spmm_narrow(k)) {
      const uint32_t g = spmm_group(k);
      CHECK(g >= k && (g & (g - 1)) == 0 && (g == 1 || g / 2 < k) && 64 % g == 0);
      CHECK(spmm_pieces_per_workgroup(k) == SPMM_WAVES * (64 / g));
    } else CHECK(spmm_pieces_per_workgroup(k) == SPMM_WAVES);
    uint32_t slabs = 0; for (uint32_t c = 0; c < k; c += S) slabs++;
    CHECK(spmm_slabs(k) == slabs);
  }
  CHECK(spmm_group(1) == 1 && spmm_group(2) == 2 && spmm_group(3) == 4 && spmm_group(33) == 64 && spmm_group(64) == 64);
  // slabs at the edges
  CHECK(spmm_slabs(S - 1) == 1 && spmm_slabs(S) == 1 && spmm_slabs(S + 1) == 2 && spmm_slabs(2 * S) == 2 && spmm_slabs(2 * S + 1) == 3);
  // chunks at the edges: a row of at most L entries is not cut
  CHECK(spmm_chunks(0) == 0 && spmm_chunks(1) == 0 && spmm_chunks(L - 1) == 0 && spmm_chunks(L) == 0);
  CHECK(spmm_chunks(L + 1) == 2 && spmm_chunks(2 * L) == 2 && spmm_chunks(2 * L + 1) == 3 && spmm_chunks(0xFFFFFFF0u) == (uint32_t)((0xFFFFFFF0ull + L - 1) / L));
  CHECK(!spmm_long(L) && spmm_long(L + 1));
  CHECK(spmm_chunk_end(0xFFFFFF00u, 0xFFFFFFF0u, 0) == 0xFFFFFFF0u);                     // (the last chunk of a matrix at the layout's limit: no 32-bit wrap)
  // the grid
  CHECK(spmm_grid(0, 4) == 1 && spmm_grid(4, 4) == 1 && spmm_grid(5, 4) == 2 && spmm_grid((uint64_t)SPMM_GRID_CAP * 4, 4) == SPMM_GRID_CAP && spmm_grid((uint64_t)SPMM_GRID_CAP * 4 + 1, 4) == SPMM_GRID_CAP);
  CHECK(spmm_grid(~0ull / 2, 1) == SPMM_GRID_CAP);
  // slots
  check_slots({});
  check_slots({0, 1, L, L - 1});
  check_slots({L + 1});
  check_slots({L + 1, L + 1, L + 1, 2 * L + 1, 2 * L, 4 * L, 1, L + 1});
  check_slots({1, L + 1, 0, 0, 2 * L + 1, L - 1, L + 1, 3, 10 * L + 7, L + 1, L + 1});
  check_slots({L - 1, 2 * L, 1, 2 * L, 1, 2 * L});
  for (uint32_t off = 0; off < L; off += 37) check_slots({off, L + 1, L + 1, 2 * L - 1, L + 2, 5 * L + off});
  // T's row pointer: first, last, all and no rows empty
  for (uint32_t k : {1u, 3u, 64u, 65u, S + 1}) {
    check_rowptr({0, 2, 5, 1}, k); check_rowptr({2, 5, 1, 0}, k); check_rowptr({0, 0, 0, 0}, k); check_rowptr({1, 2, 3, 4}, k);
    check_rowptr({0, 2, 0, 0, L + 1, 0}, k); check_rowptr({}, k);
  }
  // the overflow test around 2^32 - 16
  const uint64_t E = 1ull << 32;
  CHECK(!spmm_overflows(E - 17, 1) && spmm_overflows(E - 16, 1) && spmm_overflows(E - 15, 1));
  CHECK(!spmm_overflows(1, E - 17) && spmm_overflows(1, E - 16) && spmm_overflows(1, E - 15));
  CHECK(!spmm_overflows((E - 16) / 16 - 1, 16) && spmm_overflows((E - 16) / 16, 16) && spmm_overflows(~0ull, ~0ull) && !spmm_overflows(0, 7) && !spmm_overflows(7, 0));
  // full: every position holds an entry (and there is a position)
  CHECK(spmm_is_full(3, 4, 12) && !spmm_is_full(3, 4, 11) && !spmm_is_full(3, 4, 8) && !spmm_is_full(0, 4, 0) && !spmm_is_full(4, 0, 0) && spmm_is_full(1, 1, 1));
  CHECK(spmm_is_full(65536, 65535, 65536ull * 65535) && !spmm_is_full(1ull << 40, 1ull << 40, 0));
  printf("spmm geometry ok\n");
  return 0;
}
