// diag_geometry_check.cpp — stand-alone host check of the diagonal geometry of grb_diag.hpp (diag_len, diag_row0 / diag_col0, diag_dim, diag_rowptr_at), meant to be
// built with the address and undefined-behaviour sanitizers (host code only) and run on the CPU (tests/test_diag_host.py does): the helpers must not overflow for any int64 k.
// Each value is compared with the same quantity computed in 128-bit integers.  No device code runs.
#include "grb_diag.hpp"
#include <stdio.h>
#include <vector>

typedef __int128 i128;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_shape(uint64_t m, uint64_t n, int64_t k) {
  const i128 K = k, r0 = K < 0 ? -K : 0, c0 = K < 0 ? 0 : K;
  i128 len = 0;
  if (r0 < (i128)m && c0 < (i128)n) { const i128 a = (i128)m - r0, b = (i128)n - c0; len = a < b ? a : b; }
  CHECK((i128)grb::diag_abs(k) == (K < 0 ? -K : K), "k=%lld", (long long)k);
  CHECK((i128)grb::diag_row0(k) == r0 && (i128)grb::diag_col0(k) == c0, "k=%lld", (long long)k);
  CHECK((i128)grb::diag_len(m, n, k) == len, "m=%llu n=%llu k=%lld: %llu", (unsigned long long)m, (unsigned long long)n, (long long)k, (unsigned long long)grb::diag_len(m, n, k));
}

static void check_vector(uint64_t n_v, int64_t k) {
  const i128 K = k, ak = K < 0 ? -K : K, dim = (i128)n_v + ak;
  uint64_t n = 0; const bool ok = grb::diag_dim(n_v, k, &n);
  CHECK(ok == (dim <= (i128)UINT64_MAX) && (!ok || (i128)n == dim), "n_v=%llu k=%lld", (unsigned long long)n_v, (long long)k);
  if (!ok || n > 4096) return;                                             // the row pointer of what can be enumerated
  // presence: every second position; scan[r] = entries before r
  std::vector<uint32_t> scan(n_v + 1, 0);
  for (uint64_t r = 0; r < n_v; r++) scan[r + 1] = scan[r] + (r % 2 == 0 ? 1u : 0u);
  const uint64_t total = scan[n_v];
  std::vector<uint64_t> count(n + 1, 0);                                   // entries per row from the positions themselves
  for (uint64_t r = 0; r < n_v; r++) if (r % 2 == 0) { const uint64_t row = r + grb::diag_row0(k), col = r + grb::diag_col0(k); CHECK(row < n && col < n, "entry outside the matrix"); count[row]++; }
  uint64_t before = 0;
  for (uint64_t row = 0; row <= n; row++) {
    CHECK(grb::diag_rowptr_at(row, n_v, k, total, scan.data()) == before, "n_v=%llu k=%lld row=%llu", (unsigned long long)n_v, (long long)k, (unsigned long long)row);
    CHECK(grb::diag_rowptr_at(row, n_v, k, n_v, nullptr) == (row < grb::diag_row0(k) ? 0 : (row - grb::diag_row0(k) < n_v ? row - grb::diag_row0(k) : n_v)), "all present: row=%llu", (unsigned long long)row);
    if (row < n) before += count[row];
  }
  CHECK(before == total, "row pointer total");
}

int main() {
  const uint64_t dims[] = {0, 1, 5, 7, 64, 300, 1025, 0xFFFFFFF0ull, 1ull << 60, UINT64_MAX};
  for (uint64_t m : dims) for (uint64_t n : dims) {
    const int64_t ks[] = {INT64_MIN, INT64_MIN + 1, -(int64_t)(n & INT64_MAX), -(int64_t)(m & INT64_MAX), -(int64_t)(m & INT64_MAX) + 1, -5, -1, 0, 1, 5, (int64_t)(n & INT64_MAX), (int64_t)(n & INT64_MAX) - 1,
                          (int64_t)(m & INT64_MAX), INT64_MAX - 1, INT64_MAX};
    for (int64_t k : ks) check_shape(m, n, k);
  }
  for (uint64_t n_v : dims) {
    const int64_t ks[] = {INT64_MIN, INT64_MIN + 1, -(int64_t)(n_v & INT64_MAX), -5, -1, 0, 1, 5, (int64_t)(n_v & INT64_MAX), INT64_MAX};
    for (int64_t k : ks) check_vector(n_v, k);
  }
  printf(failures ? "diag geometry: %d checks failed\n" : "diag geometry ok\n", failures);
  return failures ? 1 : 0;
}
