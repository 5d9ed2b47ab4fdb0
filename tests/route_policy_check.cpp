// route_policy_check.cpp — grb_route.hpp on its own (plain integers, host code only): the two policy functions against the predicates they replaced, written
// out here as they stood before the routes shared one policy (one expression per family), over every combination of the hook, the device, legality, a list in
// HBM, residency, a known count and the counts around each of the ten thresholds; and every threshold against its value.  Built with the address and
// undefined-behaviour sanitizers by tests/test_route_host.py; prints "route policy ok".
#include "grb_route.hpp"
#include "grb_build_keys.hpp"
#include <stdio.h>
#include <stdlib.h>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// how every caller joins the two stages (the second is evaluated only when the first left it to the size)
static bool taken(RouteStep s, bool by_size) { return s == ROUTE_BY_SIZE ? by_size : s == ROUTE_DEVICE; }

// ---- the predicates as they were, one per family.  env: the hook (-1 unset); dev: device_ok(); cap: every container has an HBM layout (with the family's own
// bitmap-only test folded in); forced: a list of the call lies in HBM; hbm: the deciding container has dev_valid && !host_valid; known: its host_valid ----
static bool old_extract(int env, bool dev, bool cap, bool forced, bool hbm, bool known, uint64_t e, uint64_t min) {
  if (env == 0 || !dev || !cap) return false;
  if (env == 1 || forced) return true;
  if (hbm) return true;
  return known && e >= min;
}
// (C's count is taken as it is; the operand's count `e2` is asked only if C's did not suffice)
static bool old_assign(int env, bool dev, bool cap, bool forced, bool hbm, uint64_t e, uint64_t e2, uint64_t min) {
  if (env == 0 || !dev || !cap) return false;
  if (env == 1 || forced) return true;
  if (hbm) return true;
  return e >= min || e2 >= min;
}
// (`extra`: kronecker's own legality — no aliasing, a mask object with a complemented mask, the product within the 32-bit layout; `hbm`: C or an operand lives in HBM only)
static bool old_kron(int env, bool dev, bool cap, bool extra, bool hbm, uint64_t product, uint64_t min) {
  if (env == 0 || !dev || !cap) return false;
  if (!extra) return false;
  if (env == 1) return true;
  if (hbm) return true;
  return product >= min;
}
static bool old_diag(int env, bool dev, bool cap, bool hbm, bool known, uint64_t e, uint64_t min) {
  if (env == 0 || !dev || !cap) return false;
  if (env == 1) return true;
  if (hbm) return true;
  return known && e >= min;
}
// (`prim`: GRB_MI355X_SORT=prim reads as "unset" for the route)
static bool old_sort(int env, bool prim, bool dev, bool cap, bool hbm, bool known, uint64_t e, uint64_t min) {
  if (prim) env = -1;
  if (env == 0 || !dev || !cap) return false;
  if (env == 1 || hbm) return true;
  return known && e >= min;
}

// ---- the same decisions as the callers make them now ----
static bool new_extract(int env, bool dev, bool cap, bool forced, bool hbm, bool known, uint64_t e, uint64_t min) {
  return taken(route_first(env, dev, cap, forced), route_by_size(hbm, known, known ? e : 0, min));
}
static bool new_assign(int env, bool dev, bool cap, bool forced, bool hbm, uint64_t e, uint64_t e2, uint64_t min) {
  return taken(route_first(env, dev, cap, forced), route_by_size(hbm, true, hbm ? 0 : e, min) || route_by_size(false, true, e2, min));
}
static bool new_kron(int env, bool dev, bool cap, bool extra, bool hbm, uint64_t product, uint64_t min) {
  const RouteStep s = route_first(env, dev, cap, false);
  if (s == ROUTE_HOST || !extra) return false;
  return s == ROUTE_DEVICE || route_by_size(hbm, true, product, min);
}
static bool new_diag(int env, bool dev, bool cap, bool hbm, bool known, uint64_t e, uint64_t min) {
  return taken(route_first(env, dev, cap, false), route_by_size(hbm, known, known ? e : 0, min));
}
static bool new_sort(int env, bool prim, bool dev, bool cap, bool hbm, bool known, uint64_t e, uint64_t min) {
  return taken(route_first(prim ? -1 : env, dev, cap, false), route_by_size(hbm, known, known ? e : 0, min));
}

int main() {
  // the thresholds: every value as it is today
  CHECK(EXTRACT_DEVICE_MIN_ENTRIES == 10000 && ASSIGN_DEVICE_MIN_ENTRIES == 30000 && ASSIGN_ROW_DEVICE_MIN_ENTRIES == 3000000 && ASSIGN_COL_DEVICE_MIN_ENTRIES == 100000);
  CHECK(ASSIGN_VEC_DEVICE_MIN_ENTRIES == 500 && KRON_DEVICE_MIN_ENTRIES == 1000 && DIAG_MATRIX_DEVICE_MIN_ENTRIES == 1000 && DIAG_VECTOR_DEVICE_MIN_ENTRIES == 10000);
  CHECK(SORT_DEVICE_MIN_ENTRIES == 10000 && SORT_DEVICE_MIN_ENTRIES == EXTRACT_DEVICE_MIN_ENTRIES && BUILD_DEVICE_MIN_TUPLES == 10000);
  // the first stage by itself
  CHECK(route_first(0, true, true, true) == ROUTE_HOST && route_first(1, false, true, true) == ROUTE_HOST && route_first(1, true, false, true) == ROUTE_HOST);
  CHECK(route_first(1, true, true, false) == ROUTE_DEVICE && route_first(-1, true, true, true) == ROUTE_DEVICE && route_first(-1, true, true, false) == ROUTE_BY_SIZE);
  CHECK(route_by_size(true, false, 0, 1ull << 40) && !route_by_size(false, false, ~0ull, 1) && route_by_size(false, true, 7, 7) && !route_by_size(false, true, 6, 7));

  const uint64_t mins[] = {EXTRACT_DEVICE_MIN_ENTRIES, ASSIGN_DEVICE_MIN_ENTRIES, ASSIGN_ROW_DEVICE_MIN_ENTRIES, ASSIGN_COL_DEVICE_MIN_ENTRIES, ASSIGN_VEC_DEVICE_MIN_ENTRIES,
                           KRON_DEVICE_MIN_ENTRIES, DIAG_MATRIX_DEVICE_MIN_ENTRIES, DIAG_VECTOR_DEVICE_MIN_ENTRIES, SORT_DEVICE_MIN_ENTRIES, BUILD_DEVICE_MIN_TUPLES};
  const int envs[] = {-1, 0, 1};
  unsigned long cases = 0;
  for (uint64_t min : mins) for (int env : envs) for (int dev = 0; dev < 2; dev++) for (int cap = 0; cap < 2; cap++) for (int forced = 0; forced < 2; forced++)
    for (int hbm = 0; hbm < 2; hbm++) for (int known = 0; known < 2; known++) for (uint64_t e : {(uint64_t)0, min - 1, min, min + 1}) {
      CHECK(new_extract(env, dev, cap, forced, hbm, known, e, min) == old_extract(env, dev, cap, forced, hbm, known, e, min));
      CHECK(new_diag(env, dev, cap, hbm, known, e, min) == old_diag(env, dev, cap, hbm, known, e, min));
      for (int prim = 0; prim < 2; prim++) CHECK(new_sort(env, prim, dev, cap, hbm, known, e, min) == old_sort(env, prim, dev, cap, hbm, known, e, min));
      // (for kronecker `forced` enumerates its own legality tests; for assign `known` has no say and the operand's count takes the four values too)
      CHECK(new_kron(env, dev, cap, forced, hbm, e, min) == old_kron(env, dev, cap, forced, hbm, e, min));
      for (uint64_t e2 : {(uint64_t)0, min - 1, min, min + 1}) CHECK(new_assign(env, dev, cap, forced, hbm, e, e2, min) == old_assign(env, dev, cap, forced, hbm, e, e2, min));
      // build-from-tuples (grb_build_keys.hpp, unchanged) is the same policy: legality in one flag, no list, never resident, the tuple count always known
      if (min == BUILD_DEVICE_MIN_TUPLES) CHECK(build_route_taken(dev && cap, env, e) == taken(route_first(env, dev, cap, false), route_by_size(false, true, e, min)));
      cases++;
    }
  CHECK(cases == 10ul * 3 * 2 * 2 * 2 * 2 * 2 * 4);
  printf("route policy ok\n");
  return 0;
}
