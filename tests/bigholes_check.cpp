// bigholes_check.cpp — stand-alone host check of the "big holes" constants of grb_bigholes.hpp (the fill, the threshold and the four limits that keep a MIN_PLUS /
// MAX_PLUS product over an operand with holes exact), meant to be built plainly and with the address and undefined-behaviour sanitizers (host code only) and run on the
// CPU (tests/test_bigholes_host.py does).  For INT32, INT64, FP32 and FP64 under MIN and MAX, at the largest |A| and |u| the limits admit:
//   every real sum a + u lies strictly on the near side of the threshold, in both signs;
//   every sum with the fill in place of u lies on or beyond it — by the comparison k_big_to_absent makes: kept iff v < thresh (MIN) / v > thresh (MAX);
//   no such sum leaves the type's range (integers, computed in a wider type so the check itself cannot wrap) or becomes NaN (floating point);
//   a bound at or just past the limit is not admitted.
// No device code runs.
#include "grb_bigholes.hpp"
#include <stdio.h>
#include <float.h>
#include <limits.h>
#include <initializer_list>

typedef __int128 i128;
using namespace grb;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// kept iff v < thresh for MIN, v > thresh for MAX
template <class V> static bool kept(bool is_min, V v, V thresh) { return is_min ? v < thresh : v > thresh; }

// the largest integer magnitude a limit admits: the driver passes (double)|value|, which rounds an INT64 — so walk down from the limit until the double is admitted
template <class I> static I largest_admitted(int code) {
  const double limit = code == BH_INT32 ? BIG_HOLES_LIMIT_INT32 : BIG_HOLES_LIMIT_INT64;
  I x = (I)limit;
  for (int step = 0; step < 4096 && !big_holes_constants(code, true, (double)x, (double)x).admitted; step++) x--;
  return x;
}

template <class I> static void check_integer(int code, const char* name, i128 type_min, i128 type_max) {
  const I big = largest_admitted<I>(code);
  CHECK(big_holes_constants(code, true, (double)big, (double)big).admitted && !big_holes_constants(code, true, (double)(big + 1), 0).admitted, "%s: the largest admitted bound", name);
  CHECK((double)big >= (code == BH_INT32 ? 268435455.0 : 1.1499e18), "%s: the largest admitted bound is far below the limit", name);
  for (int m = 0; m < 2; m++) {
    const bool is_min = m == 0;
    const BigHolesConstants c = big_holes_constants(code, is_min, (double)big, (double)big);
    CHECK(c.admitted, "%s %s", name, is_min ? "MIN" : "MAX");
    I fill, thresh; memcpy(&fill, c.fill, sizeof(I)); memcpy(&thresh, c.thresh, sizeof(I));
    // sums are monotone in a and u: the extremes and their neighbours decide; both signs of both
    const I ends[] = {(I)-big, (I)(-big + 1), (I)-1, (I)0, (I)1, (I)(big - 1), big};
    for (I a : ends) {
      for (I u : ends) {
        const i128 real = (i128)a + (i128)u;
        CHECK(real >= type_min && real <= type_max, "%s: a real sum leaves the range", name);
        CHECK(kept<i128>(is_min, real, (i128)thresh), "%s %s: a real sum is not on the near side of the threshold (a=%lld u=%lld)", name, is_min ? "MIN" : "MAX", (long long)a, (long long)u);
      }
      const i128 hole = (i128)a + (i128)fill;
      CHECK(hole >= type_min && hole <= type_max, "%s %s: a sum over a hole leaves the range (a=%lld)", name, is_min ? "MIN" : "MAX", (long long)a);
      CHECK(!kept<i128>(is_min, hole, (i128)thresh), "%s %s: a sum over a hole is kept (a=%lld)", name, is_min ? "MIN" : "MAX", (long long)a);
    }
    // at the limit and just past it: not admitted, for either bound
    const double limit = code == BH_INT32 ? BIG_HOLES_LIMIT_INT32 : BIG_HOLES_LIMIT_INT64;
    for (double past : {limit, nextafter(limit, INFINITY), limit * 2}) {
      CHECK(!big_holes_constants(code, is_min, past, 0).admitted && !big_holes_constants(code, is_min, 0, past).admitted, "%s: a bound of %g is admitted", name, past);
    }
  }
}

template <class F> static void check_floating(int code, const char* name, double limit) {
  // the largest value of the type below the limit (the driver passes the type's own values, widened)
  F big = (F)limit;
  while ((double)big >= limit) big = (F)(sizeof(F) == 4 ? nextafterf((float)big, 0.0f) : nextafter((double)big, 0.0));
  CHECK(big_holes_constants(code, true, (double)big, (double)big).admitted, "%s: the largest value below the limit", name);
  CHECK((double)big > limit * 0.999999, "%s: the largest admitted bound is far below the limit", name);
  for (int m = 0; m < 2; m++) {
    const bool is_min = m == 0;
    const BigHolesConstants c = big_holes_constants(code, is_min, (double)big, (double)big);
    CHECK(c.admitted, "%s %s", name, is_min ? "MIN" : "MAX");
    F fill, thresh; memcpy(&fill, c.fill, sizeof(F)); memcpy(&thresh, c.thresh, sizeof(F));
    const F tiny = sizeof(F) == 4 ? (F)FLT_TRUE_MIN : (F)DBL_TRUE_MIN;
    const F ends[] = {(F)-big, (F)-1, (F)-tiny, (F)-0.0, (F)0, tiny, (F)1, big};
    for (F a : ends) {
      for (F u : ends) {
        const F real = a + u;      // (in the type itself: what the kernels compute)
        CHECK(!isnan(real) && !isinf(real), "%s: a real sum is not finite", name);
        CHECK(kept<F>(is_min, real, thresh), "%s %s: a real sum is not on the near side of the threshold (a=%g u=%g)", name, is_min ? "MIN" : "MAX", (double)a, (double)u);
      }
      const F hole = a + fill;
      CHECK(!isnan(hole), "%s %s: a sum over a hole is NaN (a=%g)", name, is_min ? "MIN" : "MAX", (double)a);
      CHECK(!kept<F>(is_min, hole, thresh), "%s %s: a sum over a hole is kept (a=%g)", name, is_min ? "MIN" : "MAX", (double)a);
    }
    for (double past : {limit, nextafter(limit, INFINITY), limit * 2, (double)INFINITY}) {
      CHECK(!big_holes_constants(code, is_min, past, 0).admitted && !big_holes_constants(code, is_min, 0, past).admitted, "%s: a bound of %g is admitted", name, past);
    }
    CHECK(!big_holes_constants(code, is_min, (double)NAN, 0).admitted && !big_holes_constants(code, is_min, 0, (double)NAN).admitted, "%s: a NaN bound is admitted", name);
  }
}

int main() {
  check_integer<int32_t>(BH_INT32, "INT32", INT32_MIN, INT32_MAX);
  check_integer<int64_t>(BH_INT64, "INT64", INT64_MIN, INT64_MAX);
  check_floating<float>(BH_FP32, "FP32", BIG_HOLES_LIMIT_FP32);
  check_floating<double>(BH_FP64, "FP64", BIG_HOLES_LIMIT_FP64);
  // the other types have no such route
  for (int code = -1; code < 16; code++)
    if (code != BH_INT32 && code != BH_INT64 && code != BH_FP32 && code != BH_FP64)
      CHECK(!big_holes_constants(code, true, 0, 0).admitted && !big_holes_constants(code, false, 1, 1).admitted, "type code %d is admitted", code);
  // the range decode: max(|min|, |max|) of the pair value_range writes
  { const int32_t mn = INT32_MIN, mx = 5; CHECK(range_abs_of(BH_INT32, &mn, &mx) == 2147483648.0, "INT32 range"); }
  { const int32_t mn = -3, mx = 7; CHECK(range_abs_of(BH_INT32, &mn, &mx) == 7.0, "INT32 range"); }
  { const int64_t mn = INT64_MIN, mx = INT64_MAX; CHECK(range_abs_of(BH_INT64, &mn, &mx) == 9223372036854775808.0, "INT64 range"); }
  { const int64_t mn = -9, mx = -2; CHECK(range_abs_of(BH_INT64, &mn, &mx) == 9.0, "INT64 range"); }
  { const float mn = -2.5f, mx = 1.0f; CHECK(range_abs_of(BH_FP32, &mn, &mx) == 2.5, "FP32 range"); }
  { const double mn = 0.25, mx = 1e300; CHECK(range_abs_of(BH_FP64, &mn, &mx) == 1e300, "FP64 range"); }
  printf(failures ? "big holes: %d checks failed\n" : "big holes ok\n", failures);
  return failures ? 1 : 0;
}
