// grb_bigholes.hpp — the constants of the "big holes" product of grb_mxv.cpp (a MIN_PLUS / MAX_PLUS product over an operand with holes, run by the full-operand
// kernels): the holes of the operand are filled with a BIG value, and a sum is an entry iff it lies on the near side of a threshold.  That is exact when
//   every real sum          a + u        lies strictly on the near side of the threshold,
//   every sum over a hole   a + fill     lies on or beyond it (k_big_to_absent keeps v < thresh for MIN, v > thresh for MAX),
//   no sum leaves the type's range (integers) or becomes NaN (floating point)
// for all |a| <= the matrix's bound and |u| <= the operand's — which is what the four limits below are for.  Host arithmetic on plain numbers only — no HIP types,
// no containers — so that a stand-alone program can check it under the sanitizers (tests/bigholes_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace grb {

// the four types that have the route, by their TypeCode numbers (grb_ops.hpp is not included here: its functions are marked for the device; grb_mxv.cpp asserts
// that the numbers agree)
constexpr int BH_INT32 = 5, BH_INT64 = 7, BH_FP32 = 9, BH_FP64 = 10;

// max(|min|, |max|) of the (min, max) pair value_range wrote for the type `code` (INT32 / INT64 / FP32 / FP64), as a double: an upper bound is all the callers need
inline double range_abs_of(int code, const void* mn, const void* mx) {
  double a = 0, b = 0;
  if (code == BH_INT32) { int32_t x, y; memcpy(&x, mn, 4); memcpy(&y, mx, 4); a = (double)x; b = (double)y; }
  else if (code == BH_INT64) { int64_t x, y; memcpy(&x, mn, 8); memcpy(&y, mx, 8); a = (double)x; b = (double)y; }
  else if (code == BH_FP32) { float x, y; memcpy(&x, mn, 4); memcpy(&y, mx, 4); a = x; b = y; }
  else { memcpy(&a, mn, 8); memcpy(&b, mx, 8); }
  const double x = fabs(a), y = fabs(b);
  return x < y ? y : x;
}

// the limits |A's values| and |u's values| must stay below — a quarter of BIG for the integers (BIG = 2^(bits-2): nothing wraps), sums that stay finite for
// floating point (BIG = infinity)
constexpr double BIG_HOLES_LIMIT_INT32 = 268435456.0;      // 2^28: real sums within +-2^29, hole sums beyond +-(2^30 - 2^28)
constexpr double BIG_HOLES_LIMIT_INT64 = 1.15e18;          // < 2^60
constexpr double BIG_HOLES_LIMIT_FP32 = 8e37;              // sums stay finite
constexpr double BIG_HOLES_LIMIT_FP64 = 4e307;

struct BigHolesConstants { bool admitted; uint8_t fill[16], thresh[16]; };      // fill / thresh: one value of the type in the first bytes

// `is_min`: the monoid is MIN (the fill and the threshold are positive), else MAX (negative); aabs / uabs: upper bounds of |A's values| and |u's values|
inline BigHolesConstants big_holes_constants(int code, bool is_min, double aabs, double uabs) {
  BigHolesConstants c{false, {0}, {0}};
  if (code == BH_INT32 && aabs < BIG_HOLES_LIMIT_INT32 && uabs < BIG_HOLES_LIMIT_INT32) {
    const int32_t f = is_min ? (1 << 30) : -(1 << 30), th = is_min ? (1 << 29) + (1 << 28) : -((1 << 29) + (1 << 28));
    memcpy(c.fill, &f, 4); memcpy(c.thresh, &th, 4); c.admitted = true;
  } else if (code == BH_INT64 && aabs < BIG_HOLES_LIMIT_INT64 && uabs < BIG_HOLES_LIMIT_INT64) {
    const int64_t f = is_min ? (1ll << 62) : -(1ll << 62), th = is_min ? (1ll << 61) + (1ll << 60) : -((1ll << 61) + (1ll << 60));
    memcpy(c.fill, &f, 8); memcpy(c.thresh, &th, 8); c.admitted = true;
  } else if (code == BH_FP32 && aabs < BIG_HOLES_LIMIT_FP32 && uabs < BIG_HOLES_LIMIT_FP32) {
    const float f = is_min ? INFINITY : -INFINITY; memcpy(c.fill, &f, 4); memcpy(c.thresh, &f, 4); c.admitted = true;
  } else if (code == BH_FP64 && aabs < BIG_HOLES_LIMIT_FP64 && uabs < BIG_HOLES_LIMIT_FP64) {
    const double f = is_min ? (double)INFINITY : -(double)INFINITY; memcpy(c.fill, &f, 8); memcpy(c.thresh, &f, 8); c.admitted = true;
  }
  return c;
}

}  // namespace grb
