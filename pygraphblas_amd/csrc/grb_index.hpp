// grb_index.hpp — what the format / index kernels share on the device (grb_extract.hip, grb_assign.hip, grb_transpose.hip, grb_matops.hip): the word a
// value of 1 / 2 / 4 / 8 bytes moves as, the grid of a 256-thread streaming kernel, and an index argument (ExIdx, grb_extract.hpp) as the kernels take it.
#pragma once
#include "grb_extract.hpp"
#include "grb_device.hpp"

namespace grb {

// ---- values move untouched, as words of their size ---------------------------------------------------------------------
template <int TS> struct WordOf { typedef typename std::conditional<TS == 8, uint64_t, typename std::conditional<TS == 4, uint32_t, typename std::conditional<TS == 2, uint16_t, uint8_t>::type>::type>::type type; };
inline void check_value_size(size_t ts, const char* what) { if (ts != 1 && ts != 2 && ts != 4 && ts != 8) fail(GrB_DOMAIN_MISMATCH, std::string(what) + ": values of this size have no device route"); }
// Run `f.template operator()<TS>()` for a checked value size (dispatch_type's form, over sizes).
template <class F> inline void dispatch_value_size(size_t ts, F&& f) {
  switch (ts) {
    case 1: f.template operator()<1>(); break;
    case 2: f.template operator()<2>(); break;
    case 4: f.template operator()<4>(); break;
    default: f.template operator()<8>(); break;
  }
}

// blocks of a 256-thread grid-stride kernel over n items
inline unsigned grid_1d(uint64_t n, uint64_t cap = 4096) { uint64_t b = (n + 255) / 256; if (b < 1) b = 1; if (b > cap) b = cap; return (unsigned)b; }

__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

// ---- an index argument on the device, both ways ---------------------------------------------------------------------------
constexpr uint32_t NONE = 0xFFFFFFFFu;
struct DIdx { int kind; uint32_t lo, step; uint64_t n; const uint32_t* list; const uint32_t* inv; };      // inv: the inverse table of a list (assign_inverse), or nullptr
inline DIdx didx(const ExIdx& x, const DevBuf* inv = nullptr) { return DIdx{x.kind, x.lo, x.step ? x.step : 1u, x.n, x.list, inv ? inv->as<uint32_t>() : nullptr}; }
__device__ __forceinline__ uint32_t idx_at(const DIdx& x, uint64_t k) {
  switch (x.kind) {
    case EX_ALL: return (uint32_t)k;
    case EX_RANGE: return x.lo + (uint32_t)k * x.step;
    case EX_BACK: return x.lo - (uint32_t)k * x.step;
    default: return x.list[k];
  }
}
// the k < n with lo + k step == x (`desc`: lo - k step == x), or NONE
__device__ __forceinline__ uint32_t range_inv(bool desc, uint32_t lo, uint32_t step, uint64_t n, uint32_t x) {
  const bool side = desc ? x <= lo : x >= lo;
  const uint32_t d = desc ? lo - x : x - lo, q = d / step;
  return (side && q * step == d && q < n) ? q : NONE;
}
// the k with I[k] == i, or NONE
__device__ __forceinline__ uint32_t idx_inv(const DIdx& x, uint32_t i) {
  switch (x.kind) {
    case EX_ALL: return i;
    case EX_RANGE: case EX_BACK: return range_inv(x.kind == EX_BACK, x.lo, x.step, x.n, i);
    default: return x.inv[i];
  }
}

}  // namespace grb
