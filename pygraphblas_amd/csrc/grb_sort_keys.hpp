// grb_sort_keys.hpp — the order of GxB_Matrix_sort / GxB_Vector_sort / GrBX_*_select_topk as unsigned keys: host and device code only (no HIP call, no
// container), so that a stand-alone program can check every pair of edge values (tests/sort_keys_check.cpp) and both routes share one definition.
//
// THE ORDER.  a precedes b when key(a) < key(b), or the keys are equal and a's index is the smaller one (the sorts are stable, or compare (key, position)
// pairs).  Under GrB_LT the key's unsigned order is the values' ascending order; under GrB_GT the key is the complement, with one exception: NaN.
//   unsigned integers, BOOL   the value itself (BOOL: x != 0), widened to 32 bits below that
//   signed integers           widened to 32 bits below that, the sign bit flipped: INT_MIN -> 0, -1 -> 0x7FFF.., 0 -> 0x8000..
//   floating point            -0.0 becomes +0.0 first (they tie); then the sign-magnitude flip: negative -> all bits complemented, else the sign bit set
//   NaN                       the largest key under LT and under GT alike: after every number, every NaN ties with every other
// Key width: 32 bits for BOOL, INT8 .. INT32, UINT8 .. UINT32 and FP32; 64 bits for INT64, UINT64 and FP64.  No real value has the all-ones key except NaN
// (LT: +inf is 0xFF80.., UINT_MAX is all ones but integers have no NaN to collide with — and equal keys only ever tie), so (all ones, 0xFFFFFFFF) is a pair
// above every real (key, position): positions stay below GRB_DIM_DEVICE_MAX.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // (the qualifiers grb_ops.hpp's GRB_HD expands to)
#endif
#include "grb_ops.hpp"
#include <string.h>

namespace grb {

constexpr uint64_t SORT_WAVE_MAX = 64;      // rows up to this long are sorted in the registers of one wave (one element per lane)
// Rows up to SORT_LDS_MAX are sorted by one workgroup in LDS, as (key, position) = (8 + 4) bytes per element for the wide keys.  Derived, not tuned: a compute
// unit has 160 KiB of LDS, two resident workgroups leave 80 KiB = 81 920 bytes each, 81 920 / 12 = 6 826 elements, and the largest power of two below that
// is 4 096 (48 KiB per workgroup: three would fit; 8 192 elements = 96 KiB would leave one).
constexpr uint64_t SORT_LDS_BYTES_PER_CU = 160 * 1024, SORT_LDS_RESIDENT = 2, SORT_LDS_ELEM_BYTES = 8 + 4;
constexpr uint64_t sort_pow2_floor(uint64_t x) { uint64_t p = 1; while (p * 2 <= x) p *= 2; return p; }
constexpr uint64_t SORT_LDS_MAX = sort_pow2_floor(SORT_LDS_BYTES_PER_CU / SORT_LDS_RESIDENT / SORT_LDS_ELEM_BYTES);
static_assert(SORT_LDS_MAX == 4096, "160 KiB / 2 workgroups / 12 bytes -> 4096 elements");

// The bin edges the default route uses: at most the capacities above, lowered where a bin measured slower than the segmented radix sort (DESIGN.md §8 "Sort and
// top-k", profiles/sort_probe.jsonl).  R-MAT-20 row sort, FP64 / INT32 ms: every row through the segmented sort 2.67 / 1.73; wave bin alone (edges 64, 64) 2.67 /
// 1.72; LDS edge 128 2.65 / 1.70 — the fastest of all, the chosen one; 256 2.76 / 1.73 and 512 2.74 / 1.72 (one wave per row); 1024 3.18 / 2.06 and the derived
// 4096 3.38 / 2.23 (four waves per row, a barrier per step): beyond 128 the bin loses, so its edge is 128.  GRB_MI355X_SORT_EDGES="64,4096" (grb_sort.hip) gives it
// other edges for one call.
constexpr uint64_t SORT_WAVE_EDGE = SORT_WAVE_MAX, SORT_LDS_EDGE = 128;
static_assert(SORT_WAVE_EDGE <= SORT_WAVE_MAX && SORT_WAVE_EDGE <= SORT_LDS_EDGE && SORT_LDS_EDGE <= SORT_LDS_MAX, "edges within the kernels' capacities");

GRB_HD bool sort_key_is_64(int code) { return code == T_INT64 || code == T_UINT64 || code == T_FP64; }

// the key type of a value type
template <class T> struct SortKeyOf { typedef typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type type; };

// key under GrB_LT
template <class T> GRB_HD typename SortKeyOf<T>::type sort_key_lt(T v) {
  typedef typename SortKeyOf<T>::type K;
  if constexpr (is_bool<T>::value) {
    return (K)(v.v != 0 ? 1u : 0u);
  } else if constexpr (std::is_same<T, float>::value) {
    if (v != v) return ~(K)0;
    uint32_t b; memcpy(&b, &v, 4);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  } else if constexpr (std::is_same<T, double>::value) {
    if (v != v) return ~(K)0;
    uint64_t b; memcpy(&b, &v, 8);
    if (b == 0x8000000000000000ull) b = 0;
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
  } else if constexpr (std::is_signed<T>::value) {
    if constexpr (sizeof(T) == 8) return (K)v ^ 0x8000000000000000ull;
    else return (K)(uint32_t)(int32_t)v ^ 0x80000000u;
  } else {
    return (K)v;
  }
}
// key under the operator of the call: `gt` = GrB_GT (the complement; NaN stays the largest)
template <class T> GRB_HD typename SortKeyOf<T>::type sort_key(T v, bool gt) {
  typedef typename SortKeyOf<T>::type K;
  const K k = sort_key_lt<T>(v);
  if (!gt) return k;
  if constexpr (std::is_floating_point<T>::value) { if (v != v) return ~(K)0; }
  return (K)~k;
}

// the same by type code over a value in memory, widened to 64 bits: the host route's comparisons (equal widths compare alike)
inline uint64_t sort_key_at(int code, const void* p, bool gt) {
  uint64_t k = 0;
  dispatch_type(code, [&]<class T>() { T v; memcpy(&v, p, sizeof(T)); k = (uint64_t)sort_key<T>(v, gt); });
  return k;
}

// how many entries of a line of `len` a top-k keeps
GRB_HD uint64_t topk_keep(uint64_t k, uint64_t len) { return k < len ? k : len; }

}  // namespace grb
