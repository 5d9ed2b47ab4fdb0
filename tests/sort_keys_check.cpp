// sort_keys_check.cpp — grb_sort_keys.hpp on its own (host code only): for every value type, over all pairs of the type's edge values, key(a) < key(b) exactly
// when a precedes b in the stated order, and key(a) == key(b) exactly when they tie — under GrB_LT and under GrB_GT.  The order is restated here from the values
// themselves (comparisons, never keys).  Built with the address and undefined-behaviour sanitizers by tests/test_sort_host.py; prints "sort keys ok".
#include "grb_sort_keys.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// -1 a before b, 0 tie, 1 a after b: NaNs last under both operators and tied; otherwise by value (-0.0 == +0.0), ascending under LT, descending under GT
template <class T> static int stated_order(T a, T b, bool gt) {
  if constexpr (is_bool<T>::value) {
    const int x = a.v != 0, y = b.v != 0;
    return x == y ? 0 : ((x < y) != gt ? -1 : 1);
  } else {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && bn ? 0 : (an ? 1 : -1);
    if (a == b) return 0;
    return (a < b) != gt ? -1 : 1;
  }
}

template <class T> static void check_all_pairs(const std::vector<T>& edge, const char* name) {
  typedef typename SortKeyOf<T>::type K;
  static_assert(sizeof(K) == (sizeof(T) == 8 ? 8 : 4), "key width");
  for (const bool gt : {false, true}) {
    for (size_t i = 0; i < edge.size(); i++) for (size_t j = 0; j < edge.size(); j++) {
      const K ka = sort_key<T>(edge[i], gt), kb = sort_key<T>(edge[j], gt);
      const int want = stated_order<T>(edge[i], edge[j], gt);
      const int got = ka < kb ? -1 : (ka == kb ? 0 : 1);
      if (want != got) { printf("FAILED %s gt=%d pair (%zu, %zu): stated %d, keys %d\n", name, (int)gt, i, j, want, got); exit(1); }
      // the by-code form of the host route agrees with the typed one
      CHECK(sort_key_at(type_code_of<T>::value, &edge[i], gt) == (uint64_t)ka);
    }
  }
}

template <class T> static std::vector<T> int_edges() {
  std::vector<T> e = {std::numeric_limits<T>::min(), (T)0, (T)1, std::numeric_limits<T>::max(), (T)(std::numeric_limits<T>::max() / 2), (T)(std::numeric_limits<T>::max() / 2 + 1)};
  if (std::is_signed<T>::value) { e.push_back((T)-1); e.push_back((T)(std::numeric_limits<T>::min() + 1)); }
  else e.push_back((T)((T)1 << (sizeof(T) * 8 - 1)));                                // the high bit of an unsigned type
  return e;
}
template <class T, class U> static T from_bits(U b) { T v; memcpy(&v, &b, sizeof(T)); return v; }
template <class T> static std::vector<T> float_edges(T nan_a, T nan_b) {
  const T inf = std::numeric_limits<T>::infinity(), den = std::numeric_limits<T>::denorm_min();
  return {(T)-0.0, (T)0.0, den, (T)-den, inf, (T)-inf, nan_a, nan_b, (T)1, (T)-1, std::numeric_limits<T>::max(), std::numeric_limits<T>::lowest(), std::numeric_limits<T>::min(), (T)-std::numeric_limits<T>::min()};
}

int main() {
  check_all_pairs<bool8>({bool8(false), bool8(true), from_bits<bool8>((uint8_t)2), from_bits<bool8>((uint8_t)255)}, "BOOL");
  check_all_pairs<int8_t>(int_edges<int8_t>(), "INT8");
  check_all_pairs<uint8_t>(int_edges<uint8_t>(), "UINT8");
  check_all_pairs<int16_t>(int_edges<int16_t>(), "INT16");
  check_all_pairs<uint16_t>(int_edges<uint16_t>(), "UINT16");
  check_all_pairs<int32_t>(int_edges<int32_t>(), "INT32");
  check_all_pairs<uint32_t>(int_edges<uint32_t>(), "UINT32");
  check_all_pairs<int64_t>(int_edges<int64_t>(), "INT64");
  check_all_pairs<uint64_t>(int_edges<uint64_t>(), "UINT64");
  check_all_pairs<float>(float_edges<float>(from_bits<float>(0x7FC00000u), from_bits<float>(0xFFC12345u)), "FP32");
  check_all_pairs<double>(float_edges<double>(from_bits<double>(0x7FF8000000000000ull), from_bits<double>(0xFFF8000000012345ull)), "FP64");
  // NaN is the largest key under both operators, and nothing else reaches it among the floating-point values
  CHECK(sort_key<float>(from_bits<float>(0xFFC12345u), false) == 0xFFFFFFFFu && sort_key<float>(from_bits<float>(0x7FC00000u), true) == 0xFFFFFFFFu);
  CHECK(sort_key<double>(from_bits<double>(0xFFF8000000012345ull), true) == ~0ull && sort_key<float>(std::numeric_limits<float>::infinity(), false) < 0xFFFFFFFFu);
  CHECK(sort_key<float>(-std::numeric_limits<float>::infinity(), true) < 0xFFFFFFFFu && sort_key<double>(-std::numeric_limits<double>::infinity(), true) < ~0ull);
  // widths, thresholds, top-k counts
  CHECK(!sort_key_is_64(T_BOOL) && !sort_key_is_64(T_INT32) && !sort_key_is_64(T_UINT32) && !sort_key_is_64(T_FP32) && sort_key_is_64(T_INT64) && sort_key_is_64(T_UINT64) && sort_key_is_64(T_FP64));
  CHECK(SORT_WAVE_MAX == 64 && SORT_LDS_MAX > SORT_WAVE_MAX && (SORT_LDS_MAX & (SORT_LDS_MAX - 1)) == 0);
  CHECK(SORT_LDS_MAX * SORT_LDS_ELEM_BYTES * SORT_LDS_RESIDENT <= SORT_LDS_BYTES_PER_CU && 2 * SORT_LDS_MAX * SORT_LDS_ELEM_BYTES * SORT_LDS_RESIDENT > SORT_LDS_BYTES_PER_CU);
  CHECK(topk_keep(0, 5) == 0 && topk_keep(3, 5) == 3 && topk_keep(5, 5) == 5 && topk_keep(~0ull, 5) == 5 && topk_keep(4, 0) == 0);
  printf("sort keys ok\n");
  return 0;
}
