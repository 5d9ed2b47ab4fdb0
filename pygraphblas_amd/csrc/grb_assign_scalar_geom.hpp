// grb_assign_scalar_geom.hpp — the region arithmetic of the matrix scalar assign C<M>(I, J) = s (grb_assign_scalar.hip, do_assign_scalar in grb_matrix_ops.cpp):
// how many indices a range triple names, where its sorted form starts, the size of the block I x J against the device layout's limit, and which column an
// entry of the block holds.  Host arithmetic on plain integers only — no HIP types, no containers — so that a stand-alone program can check it under the
// sanitizers (tests/assign_scalar_geometry_check.cpp).  Unsigned throughout; the size test never forms a product that could wrap, and the range
// helpers stay within 64 bits for every triple that extract_parse accepted (indices below the dimension).
#pragma once
#include <stdint.h>

namespace grb {

// the largest block the device layout holds (entry positions are 32-bit words): the limit do_assign_scalar has always had
constexpr uint64_t SCALAR_REGION_MAX = 0xFFFFFFF0ull;

// nsel ncs <= SCALAR_REGION_MAX, without forming a product that could wrap
inline bool scalar_region_fits(uint64_t nsel, uint64_t ncs) { return nsel == 0 || ncs == 0 || ncs <= SCALAR_REGION_MAX / nsel; }
// ... and the product itself where it fits (0 where a side is empty)
inline uint64_t scalar_region_entries(uint64_t nsel, uint64_t ncs) { return scalar_region_fits(nsel, ncs) ? nsel * ncs : 0; }

// indices named by the triple begin : end (inclusive) : step, forwards (begin <= end) or backwards (begin >= end); 0 for step 0 or an empty direction
inline uint64_t scalar_range_count(bool backwards, uint64_t begin, uint64_t end, uint64_t step) {
  if (step == 0) return 0;
  if (backwards) return begin >= end ? (begin - end) / step + 1 : 0;
  return begin <= end ? (end - begin) / step + 1 : 0;
}
// the smallest index a range of n >= 1 indices names: a backwards range is read from its far end (lo - (n - 1) step, which is >= 0 for a valid range)
inline uint64_t scalar_range_first(bool backwards, uint64_t lo, uint64_t step, uint64_t n) { return (backwards && n) ? lo - (n - 1) * step : lo; }
// the k-th smallest index of that range (k < n)
inline uint64_t scalar_range_sorted_at(bool backwards, uint64_t lo, uint64_t step, uint64_t n, uint64_t k) { return scalar_range_first(backwards, lo, step, n) + k * step; }

// entry p of the block (row-major, ncs > 0 columns per selected row) holds the (p mod ncs)-th smallest selected column and lies in the (p / ncs)-th selected row;
// the row pointer of a row that has `rank` selected rows before it is rank ncs
inline uint64_t scalar_block_slot(uint64_t p, uint64_t ncs) { return p % ncs; }
inline uint64_t scalar_block_rowptr(uint64_t rank, uint64_t ncs) { return rank * ncs; }
// the slot after `slot` (the fill kernel divides once per group of entries and steps from there)
inline uint64_t scalar_block_next_slot(uint64_t slot, uint64_t ncs) { return slot + 1 == ncs ? 0 : slot + 1; }

}  // namespace grb
