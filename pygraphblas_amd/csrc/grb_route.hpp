// grb_route.hpp — host route or device route: the one policy of every container operation that has both (index-list extract and assign, kronecker, the two
// diagonal forms, sort / top-k; build-from-tuples follows the same rule through grb_build_keys.hpp).  Plain integers only — no HIP types, no containers — so that
// a stand-alone program can check it under the sanitizers (tests/route_policy_check.cpp).  The helpers that read containers (route_env, dev_capable, mat_capable,
// hbm_only, entries_of, entries_known, route_by_host_count) are in grb_internal.hpp.
//
// THE RULE, in two stages so that a caller asks for an entry count (and completes deferred work on a vector) only when the first stage left it to the size:
//   route_first    the test hook (0: host, 1: device wherever legal, -1 unset: go on), then legality — a HIP device, an HBM layout for every container of the
//                  call — then `forced`: an index list of the call lies in HBM, and it is not downloaded to pick a route.
//   route_by_size  an operand that lives in HBM only is not downloaded either: the device route, without asking for a count.  Otherwise a count that costs no
//                  device work (`count_known`) against the entry point's threshold below.
#pragma once
#include <cstdint>

namespace grb {

enum RouteStep { ROUTE_HOST, ROUTE_DEVICE, ROUTE_BY_SIZE };
constexpr RouteStep route_first(int env, bool have_device, bool all_capable, bool forced) {
  if (env == 0 || !have_device || !all_capable) return ROUTE_HOST;
  return (env == 1 || forced) ? ROUTE_DEVICE : ROUTE_BY_SIZE;
}
constexpr bool route_by_size(bool lives_in_hbm_only, bool count_known, uint64_t entries, uint64_t min_entries) {
  return lives_in_hbm_only || (count_known && entries >= min_entries);
}

// THE THRESHOLDS: entries from which an operation takes the device route by itself, each against its own host route, upload included (DESIGN.md "Routes").
// The tenth, BUILD_DEVICE_MIN_TUPLES, stays with the key arithmetic it is tested with (grb_build_keys.hpp).
constexpr uint64_t EXTRACT_DEVICE_MIN_ENTRIES = 10000;           // the three extract forms: the measured crossover against the host route, upload included
constexpr uint64_t ASSIGN_DEVICE_MIN_ENTRIES = 30000;            // GrB_Matrix_assign
constexpr uint64_t ASSIGN_ROW_DEVICE_MIN_ENTRIES = 3000000;      // GrB_Row_assign: the host replaces the row's run of tuples in place, cheap up to ~1e6 entries
constexpr uint64_t ASSIGN_COL_DEVICE_MIN_ENTRIES = 100000;       // GrB_Col_assign: the host's one merge pass
constexpr uint64_t ASSIGN_VEC_DEVICE_MIN_ENTRIES = 500;          // GrB_Vector_assign: the host route is map-based for every shape (the smallest size measured; the device route won all)
constexpr uint64_t KRON_DEVICE_MIN_ENTRIES = 1000;              // provisional: reasoned from the assign route's fixed cost, not yet measured
constexpr uint64_t DIAG_MATRIX_DEVICE_MIN_ENTRIES = 1000;       // GxB_Matrix_diag: measured, the host route is one std::map insertion per entry (0.11 ms against 0.07 ms at 1e3 entries)
constexpr uint64_t DIAG_VECTOR_DEVICE_MIN_ENTRIES = 10000;      // GxB_Vector_diag: measured, the host route is one pass over A's tuples (0.11 ms against 0.07 ms at 1e4 entries)
constexpr uint64_t SORT_DEVICE_MIN_ENTRIES = EXTRACT_DEVICE_MIN_ENTRIES;      // sort and top-k borrow extract's value: not measured on their own
constexpr uint64_t CONCAT_DEVICE_MIN_ENTRIES = EXTRACT_DEVICE_MIN_ENTRIES;    // GxB_Matrix_concat, on the sum of the tiles' entries: provisional, extract's value, not measured
constexpr uint64_t SPLIT_DEVICE_MIN_ENTRIES = EXTRACT_DEVICE_MIN_ENTRIES;     // GxB_Matrix_split, on A's entries: provisional, extract's value, not measured
// Not a host / device threshold but one between two device routes of GrB_mxm: products (nnz(A) k) from which an unmasked product with a full right operand takes
// the spmm_full route by itself instead of the two-pass hash product (GRB_MI355X_FULL: 0 never, 1 wherever legal).
constexpr uint64_t SPMM_FULL_MIN_PRODUCTS = 1ull << 18;          // the work count batch_wanted uses; measured: from 2.3e5 products (R-MAT-14, k = 1) up the route never lost to GRB_MI355X_FULL=0, the crossover below was not searched (DESIGN.md "Products with a full operand")
// Between two device routes of GrB_mxm as well: the work of the masked Gustavson route, m k n mask probes, from which a product of two full operands under a plain
// mask takes the sddmm route by itself (GRB_MI355X_SDDMM: 0 never, 1 wherever legal).
constexpr uint64_t SDDMM_MIN_WORK = 1ull << 16;                  // the smallest measured work count: from 6.6e4 (m = n = 256, k = 1: 0.016 ms against 0.177 ms) to 4.3e9 (m = n = 4096, k = 256: 0.141 against 1.496 ms) the route never lost to GRB_MI355X_SDDMM=0 in 100 points, the crossover below was not searched (DESIGN.md "Masked product of two full matrices")
// And a third: the multiply-adds m k n from which a product of two full operands without a plain mask takes the gemm_full route by itself, given at least two
// columns and GEMM_MIN_TILES tiles of the result (grb_gemm_geom.hpp) — calls that took spmm_full before, which read the left operand as an ordinary CSR
// (GRB_MI355X_GEMM: 0 never, 1 wherever legal; GRB_MI355X_FULL set: spmm_full's hook decides).
constexpr uint64_t GEMM_FULL_MIN_WORK = 1ull << 18;              // the count SPMM_FULL_MIN_PRODUCTS compares nnz(A) k against; measured: of the 128 sweep points from 2^18 up (m = 2^10 .. 2^20, k = 16 .. 256, n = 2 .. 256) the route lost to GRB_MI355X_GEMM=0 only at 4 and 8 tall tiles with k = 256 (0.060 against 0.052 ms), which the tile condition now leaves to spmm_full; the other 126 took 0.13 - 0.78 of its time; the crossover below 2^18 was not searched (DESIGN.md "Product of two full matrices")
// Between two device routes of GrB_mxv / GrB_vxm: the entries nrows ncols of a FULL matrix from which a product that is not transposed and has rows of at least
// GEMV_DEFAULT_MIN_INNER values takes the gemv_full route by itself instead of the SpMV kernels (GRB_MI355X_GEMV: 0 never, 1 wherever legal; grb_gemv_geom.hpp holds the rule).
constexpr uint64_t GEMV_FULL_MIN_WORK = 1ull << 24;              // measured, warm regime: the smallest work count from which layout N with rows of >= 2^16 values never lost to GRB_MI355X_GEMV=0 (256 x 2^16: 0.021 against 0.107 ms; 16 x 2^20, 64 x 2^20, 16 x 2^22 as well); 16 x 2^16 = 2^20 lost (0.017 against 0.012 ms), nothing between was measured (DESIGN.md "Full matrix times a vector")

}  // namespace grb
