// grb_build.hpp — host interface of build-from-tuples in HBM (grb_build.hip); the routes are mat_build / vec_build in grb_build_ops.cpp, the key arithmetic and the
// thresholds are in grb_build_keys.hpp.
#pragma once
#include "grb_internal.hpp"
#include "grb_build_keys.hpp"

namespace grb {

enum BuildStatus { BUILD_OK = 0, BUILD_OUT_OF_BOUNDS, BUILD_DUPLICATE, BUILD_RUN_TOO_LONG };
struct BuildResult {
  BuildStatus status = BUILD_OK;
  uint64_t nvals = 0;            // distinct positions
  bool key64 = false;            // the sort key needed 64 bits
  bool sorted = false;           // the keys came strictly increasing: no sort, no duplicate pass
  bool search = false;           // the row pointer was bisected per row (BUILD_ROWPTR_SEARCH_FACTOR), not written from the run heads
  const char* fold = "none";     // none: no duplicates; serial: every run folded left to right by one lane (or one wave's lane order); wave: some run took the shuffle tree
};

// The tuples (I[k], J[k], X[k]), k < n, as `rows` / `col` / `val` of the nvals distinct positions in (row, column) order, duplicates folded with `dup_op` LEFT TO RIGHT
// IN INPUT ORDER (z = dup(dup(x0, x1), x2) ...: what build_tuples does on the host, bit for bit).  All pointers are device pointers; I / J hold 64-bit indices and are
// tested against nrows / ncols as such; J == nullptr: a vector (ncols = 1, key = i).  X and val hold values of type `tcode`; dup_op < 0: no operator (a duplicate
// is BUILD_DUPLICATE).  nrows, ncols <= BUILD_DIM_MAX, n <= BUILD_TUPLES_MAX (checked by the caller: the kernels' bounds depend on it).
// Outcomes in the host route's order: BUILD_OUT_OF_BOUNDS, then BUILD_DUPLICATE, then BUILD_RUN_TOO_LONG (a run beyond BUILD_RUN_SERIAL_MAX of an operator that is
// not exactly associative: the caller takes the host route); on each of them `rows` / `col` / `val` are left unallocated.  Temporaries come from the pool.
BuildResult build_from_tuples(int tcode, const uint64_t* I, const uint64_t* J, const void* X, uint64_t n, uint64_t nrows, uint64_t ncols, int dup_op,
                              DevBuf& rows, DevBuf* col, DevBuf& val);
// rowptr[0 .. nrows] of the sorted row list rows[0 .. nvals): k_rowptr_from_sorted (grb_transpose.hip), or a bisection per row when the rows outnumber the
// entries BUILD_ROWPTR_SEARCH_FACTOR times; true when it bisected
bool build_rowptr(const uint32_t* rows, uint64_t nvals, uint32_t nrows, uint32_t* rowptr);

// grb_transpose.hip: row pointers from SORTED row (or column) keys — position i starts the run of k[i], and every key between its predecessor and k[i] is an empty row that starts there too
void rowptr_from_sorted(const uint32_t* keys, uint64_t n, uint32_t nkeys, uint32_t* rowptr);

}  // namespace grb
