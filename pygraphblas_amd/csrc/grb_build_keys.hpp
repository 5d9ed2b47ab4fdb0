// grb_build_keys.hpp — the integer side of build-from-tuples on the device (grb_build.hip, mat_build / vec_build in grb_build_ops.cpp): how a tuple's
// (i, j) packs into one sort key, which key width a pair of dimensions needs, the bounds test on the 64-bit indices as the C ABI hands them over, the three
// thresholds, and the route predicate.  Plain integers only — no HIP types, no containers — so that a stand-alone program can check it under the sanitizers
// (tests/build_keys_check.cpp).  Every function is constexpr: host code and the kernels call the same text.
//
// THE THRESHOLDS
//   BUILD_DEVICE_MIN_TUPLES  tuples from which a build takes the device route by itself: the measured crossover against the host route (a stable sort of an index
//                            permutation on one thread), upload of the tuples included — tools/build_probe.py --what sweep, profiles/build_probe.jsonl, DESIGN.md §8.
//   BUILD_RUN_SERIAL         a run of duplicates up to this long is folded by ONE LANE (a lane per run).  A lane's fold is a chain of dependent gathers
//                            X[perm[p]], and the other 63 lanes of its wave wait for the longest run among them; a wave per run gathers 64 values at once and
//                            folds them in six shuffle steps, but occupies a whole wave for one output.  With ~5 % duplicates nearly every run has 1 or 2
//                            entries, so the lane form must cover the common case and the wave form pays from the length at which one lane's chain
//                            (L gathers of ~1 us issue-to-use under load, partly overlapped) outlasts a wave's gather + tree (~one gather + 6 x 2 cross-lane
//                            moves): between one and two dozen.  16 = a quarter of a wave, and a lane's 16 gathers of 8 bytes touch at most 16 cache lines.
//   BUILD_RUN_SERIAL_MAX     the longest run that an operator WITHOUT exact associativity (FP PLUS / TIMES, MINUS, DIV, ...) may have on the device: such a run
//                            is folded left to right by one wave, 64 gathered values at a time, ~10 cycles per value (a broadcast and the operator) — 65 536
//                            values are ~0.3 ms, about what the sort of a 10^6-tuple build takes.  Beyond it one wave's tail would dominate the call while
//                            255 compute units idle, and the host folds at the same rate: the whole call keeps the host route (decided before C is touched).
//   The figures behind BUILD_RUN_SERIAL and BUILD_RUN_SERIAL_MAX (gather latency, cycles per value, the 0.3 ms) are ESTIMATES from the kernel's shape, not
//   measurements: neither constant has been swept.  The serial branch pays a variable-index shuffle per value, so ~10 cycles is the optimistic end.
//   BUILD_ROWPTR_SEARCH_FACTOR (below) is not measured either: it only has to keep the bisection away from ordinary shapes (a few entries per row).
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint64_t BUILD_DIM_MAX = 0xFFFFFFF0ull;            // == GRB_DIM_DEVICE_MAX: rows and columns are 32-bit words in HBM
constexpr uint64_t BUILD_TUPLES_MAX = 0xFFFFFFF0ull;         // the sort payload is the 32-bit input position
constexpr uint64_t BUILD_DEVICE_MIN_TUPLES = 10000;          // measured (DESIGN.md §8 "Build from tuples"): the device route wins from 10^4 tuples on, at every larger swept size
constexpr uint32_t BUILD_RUN_SERIAL = 16;
constexpr uint32_t BUILD_RUN_SERIAL_MAX = 65536;
// row pointers: k_rowptr_from_sorted lets the thread in front of a gap of empty rows write the whole gap; when the rows outnumber the entries by more than this factor
// (gaps that long on average) every row bisects the sorted row list instead
constexpr uint64_t BUILD_ROWPTR_SEARCH_FACTOR = 64;

// bits(dim - 1): how many bits an index below `dim` needs (0 for dim <= 1: the only index is 0)
constexpr int build_bits(uint64_t dim) { int b = 0; if (dim > 1) { uint64_t m = dim - 1; while (m) { b++; m >>= 1; } } return b; }
// the key holds rbits + cbits bits: a 32-bit word when they fit one
constexpr bool build_key_is_u32(int rbits, int cbits) { return rbits + cbits <= 32; }
// both indices below their dimension, tested on the full 64-bit values (never after truncation: 2^32 + 3 is not row 3)
constexpr bool build_in_bounds(uint64_t i, uint64_t j, uint64_t nrows, uint64_t ncols) { return i < nrows && j < ncols; }
// key = (i << cbits) | j for in-bounds indices (cbits <= 32, i < 2^32: no bit is lost in 64 bits; cbits == 0: the key is i)
constexpr uint64_t build_pack(uint64_t i, uint64_t j, int cbits) { return (i << cbits) | j; }
constexpr uint32_t build_key_row(uint64_t key, int cbits) { return (uint32_t)(key >> cbits); }
constexpr uint32_t build_key_col(uint64_t key, int cbits) { return (uint32_t)(key & ((1ull << cbits) - 1ull)); }
// the sort's end bit (rocPRIM wants a non-empty bit range: a 1 x 1 container sorts on bit 0, which every key has clear)
constexpr int build_sort_bits(int rbits, int cbits) { return rbits + cbits > 0 ? rbits + cbits : 1; }

// Is the device route LEGAL for a call?  `real_type`: one of the 11 real types; `same_type`: the tuples' type is the container's; `dup_ok`: no dup, or a built-in,
// non-positional operator on the container's type that the device evaluates to the host's bits.
constexpr bool build_route_legal(bool have_device, bool real_type, bool same_type, bool dup_ok, uint64_t nrows, uint64_t ncols, uint64_t n) {
  return have_device && real_type && same_type && dup_ok && nrows <= BUILD_DIM_MAX && ncols <= BUILD_DIM_MAX && n <= BUILD_TUPLES_MAX;
}
// ... and is it TAKEN?  env: the GRB_MI355X_BUILD hook (0 host, 1 device wherever legal, -1 unset: by size)
constexpr bool build_route_taken(bool legal, int env, uint64_t n) { return legal && env != 0 && (env == 1 || n >= BUILD_DEVICE_MIN_TUPLES); }

// can a run of `op` values be folded as a tree?  Exactly associative on the type: the selectors, MIN / MAX, the logical operators, and on integer and BOOL types
// also the wrapping PLUS / TIMES and the bitwise operators.  (MINUS, DIV, the comparisons ... are not associative on any type: they fold left to right.)
// Opcodes are grb_ops.hpp's BinOpCode, passed as integers: FIRST 0, SECOND 1, PAIR 2, ANY 3, MIN 4, MAX 5, PLUS 6, TIMES 9, LOR 19, LAND 20, LXOR 21, LXNOR 28, BOR..BXNOR 29..32.
constexpr bool build_op_tree_foldable(int op, bool fp_type, bool bool_type) {
  if (op <= 5 || (op >= 19 && op <= 21)) return true;
  if (fp_type) return false;
  if (op == 6 || op == 9) return true;
  if (bool_type) return op == 13 || op == 22 || op == 28 || op == 14 || op == 23 || op == 7 || op == 8;      // ISEQ / EQ / LXNOR (xnor) and ISNE / NE / MINUS / RMINUS (xor) on BOOL
  return op >= 29 && op <= 32;
}

}  // namespace grb
