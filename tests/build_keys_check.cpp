// build_keys_check.cpp — grb_build_keys.hpp on its own (plain integers, host code only): the bit counts of the dimensions, the key width, pack / unpack round trips
// at the 32 / 64-bit boundary, the bounds test on untruncated indices, the route predicate and the tree-foldable operators.  Built with the address and
// undefined-behaviour sanitizers by tests/test_build_host.py; prints "build keys ok".
#include "grb_build_keys.hpp"
#include <stdio.h>
#include <stdlib.h>

using namespace grb;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static void round_trip(uint64_t nrows, uint64_t ncols) {
  const int rbits = build_bits(nrows), cbits = build_bits(ncols);
  const uint64_t is[] = {0, 1, nrows / 2, nrows - 1}, js[] = {0, 1, ncols / 2, ncols - 1};
  for (uint64_t i : is) for (uint64_t j : js) {
    if (i >= nrows || j >= ncols) continue;
    const uint64_t key = build_pack(i, j, cbits);
    CHECK(build_key_row(key, cbits) == i && build_key_col(key, cbits) == j);
    CHECK(rbits + cbits == 64 || key < (1ull << (rbits + cbits)));
    if (build_key_is_u32(rbits, cbits)) CHECK(key == (uint64_t)(uint32_t)key);
    if (j + 1 < ncols) CHECK(build_pack(i, j + 1, cbits) > key);      // (i, j) in lexicographic order gives keys in order
    if (i + 1 < nrows) CHECK(build_pack(i + 1, 0, cbits) > build_pack(i, ncols - 1, cbits));
  }
}

int main() {
  // bits(dim - 1)
  CHECK(build_bits(0) == 0 && build_bits(1) == 0 && build_bits(2) == 1 && build_bits(3) == 2 && build_bits(4) == 2 && build_bits(5) == 3);
  CHECK(build_bits(1ull << 16) == 16 && build_bits((1ull << 16) + 1) == 17 && build_bits(BUILD_DIM_MAX) == 32 && build_bits(1ull << 32) == 32);
  // key width at the boundary: rbits + cbits = 32 is one word, 33 is two
  CHECK(build_key_is_u32(16, 16) && !build_key_is_u32(17, 16) && !build_key_is_u32(16, 17) && build_key_is_u32(32, 0) && build_key_is_u32(0, 0) && !build_key_is_u32(32, 32));
  CHECK(build_key_is_u32(build_bits(1ull << 16), build_bits(1ull << 16)) && !build_key_is_u32(build_bits((1ull << 16) + 1), build_bits(1ull << 16)));
  CHECK(build_sort_bits(0, 0) == 1 && build_sort_bits(16, 17) == 33 && build_sort_bits(32, 32) == 64);
  // round trips
  const uint64_t dims[] = {1, 2, 1ull << 16, (1ull << 16) + 1, BUILD_DIM_MAX};
  for (uint64_t r : dims) for (uint64_t c : dims) round_trip(r, c);
  CHECK(build_pack((1ull << 16) - 1, (1ull << 16) - 1, 16) == 0xFFFFFFFFull);                       // the extreme key of a 32-bit layout
  CHECK(build_pack(1ull << 16, (1ull << 16) - 1, 16) == 0x10000FFFFull);                           // ... and of a 33-bit one
  CHECK(build_pack(BUILD_DIM_MAX - 1, BUILD_DIM_MAX - 1, 32) == 0xFFFFFFEFFFFFFFEFull);
  CHECK(build_pack(7, 0, 0) == 7 && build_key_row(7, 0) == 7 && build_key_col(7, 0) == 0);          // a vector: the key is the index
  // bounds on the full 64-bit values
  CHECK(build_in_bounds(3, 0, 10, 1) && !build_in_bounds((1ull << 32) + 3, 0, 10, 1) && !build_in_bounds(0, (1ull << 32) + 3, 10, 10));
  CHECK(!build_in_bounds(10, 0, 10, 10) && build_in_bounds(9, 9, 10, 10) && !build_in_bounds(0, 0, 0, 5) && !build_in_bounds(~0ull, 0, BUILD_DIM_MAX, 1));
  // the route
  CHECK(build_route_legal(true, true, true, true, BUILD_DIM_MAX, BUILD_DIM_MAX, BUILD_TUPLES_MAX));
  CHECK(!build_route_legal(false, true, true, true, 10, 10, 10) && !build_route_legal(true, false, true, true, 10, 10, 10));
  CHECK(!build_route_legal(true, true, false, true, 10, 10, 10) && !build_route_legal(true, true, true, false, 10, 10, 10));
  CHECK(!build_route_legal(true, true, true, true, BUILD_DIM_MAX + 1, 10, 10) && !build_route_legal(true, true, true, true, 10, BUILD_DIM_MAX + 1, 10));
  CHECK(!build_route_legal(true, true, true, true, 10, 10, BUILD_TUPLES_MAX + 1) && !build_route_legal(true, true, true, true, 1ull << 60, 1ull << 60, 3));
  CHECK(build_route_taken(true, -1, BUILD_DEVICE_MIN_TUPLES) && !build_route_taken(true, -1, BUILD_DEVICE_MIN_TUPLES - 1));
  CHECK(build_route_taken(true, 1, 0) && !build_route_taken(true, 0, 1ull << 30) && !build_route_taken(false, 1, 1ull << 30) && !build_route_taken(false, -1, 1ull << 30));
  CHECK(BUILD_DEVICE_MIN_TUPLES > 9 && BUILD_RUN_SERIAL >= 2 && BUILD_RUN_SERIAL < 64 && BUILD_RUN_SERIAL_MAX > 129 && BUILD_RUN_SERIAL_MAX <= BUILD_TUPLES_MAX);
  // which operators fold as a tree (opcodes: grb_ops.hpp; grb_build.hip asserts the numbers)
  const int FIRST = 0, SECOND = 1, PAIR = 2, ANY = 3, MIN = 4, MAX = 5, PLUS = 6, MINUS = 7, TIMES = 9, DIV = 10, LOR = 19, LXOR = 21, BXNOR = 32;
  for (int op : {FIRST, SECOND, PAIR, ANY, MIN, MAX, LOR, LXOR}) CHECK(build_op_tree_foldable(op, true, false) && build_op_tree_foldable(op, false, false) && build_op_tree_foldable(op, false, true));
  CHECK(!build_op_tree_foldable(PLUS, true, false) && !build_op_tree_foldable(TIMES, true, false) && build_op_tree_foldable(PLUS, false, false) && build_op_tree_foldable(TIMES, false, true));
  CHECK(!build_op_tree_foldable(MINUS, false, false) && !build_op_tree_foldable(DIV, false, false) && !build_op_tree_foldable(MINUS, true, false) && build_op_tree_foldable(MINUS, false, true));
  CHECK(build_op_tree_foldable(BXNOR, false, false) && !build_op_tree_foldable(BXNOR, true, false));
  printf("build keys ok\n");
  return 0;
}
