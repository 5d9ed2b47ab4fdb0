// vec_facts_check.cpp — the three transitions of grb_vecfacts.hpp (what is remembered about a vector's device image) on a record with every fact set: a stand-alone
// host program, meant to be built plainly and with the address and undefined-behaviour sanitizers and run on the CPU (tests/test_vec_facts_host.py does).
//   image_dropped             every field as in a default-constructed record;
//   image_replaced(k, known)  the same, but for the count: (k, known), or (0, unknown) — k is ignored when the count is not known;
//   image_extended            the three fields of the edge bound as they were, the count unknown, every other field at its default;
//   holes_hold                the two hole facts, nothing else.
// Every field is set and compared by name, and the size of the record is pinned: a fact added to the header without a line here does not compile.
// No device code runs.
#include "grb_vecfacts.hpp"
#include <stdio.h>

using grb::VecFacts;

// x86-64 / libstdc++ and libc++, from the build: dnvals 8 | dnvals_known 1 (+7) | fe_lb 8 | fe_lb_key 8 | fe_lb_true, holes_zero, holes_big 3 | holes_big_val 16 |
// lor_state 1 | lor_tag 4 | lor_key 8 | abs_bound 8 | small_idx 24 | small_valid, small_truthy, code_valid 3 (+5) = 104
static_assert(sizeof(VecFacts) == 104, "a fact was added to or taken from VecFacts: extend set_all(), differing() with NFIELDS and the field list above, then this number");

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int dummy_key;

static void set_all(VecFacts& f) {
  f.dnvals = 41; f.dnvals_known = false;
  f.fe_lb = 1000003; f.fe_lb_key = 77; f.fe_lb_true = true;
  f.holes_zero = true;
  f.holes_big = true; for (int b = 0; b < 16; b++) f.holes_big_val[b] = (uint8_t)(0xA0 + b);
  f.lor_state = 3; f.lor_tag = 0xBEEF; f.lor_key = &dummy_key;
  f.abs_bound = 12.5;
  f.small_idx = {1, 5, 9}; f.small_valid = true; f.small_truthy = true;
  f.code_valid = true;
}

// field by field: the number of fields that differ, each reported when `what` is given; the count and the edge bound are compared by the caller's choice
constexpr int NFIELDS = 16;
static int differing(const VecFacts& a, const VecFacts& b, bool count, bool edges, const char* what) {
  int d = 0;
#define FIELD(eq, name) do { if (!(eq)) { d++; if (what) { failures++; printf("FAILED %s: %s\n", what, name); } } } while (0)
  if (count) { FIELD(a.dnvals == b.dnvals, "dnvals"); FIELD(a.dnvals_known == b.dnvals_known, "dnvals_known"); }
  if (edges) { FIELD(a.fe_lb == b.fe_lb, "fe_lb"); FIELD(a.fe_lb_key == b.fe_lb_key, "fe_lb_key"); FIELD(a.fe_lb_true == b.fe_lb_true, "fe_lb_true"); }
  FIELD(a.holes_zero == b.holes_zero, "holes_zero");
  FIELD(a.holes_big == b.holes_big, "holes_big");
  FIELD(memcmp(a.holes_big_val, b.holes_big_val, 16) == 0, "holes_big_val");
  FIELD(a.lor_state == b.lor_state, "lor_state");
  FIELD(a.lor_tag == b.lor_tag, "lor_tag");
  FIELD(a.lor_key == b.lor_key, "lor_key");
  FIELD(a.abs_bound == b.abs_bound, "abs_bound");
  FIELD(a.small_idx == b.small_idx, "small_idx");
  FIELD(a.small_valid == b.small_valid, "small_valid");
  FIELD(a.small_truthy == b.small_truthy, "small_truthy");
  FIELD(a.code_valid == b.code_valid, "code_valid");
#undef FIELD
  return d;
}
static void same(const VecFacts& a, const VecFacts& b, bool count, bool edges, const char* what) { differing(a, b, count, edges, what); }

int main() {
  const VecFacts fresh;
  CHECK(fresh.dnvals == 0 && fresh.dnvals_known, "defaults: the count is known and 0");
  CHECK(fresh.abs_bound == -1, "defaults: abs_bound %g", fresh.abs_bound);
  { VecFacts set; set_all(set); const int d = differing(set, fresh, true, true, nullptr); CHECK(d == NFIELDS, "set_all leaves %d field(s) at their defaults", NFIELDS - d); }

  { VecFacts f; set_all(f); f.image_dropped(); same(f, fresh, true, true, "image_dropped"); }

  for (int known = 0; known < 2; known++) {
    VecFacts f; set_all(f); f.image_replaced(12345, known != 0);
    same(f, fresh, false, true, known ? "image_replaced(k, known)" : "image_replaced(k, unknown)");
    CHECK(f.dnvals_known == (known != 0) && f.dnvals == (known ? 12345u : 0u), "image_replaced: count (%llu, %d)", (unsigned long long)f.dnvals, (int)f.dnvals_known);
  }

  {
    VecFacts f, was; set_all(f); set_all(was); f.dnvals_known = true; f.image_extended();
    same(f, fresh, false, false, "image_extended");
    CHECK(f.fe_lb == was.fe_lb && f.fe_lb_key == was.fe_lb_key && f.fe_lb_true == was.fe_lb_true, "image_extended: the edge bound is unchanged");
    CHECK(!f.dnvals_known && f.dnvals == 0, "image_extended: the count is unknown");
  }

  {
    // the transitions do no heap work: the list's storage is kept for the next list
    VecFacts f; set_all(f); const size_t cap = f.small_idx.capacity(); const uint32_t* at = f.small_idx.data();
    f.image_replaced(0, false);
    CHECK(f.small_idx.empty() && f.small_idx.capacity() == cap && f.small_idx.data() == at, "image_replaced: small_idx keeps its storage");
  }

  {
    VecFacts f, want; set_all(f); set_all(want); f.holes_big = false;
    uint8_t v[16]; for (int b = 0; b < 16; b++) v[b] = (uint8_t)(b + 1);
    f.holes_hold(v);
    want.holes_zero = false; want.holes_big = true; memcpy(want.holes_big_val, v, 16);
    same(f, want, true, true, "holes_hold");
  }

  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("vec facts ok (sizeof %zu)\n", sizeof(VecFacts));
  return 0;
}
