// grb_vecfacts.hpp — what the library remembers about the device image of a vector (val T[n] | present u8[n] in HBM) so that the next call can skip a pass.
// Plain host data: no HIP, no device buffers, so that a stand-alone program can check the transitions under the sanitizers (tests/vec_facts_check.cpp).
//
// THE RULE.  A fact is valid only for the image it was recorded for.  Whoever writes the image passes exactly one of the three transitions below — they are the
// only code that clears facts — and then states, in plain assignments, what it knows about the NEW image (`holes_zero = true` after a chain, `code_valid` after
// the masked assign that wrote the code bytes, the merged small list, the fill and the bound after a big-holes sweep, `lor_state` through any_true_written).
// No transition keeps a fact "because this caller knows better".  A kernel that reads the image and learns something (the count, the edges leaving the entries,
// the code bytes) records it without a transition.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace grb {

struct VecFacts {
  uint64_t dnvals = 0; bool dnvals_known = true;   // entry count of the device bitmap, recounted lazily
  // a lower bound of the edges that leave the vector's entries in one matrix (keyed by the serial of its row-pointer allocation, 0 = none), valid while entries
  // are only added (scalar assign under a mask without replace — the `v[q] = level` of a BFS loop): a masked product whose operand was already too heavy for a
  // push step needs no recount to stay a pull step.  A stale value can only cost speed, never correctness.
  // fe_lb_true: the bound counts the edges of the TRUE entries only (the product's summary), not of every present one
  uint64_t fe_lb = 0; uint64_t fe_lb_key = 0; bool fe_lb_true = false;
  bool holes_zero = false;     // the device values of absent positions are all-zero bits (written so by the element-wise chain kernel)
  bool holes_big = false; uint8_t holes_big_val[16] = {0};      // ... or all hold this value of the vector's type (the BIG fill of a MIN_PLUS / MAX_PLUS sweep, grb_mxv.cpp)
  // BOOL vectors: "is any stored value true", recorded by the product kernel that wrote the device buffers `lor_key`
  // (0 unknown, 1 in the device word of grb_any_true.cpp, 2 false, 3 true) — `while q.reduce_bool()` of a BFS loop
  uint8_t lor_state = 0; uint32_t lor_tag = 0; const void* lor_key = nullptr;
  // an upper bound of |value| over the stored entries, left behind by the "big holes" product that wrote them (grb_mxv.cpp: the next
  // sweep of a shortest-path loop needs no range kernel and no read-back); < 0 = unknown
  double abs_bound = -1;
  // the entries as a list, when there are at most 64 of them and the list is known for free (uploaded from a small host mirror; `v(q) = s` over the entries of
  // such a q): the first level of a BFS then pushes from the list — no frontier compaction (a flag pass, a scan and a scatter over all n positions), no counting
  // kernel, no read-back.  small_truthy: every listed value is non-zero.
  std::vector<uint32_t> small_idx; bool small_valid = false, small_truthy = false;
  // the vector's code buffer (GrB_Vector_opaque::dcode) holds one CODE byte per position of this image: bit 0 = present, bit 1 = present and its value is not
  // zero — what the masked pull of a BFS level gathers per neighbour as ONE byte instead of a presence byte and a value byte (grb_spmv_kernels.hpp:
  // k_spmv_rowlane_k<..., CODE>).  Written for free by the masked scalar assign that precedes the product (`v[q] = level`), else by one pass before the pull.
  bool code_valid = false;

  // ---- the transitions (no heap work: a BFS level is ~50 us of host time; small_idx keeps its capacity) ----
  // entries were only added to the image (values may have changed): the edge bound still bounds from below, nothing else is known
  void image_extended() {
    dnvals = 0; dnvals_known = false;
    holes_zero = false; holes_big = false; memset(holes_big_val, 0, 16);
    lor_state = 0; lor_tag = 0; lor_key = nullptr;
    abs_bound = -1;
    small_idx.clear(); small_valid = false; small_truthy = false;
    code_valid = false;
  }
  // a kernel wrote the image as a whole, or new buffers were installed: nothing is known but the count the writer gives (`nvals` is ignored when not `known`)
  void image_replaced(uint64_t nvals, bool known) {
    image_extended();
    fe_lb = 0; fe_lb_key = 0; fe_lb_true = false;
    dnvals = known ? nvals : 0; dnvals_known = known;
  }
  // there is no device image any more
  void image_dropped() { image_replaced(0, true); }

  // ---- a fact with two fields that exclude each other ----
  // the absent positions of the image now all hold `val` (16 bytes, a value of the vector's type first): the entries are what they were
  void holes_hold(const uint8_t* val) { holes_zero = false; holes_big = true; memcpy(holes_big_val, val, 16); }
};

}  // namespace grb
