// csr_derived_check.cpp — the transitions of grb_devcsr.hpp (what is derived from a matrix's device CSR, and the only code that clears it) on a CSR with an image,
// every derived field set and every buffer allocated: a stand-alone host program, meant to be built plainly and with the address and undefined-behaviour
// sanitizers and run on the CPU (tests/test_csr_derived_host.py does).  The allocator the header only declares is malloc / free here, with a count of the live
// allocations.
//   structure_changed   every derived field as in a default-constructed record, the live allocations are the image's three;
//   values_changed      xcd, range_state, range_abs, heads_valid, heads_vals at their defaults; every other field, the buffers included, as it was;
//   drop_wavepipe       the eight wp_* fields at their defaults, nothing else;
//   clear               no live allocation, valid == false, the image fields and the record at their defaults;
//   move assignment     of a fresh DevCSR over a fully cached one leaves no allocation of the old one alive.
// Every field is set and compared by name, and the size of the record is pinned: a field added to the header without a line here does not compile.
// No device code runs.
#include "grb_devcsr.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <array>
#include <utility>

static long live = 0;
namespace grb {
void* dev_alloc(size_t bytes) { void* p = malloc(bytes); if (!p) abort(); live++; return p; }
void dev_free(void* p) { live--; free(p); }
uint64_t dev_alloc_serial() { static uint64_t s = 0; return ++s; }
}  // namespace grb

using grb::CsrDerived; using grb::DevBuf; using grb::DevCSR;

// x86-64 / libstdc++ and libc++, from the build (DevBuf: p 8 | bytes 8 | serial 8 | borrowed 1 (+7) = 32): plan_blocks 32 | plan_nblocks 4 (+4) | plan_aux 32 |
// plan_nlong 4 | has_plan 1 (+3) | range_state 4 (+4) | range_abs 8 | locality_pct 4 (+4) | wp_rs, wp_hot, wp_pcol, wp_carry 128 | wp_nhot, wp_ntasks, wp_nwarm 12 |
// wp_tsize 4 | xcd 16 | heads, nonempty 64 | heads_valid, heads_vals 2 (+2) | pipe_uses 4 = 336
static_assert(sizeof(DevBuf) == 32, "DevBuf changed: check the field list below");
static_assert(sizeof(CsrDerived) == 336, "a field was added to or taken from CsrDerived: extend Field, NAME, snap(), set_all() and the field list above, then this number");

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

enum Field { plan_blocks, plan_nblocks, plan_aux, plan_nlong, has_plan, range_state, range_abs, locality_pct, wp_rs, wp_hot, wp_pcol, wp_carry, wp_nhot, wp_ntasks,
             wp_nwarm, wp_tsize, xcd, heads, nonempty, heads_valid, heads_vals, pipe_uses, NFIELDS };
static const char* const NAME[NFIELDS] = {"plan_blocks", "plan_nblocks", "plan_aux", "plan_nlong", "has_plan", "range_state", "range_abs", "locality_pct", "wp_rs", "wp_hot",
                                          "wp_pcol", "wp_carry", "wp_nhot", "wp_ntasks", "wp_nwarm", "wp_tsize", "xcd", "heads", "nonempty", "heads_valid", "heads_vals",
                                          "pipe_uses"};
constexpr int NBUFS = 9;      // the eight DevBufs of the record and the one inside the stand-in for kernel X's plan
typedef std::array<uint64_t, NFIELDS> Snap;      // one comparable word per field: a buffer by its address, the range by its bits
static uint64_t bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static Snap snap(const CsrDerived& d) {
  Snap s;
  s[plan_blocks] = (uintptr_t)d.plan_blocks.p; s[plan_nblocks] = d.plan_nblocks; s[plan_aux] = (uintptr_t)d.plan_aux.p; s[plan_nlong] = d.plan_nlong; s[has_plan] = d.has_plan;
  s[range_state] = (uint64_t)d.range_state; s[range_abs] = bits(d.range_abs); s[locality_pct] = (uint64_t)d.locality_pct;
  s[wp_rs] = (uintptr_t)d.wp_rs.p; s[wp_hot] = (uintptr_t)d.wp_hot.p; s[wp_pcol] = (uintptr_t)d.wp_pcol.p; s[wp_carry] = (uintptr_t)d.wp_carry.p;
  s[wp_nhot] = d.wp_nhot; s[wp_ntasks] = d.wp_ntasks; s[wp_nwarm] = d.wp_nwarm; s[wp_tsize] = (uint64_t)d.wp_tsize;
  s[xcd] = (uintptr_t)d.xcd.get();
  s[heads] = (uintptr_t)d.heads.p; s[nonempty] = (uintptr_t)d.nonempty.p; s[heads_valid] = d.heads_valid; s[heads_vals] = d.heads_vals;
  s[pipe_uses] = d.pipe_uses;
  return s;
}

struct XPlanStandIn { DevBuf copy{64}; };      // kernel X's plan owns device buffers: dropping the plan must free them

static void set_all(CsrDerived& d) {
  d.plan_blocks.alloc(48); d.plan_nblocks = 3; d.plan_aux.alloc(40); d.plan_nlong = 2; d.has_plan = true;
  d.range_state = 1; d.range_abs = 12.5; d.locality_pct = 37;
  d.wp_rs.alloc(16); d.wp_hot.alloc(24); d.wp_pcol.alloc(32); d.wp_carry.alloc(8); d.wp_nhot = 5; d.wp_ntasks = 7; d.wp_nwarm = 6; d.wp_tsize = 8;
  d.xcd = std::make_shared<XPlanStandIn>();
  d.heads.alloc(64); d.nonempty.alloc(68); d.heads_valid = true; d.heads_vals = true;
  d.pipe_uses = 2;
}
// a CSR with an image (three allocations) and everything derived
static void fill(DevCSR& m) {
  m.nrows = 4; m.ncols = 5; m.nnz = 6; m.rowptr.alloc(20); m.col.alloc(24); m.val.alloc(48); m.valid = true;
  set_all(m.derived);
}

// every field in `cleared` equals the default record's, every other one is what it was
static void expect(const CsrDerived& d, const Snap& was, const Snap& fresh, std::initializer_list<Field> cleared, const char* what) {
  bool is_cleared[NFIELDS] = {false}; for (Field f : cleared) is_cleared[f] = true;
  const Snap now = snap(d);
  for (int f = 0; f < NFIELDS; f++) {
    const uint64_t want = is_cleared[f] ? fresh[f] : was[f];
    if (now[f] != want) { failures++; printf("FAILED %s: %s is %s\n", what, NAME[f], is_cleared[f] ? "not at its default" : "not what it was"); }
  }
}
static const std::initializer_list<Field> ALL = {plan_blocks, plan_nblocks, plan_aux, plan_nlong, has_plan, range_state, range_abs, locality_pct, wp_rs, wp_hot, wp_pcol, wp_carry,
                                                wp_nhot, wp_ntasks, wp_nwarm, wp_tsize, xcd, heads, nonempty, heads_valid, heads_vals, pipe_uses};
static bool image_intact(const DevCSR& m) { return m.nrows == 4 && m.ncols == 5 && m.nnz == 6 && m.rowptr.p && m.col.p && m.val.p && m.valid; }

int main() {
  const Snap fresh = snap(CsrDerived());
  CHECK(fresh[locality_pct] == (uint64_t)-1 && fresh[range_state] == 0 && fresh[pipe_uses] == 0 && fresh[xcd] == 0, "defaults: nothing derived yet");
  CHECK(ALL.size() == NFIELDS, "ALL names %zu of %d fields", ALL.size(), (int)NFIELDS);
  {
    CsrDerived d; set_all(d); const Snap s = snap(d); int same = 0;
    for (int f = 0; f < NFIELDS; f++) if (s[f] == fresh[f]) { same++; printf("set_all leaves %s at its default\n", NAME[f]); }
    CHECK(same == 0, "set_all leaves %d field(s) at their defaults", same);
    CHECK(live == NBUFS, "set_all: %ld live allocations, expected %d", live, NBUFS);
  }
  CHECK(live == 0, "a record that goes out of scope frees its buffers: %ld live", live);

  {
    DevCSR m; fill(m); const Snap was = snap(m.derived);
    CHECK(live == 3 + NBUFS, "fill: %ld live allocations", live);
    m.derived.structure_changed();
    expect(m.derived, was, fresh, ALL, "structure_changed");
    CHECK(live == 3, "structure_changed: %ld live allocations, expected the image's three", live);
    CHECK(image_intact(m), "structure_changed: the image is untouched");
  }
  CHECK(live == 0, "after structure_changed: %ld live", live);

  {
    DevCSR m; fill(m); const Snap was = snap(m.derived);
    m.derived.values_changed();
    expect(m.derived, was, fresh, {xcd, range_state, range_abs, heads_valid, heads_vals}, "values_changed");
    CHECK(live == 3 + NBUFS - 1, "values_changed: %ld live allocations, expected all but the one of kernel X's plan", live);
    CHECK(image_intact(m), "values_changed: the image is untouched");
  }

  {
    DevCSR m; fill(m); const Snap was = snap(m.derived);
    const DevCSR& seen_by_a_launcher = m;      // the launchers hold the CSR const: the record is mutable
    seen_by_a_launcher.derived.drop_wavepipe();
    expect(m.derived, was, fresh, {wp_rs, wp_hot, wp_pcol, wp_carry, wp_nhot, wp_ntasks, wp_nwarm, wp_tsize}, "drop_wavepipe");
    CHECK(live == 3 + NBUFS - 4, "drop_wavepipe: %ld live allocations, expected all but W's four", live);
    CHECK(image_intact(m), "drop_wavepipe: the image is untouched");
  }

  {
    DevCSR m; fill(m); const Snap was = snap(m.derived);
    m.clear();
    expect(m.derived, was, fresh, ALL, "clear");
    CHECK(live == 0, "clear: %ld live allocations", live);
    CHECK(!m.valid && m.nrows == 0 && m.ncols == 0 && m.nnz == 0 && !m.rowptr.p && !m.col.p && !m.val.p, "clear: the image fields are at their defaults");
  }

  {
    DevCSR m; fill(m); const Snap was = snap(m.derived);
    DevCSR next; next.nrows = 2; next.ncols = 2; next.nnz = 1; next.rowptr.alloc(12); next.col.alloc(4); next.val.alloc(8); next.valid = true;
    const void* rp = next.rowptr.p;
    m = std::move(next);
    expect(m.derived, was, fresh, ALL, "move assignment of a fresh CSR");
    CHECK(live == 3, "move assignment: %ld live allocations, expected the new image's three", live);
    CHECK(m.rowptr.p == rp && m.nrows == 2 && m.nnz == 1 && m.valid, "move assignment: the new image is installed");
  }
  CHECK(live == 0, "at the end: %ld live allocations", live);

  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("csr derived ok (sizeof %zu)\n", sizeof(CsrDerived));
  return 0;
}
