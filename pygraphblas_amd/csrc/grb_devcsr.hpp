// grb_devcsr.hpp — the device image of a matrix (CSR in HBM, or the bitmap of a batch matrix) and what the library derives from a CSR image so that the next
// product can skip work.  Plain C++: no HIP, and the allocator is only declared (the runtime defines it for the library), so that a stand-alone program can check
// the transitions under the sanitizers (tests/csr_derived_check.cpp).
//
// THE RULE.  Everything in DevCSR::derived is valid only for the image it was derived from.  The transitions of CsrDerived (and DevCSR::clear) are the only code
// that clears derived state; whoever writes an image passes exactly one of them, and a writer that knows something about the new image states it afterwards in
// plain assignments.  No transition takes a flag that keeps a cache.  A planner that reads the image and derives something from it fills `derived` without a
// transition: a cache filled on first use, which is why the member is `mutable` and the planners take `const DevCSR&`.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <memory>

namespace grb {

void* dev_alloc(size_t bytes);    // pooled hipMalloc; throws GrbError(OUT_OF_MEMORY/PANIC)
void dev_free(void* p);
uint64_t dev_alloc_serial();      // a number no other allocation of this process gets (the pool hands the same addresses out again)

// owning device buffer
struct DevBuf {
  void* p = nullptr; size_t bytes = 0;
  uint64_t serial = 0;              // identifies this allocation where a raw address could be a recycled one (VecFacts::fe_lb_key)
  bool borrowed = false;            // a view of memory another DevBuf owns (a row of a batch matrix's bitmap handed to a vector kernel, grb_mxm_rows.cpp): never freed here
  DevBuf() {}
  explicit DevBuf(size_t n) { alloc(n); }
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), serial(o.serial), borrowed(o.borrowed) { o.p = nullptr; o.bytes = 0; o.serial = 0; o.borrowed = false; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; bytes = o.bytes; serial = o.serial; borrowed = o.borrowed; o.p = nullptr; o.bytes = 0; o.serial = 0; o.borrowed = false; } return *this; }
  ~DevBuf() { reset(); }
  void alloc(size_t n) { reset(); if (n) { p = dev_alloc(n); bytes = n; serial = dev_alloc_serial(); } }
  void borrow(void* q, size_t n) { reset(); p = q; bytes = n; serial = dev_alloc_serial(); borrowed = true; }
  void reset() { if (p && !borrowed) dev_free(p); p = nullptr; bytes = 0; serial = 0; borrowed = false; }
  template <class T> T* as() const { return (T*)p; }
};

// ---- what is derived from a CSR image ---------------------------------------------------------
// A default-constructed record means "nothing derived yet".
struct CsrDerived {
  // SpMV row-block plan (grb_spmv.hip): blocks of consecutive rows holding <= SPMV_BLOCK_NNZ
  // entries, long rows split into parts.  Built on first mxv, cached with the matrix.
  DevBuf plan_blocks; uint32_t plan_nblocks = 0; DevBuf plan_aux; uint32_t plan_nlong = 0;
  bool has_plan = false;
  int range_state = 0;          // largest |value| of the stored values: 0 not measured, 1 = range_abs holds it, 2 = not usable (NaN / infinity / a type without a range)
  double range_abs = 0;         // (as a double: an upper bound is all the caller needs — grb_mxv.cpp "big holes")
  int locality_pct = -1;        // share of entries whose column is < 16 behind its predecessor in the row (measured once, -1 = not yet): gathers with locality need no panels
  // kernel-W plan (grb_spmv_wavepipe.hpp): per-task first row, hot-column list, remapped column array, per-wave carries
  DevBuf wp_rs, wp_hot, wp_pcol, wp_carry; uint32_t wp_nhot = 0, wp_ntasks = 0, wp_nwarm = 0; int wp_tsize = 0;
  std::shared_ptr<void> xcd;    // kernel-X plan (grb_spmv_xcd.hpp: XcdPlan), panel-major copy of the matrix
  // row heads (grb_spmv_kernels.hpp, round 5): for the masked pull of a BFS level — per row its first four entries as one 16-byte word (per entry:
  // bits 29..0 the column, bit 31 its BOOL value, in the fourth bit 30 = the row has more entries; absent = 0xFFFFFFFF) and one bit per row "has an
  // entry": a level then costs what its unvisited NON-EMPTY rows cost, and a row decided by its first entries never touches the column array.
  // Built at the first masked pull of a matrix with < 2^30 - 1 columns; heads_vals: the value bits come from one-byte BOOL values (else they are 1).
  DevBuf heads, nonempty; bool heads_valid = false, heads_vals = false;
  uint32_t pipe_uses = 0;       // full-operand pull products this matrix has served: the first runs kernel W (cheap plan), kernel X's plan is built for the second

  // ---- the transitions ----
  // rows, columns or the entry set changed: nothing derived is left, the buffers are freed (assignment from a default record: a field added later cannot be missed)
  void structure_changed() { *this = CsrDerived(); }
  // values were overwritten in place, the structure is what it was
  void values_changed() {
    xcd.reset();                                      // X's plan may hold a copy of the values (XcdPlan::has_vals)
    range_state = 0; range_abs = 0;                   // the largest |value| is a fact about the values
    heads_valid = false; heads_vals = false;          // the row heads carry the BOOL value bits of each row's first four entries (the buffers stay: rebuilt into)
    // kept: the row-block plan (rows and entry counts only), W's plan (it holds no matrix values: columns remapped, the values are read from the image),
    // locality_pct (a fact about the columns) and pipe_uses (a count of products, not of images)
  }
  // kernel X's plan supersedes kernel W's: W's copy of the column array goes
  void drop_wavepipe() { wp_rs.reset(); wp_hot.reset(); wp_pcol.reset(); wp_carry.reset(); wp_nhot = wp_ntasks = wp_nwarm = 0; wp_tsize = 0; }
};

// ---- device CSR ---------------------------------------------------------------------------
struct DevCSR {
  uint32_t nrows = 0, ncols = 0; uint64_t nnz = 0;
  DevBuf rowptr, col, val;      // u32[nrows+1], u32[nnz], T[nnz]
  bool valid = false;
  mutable CsrDerived derived;   // caches of this image, filled on first use by the planners (see THE RULE)
  // no image: the caller sets the dimensions of the next one
  void clear() { nrows = ncols = 0; nnz = 0; rowptr.reset(); col.reset(); val.reset(); valid = false; derived.structure_changed(); }
};

// A matrix of a few very long rows (the ns x n batches of the reference's betweenness centrality, gap/bcmark.py:16-67) as a BITMAP: val T[nrows x ncols]
// | pres u8[nrows x ncols], row-major — i.e. ns bitmap vectors back to back, or one bitmap vector of nrows x ncols positions.  Round 6: such a matrix may
// live in this form alone (dev_valid == host_valid == false, bm.valid == true): the batch operations (grb_mxm_rows.cpp) read and write it directly, and the
// CSR is made from it only when something else asks (mat_to_device).
struct DevBitmap { DevBuf val, pres; bool valid = false; uint64_t nvals = 0; bool nvals_known = false;
                   void clear() { val.reset(); pres.reset(); valid = false; nvals = 0; nvals_known = false; } };

}  // namespace grb
