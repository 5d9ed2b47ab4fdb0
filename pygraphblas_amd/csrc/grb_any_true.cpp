// grb_any_true.cpp — the result summary of a BOOL product: "any stored value true", and the edges that leave the true entries (grb_spmv.hpp:
// SpmvCall::any_true, SpmvCall::fe_host).  Product machinery: the SpMV kernels write the words, GrB_Vector_reduce_BOOL and the direction choice of the next
// product read them (VecFacts::lor_state, fe_lb).
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_spmv.hpp"
#include <string.h>

namespace grb {

// ---- "any stored value true" of a BOOL product result (grb_spmv.hpp: SpmvCall::any_true) -----------------------------------
// One device word per thread.  Every product brings a fresh non-zero tag and its kernels store that tag, so the word never has
// to be cleared: it answers "true" for the vector that holds the tag it currently shows, and only the latest product's vector
// may ask (GrB_Vector_reduce_BOOL with LOR then reads four bytes instead of launching a kernel over the vector).
// Round 5: the summary of a BOOL result's true entries (SpmvCall::fe_host) — every workgroup of the product stores its (edge sum, entry count),
// tagged, into its own pair of page-locked HOST words, and the lookup spins until all pairs carry the product's tag: no copy, no stream
// synchronisation.
namespace {
constexpr size_t FE_HOST_PAIRS = 2048;
static_assert(FE_HOST_PAIRS >= FE_MAX_BLOCKS, "every workgroup that reports a summary needs a host word of its own");
struct AnyTrue { DevBuf word; GrB_Vector owner = nullptr; uint32_t tag = 0; bool fe_has = false; uint64_t fe_key = 0; uint32_t fe_nblocks = 0; unsigned long long* host = nullptr; unsigned long long* host_dev = nullptr; };
thread_local AnyTrue t_any;
}
uint32_t* any_true_acquire(uint32_t* tag) {
  AnyTrue& s = t_any;
  if (!s.word.p) {
    s.word.alloc(64); GRB_HIP(hipMemsetAsync(s.word.p, 0, 64, stream()));
    void* h = nullptr; GRB_HIP(hipHostMalloc(&h, FE_HOST_PAIRS * 8, hipHostMallocMapped | hipHostMallocCoherent)); memset(h, 0, FE_HOST_PAIRS * 8); s.host = (unsigned long long*)h;      // (lives as long as the thread's pinned scratch: never freed)
    void* dp = nullptr; if (hipHostGetDevicePointer(&dp, h, 0) != hipSuccess) { (void)hipGetLastError(); dp = h; }
    s.host_dev = (unsigned long long*)dp;
    if (const char* e = getenv("GRB_MI355X_SUMMARY_TAG0")) s.tag = (uint32_t)strtoul(e, nullptr, 0);      // test hook: start the tags just below the 24-bit wrap
  }
  if ((++s.tag & 0xFFFFFFu) == 0) {                   // (the low 24 bits travel in the host words of the summary: never zero)
    s.tag++;
    // the 24-bit tags start over: a word that a product 2^24 calls ago left unread (its summary was never asked for, and no product since had as many
    // workgroups) must not pass for the coming product's — once per 16.7 million products, wait for the stream and wipe the words
    GRB_HIP(hipStreamSynchronize(stream())); memset(s.host, 0, FE_HOST_PAIRS * 8);
  }
  s.owner = nullptr; s.fe_has = false; *tag = s.tag;
  return s.word.as<uint32_t>();
}
unsigned long long* fe_summary_host() { return t_any.host_dev; }      // (after any_true_acquire)
void any_true_written(GrB_Vector w, const void* key, uint32_t tag, uint64_t fe_key, uint32_t fe_nblocks) {
  AnyTrue& s = t_any;
  s.owner = w; s.fe_has = fe_key != 0 && w != nullptr && fe_nblocks > 0 && fe_nblocks <= FE_HOST_PAIRS; s.fe_key = fe_key; s.fe_nblocks = fe_nblocks;
  if (w) { w->facts.lor_state = 1; w->facts.lor_key = key; w->facts.lor_tag = tag; }
}
bool any_true_lookup(GrB_Vector u, bool* value) {
  if (!u->facts.lor_state || u->lazy || u->q_reads || !u->dev_valid || u->dval.p != u->facts.lor_key) return false;
  if (u->facts.lor_state == 1) {
    AnyTrue& s = t_any;
    if (s.owner != u || s.tag != u->facts.lor_tag) { u->facts.lor_state = 0; return false; }
    if (s.fe_has) {
      // every workgroup stores  tag (24 bits) | true entries, saturating (8) | edge sum, saturating (32)  into its host word: wait for all of them,
      // and clear what was read (a word is never mistaken for a later product's with the same 24-bit tag)
      volatile unsigned long long* h = s.host; const unsigned long long want = (unsigned long long)(u->facts.lor_tag & 0xFFFFFFu);
      unsigned long long fe = 0, cnt = 0; uint32_t i = 0; const uint32_t nb = s.fe_nblocks;
      for (int round = 0; round < 2 && i < nb; round++) {
        for (uint64_t spin = 0; spin < (1ull << 22) && i < nb;) {
          const unsigned long long a = h[i];
          if ((a >> 40) == want && a != 0) { fe += a & 0xFFFFFFFFull; cnt += (a >> 32) & 0xFFull; h[i] = 0; i++; } else { spin++; __builtin_ia32_pause(); }
        }
        if (i < nb) GRB_HIP(hipStreamSynchronize(stream()));      // (far beyond any product's time: let a failed launch report itself, then look once more)
      }
      s.owner = nullptr; s.fe_has = false;
      if (i < nb) { u->facts.lor_state = 0; return false; }
      u->facts.lor_state = cnt ? 3 : 2;
      u->facts.fe_lb = fe; u->facts.fe_lb_key = s.fe_key; u->facts.fe_lb_true = true;      // the edges leaving u's true entries (exact when the kernel counted: a lower bound is all the direction choice asks for)
    } else {
      uint32_t* pin = (uint32_t*)pinned_scratch();
      GRB_HIP(hipMemcpyAsync(pin, s.word.p, 4, hipMemcpyDeviceToHost, stream()));
      GRB_HIP(hipStreamSynchronize(stream()));
      u->facts.lor_state = pin[0] == u->facts.lor_tag ? 3 : 2; s.owner = nullptr;
    }
  }
  *value = u->facts.lor_state == 3; return true;
}

}  // namespace grb
