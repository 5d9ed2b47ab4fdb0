// grb_compact.hip — bitmap compaction (grb_compact.hpp): the bytes widened to 0/1 words, rocPRIM's exclusive scan over them, and one scatter kernel.
// Streaming passes: 256 threads, a capped grid with a loop past the cap, no LDS, no atomics, every output place has one writer.
//   traffic             scan: read n bytes, write and read 4 (n + 1) flag bytes, write 4 (n + 1) position bytes.
//                       scatter: read n bytes, and per present position 4 position bytes (+ ts value bytes); written 4 (+ ts) bytes per present position.
#include "grb_compact.hpp"

namespace grb {
namespace {

__global__ void k_present_to_u32(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t* __restrict__ out) {      // out[n] = 0: the scan's last word is the total
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= n; i += gridDim.x * 256ull) out[i] = (i < n && bytes[i]) ? 1u : 0u;
}

// TS == 0: positions only, no value is loaded.  COL is a CompactCol: the division exists in the COMPACT_COL_MOD instances alone.
template <int TS, int COL>
__global__ void k_scatter_present(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ pos, uint64_t n, uint32_t base, uint64_t ncols, uint32_t* __restrict__ ocol,
                                  const uint8_t* __restrict__ val, uint8_t* __restrict__ oval) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) if (bytes[i]) {
    const size_t w = (size_t)base + pos[i];
    if (ocol) ocol[w] = COL == COMPACT_COL_INDEX ? (uint32_t)i : COL == COMPACT_COL_MOD ? (uint32_t)(i % ncols) : 0u;
    if constexpr (TS != 0) ((W*)oval)[w] = ((const W*)val)[i];
  }
}

template <int TS> void launch_scatter(const uint8_t* bytes, const uint32_t* pos, uint64_t n, uint32_t base, CompactCol column, uint64_t ncols, uint32_t* ocol, const void* val, void* oval, unsigned grid) {
#define GRB_SCATTER(COL) hipLaunchKernelGGL((k_scatter_present<TS, COL>), dim3(grid), dim3(256), 0, stream(), bytes, pos, n, base, ncols, ocol, (const uint8_t*)val, (uint8_t*)oval)
  switch (column) { case COMPACT_COL_INDEX: GRB_SCATTER(COMPACT_COL_INDEX); break; case COMPACT_COL_MOD: GRB_SCATTER(COMPACT_COL_MOD); break; default: GRB_SCATTER(COMPACT_COL_ZERO); }
#undef GRB_SCATTER
}

}  // namespace

void present_positions(const uint8_t* bytes, uint64_t n, uint32_t* pos, uint64_t grid_cap) {
  DevBuf flags((n + 1) * 4);
  hipLaunchKernelGGL(k_present_to_u32, dim3(grid_1d(n + 1, grid_cap)), dim3(256), 0, stream(), bytes, n, flags.as<uint32_t>());
  exclusive_scan_u32(flags.as<uint32_t>(), pos, n + 1);
  // `flags` returns to the pool here with the scan still queued, and needs no synchronisation for it: the pool's reuse is stream-ordered (every kernel runs on the
  // one library stream, grb_runtime.cpp dev_free), so whoever gets the block next writes it after the scan has read it
}

uint32_t present_positions_total(const uint8_t* bytes, uint64_t n, uint32_t* pos, uint64_t grid_cap) {
  present_positions(bytes, n, pos, grid_cap);
  uint32_t* pin = (uint32_t*)pinned_scratch();
  GRB_HIP(hipMemcpyAsync(pin, pos + n, 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  return pin[0];
}

void scatter_present(const uint8_t* bytes, const uint32_t* pos, uint64_t n, uint32_t base, CompactCol column, uint64_t ncols, uint32_t* ocol, size_t ts, const void* val, void* oval,
                     uint64_t grid_cap) {
  if (!n) return;
  if (column == COMPACT_COL_MOD && !ncols) fail(GrB_PANIC, "compaction: a bitmap of rows needs the row length");
  const unsigned grid = grid_1d(n, grid_cap);
  if (!oval) launch_scatter<0>(bytes, pos, n, base, column, ncols, ocol, nullptr, nullptr, grid);
  else { check_value_size(ts, "compaction"); dispatch_value_size(ts, [&]<int TS>() { launch_scatter<TS>(bytes, pos, n, base, column, ncols, ocol, val, oval, grid); }); }
}

}  // namespace grb
