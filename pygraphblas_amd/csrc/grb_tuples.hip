// grb_tuples.hip — extractTuples in HBM: a device CSR to the lists (I, J, X), a bitmap vector to the ordered lists (I, X), the outputs 64-bit indices and values
// of the container's own type in arrays the caller owns (torch tensors, usually).  The entry points and what they do before the kernels run (the flush, the
// upload of a host-resident container, the capacity test) are GrBX_*_extractTuples_at in grb_tuples_ops.cpp; the tile arithmetic is grb_tuples_geom.hpp.
// All kernels: wave64, 256 threads, a capped grid with a loop past the cap, no LDS, no atomics, plain vector stores.
//
//   k_tuples_csr<TS>    one pass over tiles of TUPLES_TILE consecutive ENTRIES.  Per entry it reads col (4 B) and val (TS B) and writes I (8 B), J (8 B, the
//                       column zero-extended) and X (TS B).  The row of an entry comes from rowptr: the workgroup brackets its tile's rows (tuples_row_of over
//                       the whole row pointer for the first entry — every lane the same loads, served as broadcasts — and tuples_row_from for the last), and
//                       each lane bisects inside the bracket, which is a handful of rows unless empty rows lie in it.  The work is balanced by entries: a row
//                       of 10^5 entries is a hundred tiles whose bracket is that one row, a run of empty rows costs the bisection its logarithm and nothing else.
//                       Streams: with 16-byte aligned outputs a lane holds two neighbouring entries and stores 16 B into I and into J, and X is copied as 16-byte
//                       words; an output that is only 8-byte aligned (a tensor slice) takes the other instantiation, one entry per lane and round.  Either way a
//                       wave's stores of one instruction are one contiguous run.  A stream whose pointer is NULL is neither computed nor written: without I no
//                       row pointer is read at all.
//   k_tuples_count      vector, pass 1: present bytes (pres[p] != 0: GrBX_Vector_import_Bitmap's rule) per TUPLES_VEC_WAVE positions, four wave ballots each.
//   (scan)              exclusive_scan_u32 over the count words; the last word is nvals, read back for the capacity test before anything is written.
//   k_tuples_scatter<TS> pass 2: the same ballots; a lane's rank inside its round is the ballot's prefix popcount (mbcnt), so I[rank] = p, X[rank] = val[p]
//                       land in ascending order and a round's stores are one contiguous run.
//   k_tuples_iota       a vector whose facts say "all present" skips both passes: I[p] = p, and X is a device-to-device copy of the values.
#include "grb_tuples.hpp"
#include "grb_index.hpp"

namespace grb {
namespace {

static_assert(TUPLES_GRID_CAP == 4096, "GrBX_tuples_geometry reports the cap grid_1d gives the other O(nnz) kernels");

struct alignas(16) U64x2 { uint64_t a, b; };

template <int TS, bool WIDE_IJ, bool WIDE_X>
__global__ __launch_bounds__(256) void k_tuples_csr(const uint32_t* __restrict__ rowptr, uint32_t nrows, const uint32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                    uint64_t nnz, uint64_t ntiles, uint64_t* __restrict__ I, uint64_t* __restrict__ J, uint8_t* __restrict__ X) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = tuples_tile_begin(t, TUPLES_TILE), end = tuples_tile_end(t, TUPLES_TILE, nnz);      // base < end <= nnz <= 0xFFFFFFF0: entries are 32-bit words in rowptr
    uint32_t rlo = 0, rhi = 0;                                                                                // the rows of the tile's first and last entry
    if (I) { rlo = tuples_row_of(rowptr, 0, nrows - 1, (uint32_t)base); rhi = tuples_row_from(rowptr, rlo, nrows - 1, (uint32_t)(end - 1)); }
    if constexpr (WIDE_IJ) {
      for (uint64_t e = base + 2ull * threadIdx.x; e < end; e += 2ull * TUPLES_THREADS) {                     // e is even: I + e and J + e are 16-byte aligned
        const bool two = e + 1 < end;
        if (I) {
          const uint32_t r0 = tuples_row_of(rowptr, rlo, rhi, (uint32_t)e);
          uint32_t r1 = r0;
          if (two && rowptr[r0 + 1] <= (uint32_t)(e + 1)) r1 = tuples_row_of(rowptr, r0 + 1, rhi, (uint32_t)(e + 1));      // (then r0 < rhi: the tile's last entry lies in rhi)
          if (two) *(U64x2*)(I + e) = U64x2{r0, r1}; else I[e] = r0;
        }
        if (J) { const uint32_t c0 = col[e]; if (two) *(U64x2*)(J + e) = U64x2{c0, col[e + 1]}; else J[e] = c0; }
      }
    } else {
      for (uint64_t e = base + threadIdx.x; e < end; e += TUPLES_THREADS) {
        if (I) I[e] = tuples_row_of(rowptr, rlo, rhi, (uint32_t)e);
        if (J) J[e] = col[e];
      }
    }
    if (X) {
      const uint64_t cnt = end - base; uint64_t done = 0;
      if constexpr (WIDE_X) {                                           // base * TS is a multiple of 16: the tile's values begin on a 16-byte boundary of both arrays
        constexpr uint32_t PER = 16 / TS;
        const uint64_t chunks = cnt / PER;
        const uint4* s = (const uint4*)(val + base * TS); uint4* d = (uint4*)(X + base * TS);
        for (uint64_t c = threadIdx.x; c < chunks; c += TUPLES_THREADS) d[c] = s[c];
        done = chunks * PER;                                            // (the last tile's tail: fewer than PER values)
      }
      for (uint64_t k = done + threadIdx.x; k < cnt; k += TUPLES_THREADS) ((W*)X)[base + k] = ((const W*)val)[base + k];
    }
  }
}

// lanes below this one among the set bits of a ballot
__device__ __forceinline__ uint32_t ballot_rank(uint64_t mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)); }

// word q counts the present positions of [q * TUPLES_VEC_WAVE, (q + 1) * TUPLES_VEC_WAVE); q depends on the wave only, so the ballots are convergent
__global__ __launch_bounds__(256) void k_tuples_count(const uint8_t* __restrict__ pres, uint64_t n, uint64_t nwords, uint32_t* __restrict__ counts) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t q = blockIdx.x * 4ull + (threadIdx.x >> 6); q < nwords; q += gridDim.x * 4ull) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t r = 0; r < TUPLES_VEC_WAVE / 64; r++) { const uint64_t p = q * TUPLES_VEC_WAVE + r * 64u + lane; c += (uint32_t)__popcll(__ballot(p < n && pres[p] != 0)); }
    if (lane == 0) counts[q] = c;
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_tuples_scatter(const uint8_t* __restrict__ pres, const uint8_t* __restrict__ val, uint64_t n, uint64_t nwords, const uint32_t* __restrict__ offs,
                                                        uint64_t* __restrict__ I, uint8_t* __restrict__ X) {
  typedef typename WordOf<TS>::type W;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t q = blockIdx.x * 4ull + (threadIdx.x >> 6); q < nwords; q += gridDim.x * 4ull) {
    uint64_t rank0 = offs[q];                                           // (offs[q] + the word's count = offs[q + 1] <= nvals: every rank below is inside the outputs)
#pragma unroll
    for (uint32_t r = 0; r < TUPLES_VEC_WAVE / 64; r++) {
      const uint64_t p = q * TUPLES_VEC_WAVE + r * 64u + lane;
      const bool here = p < n && pres[p] != 0;
      const uint64_t mask = __ballot(here);
      if (here) { const uint64_t k = rank0 + ballot_rank(mask); if (I) I[k] = p; if (X) ((W*)X)[k] = ((const W*)val)[p]; }
      rank0 += (uint32_t)__popcll(mask);
    }
  }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_tuples_iota(uint64_t* __restrict__ I, uint64_t n) {
  if constexpr (WIDE) {
    for (uint64_t p = (blockIdx.x * 256ull + threadIdx.x) * 2; p < n; p += gridDim.x * 512ull) { if (p + 1 < n) *(U64x2*)(I + p) = U64x2{p, p + 1}; else I[p] = p; }
  } else {
    for (uint64_t p = blockIdx.x * 256ull + threadIdx.x; p < n; p += gridDim.x * 256ull) I[p] = p;
  }
}

inline bool aligned16(const void* p) { return tuples_aligned16((uint64_t)(uintptr_t)p); }

}  // namespace

void tuples_from_csr(const DevCSR& A, size_t ts, uint64_t* I, uint64_t* J, void* X) {
  check_value_size(ts, "extractTuples");
  const uint64_t nnz = A.nnz;
  if (!nnz || (!I && !J && !X)) return;
  if (!A.nrows || nnz > GRB_DIM_DEVICE_MAX) fail(GrB_PANIC, "extractTuples: the CSR does not fit the 32-bit device layout");      // (the kernels' bounds depend on it)
  const uint64_t ntiles = tuples_tiles(nnz, TUPLES_TILE);
  const bool wide_ij = aligned16(I) && aligned16(J), wide_x = aligned16(X) && aligned16(A.val.p);
  dispatch_value_size(ts, [&]<int TS>() {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(tuples_grid(ntiles)), dim3(TUPLES_THREADS), 0, stream(), A.rowptr.as<uint32_t>(), A.nrows, A.col.as<uint32_t>(), A.val.as<uint8_t>(),
                         nnz, ntiles, I, J, (uint8_t*)X);
    };
    if (wide_ij) { if (wide_x) launch(k_tuples_csr<TS, true, true>); else launch(k_tuples_csr<TS, true, false>); }
    else { if (wide_x) launch(k_tuples_csr<TS, false, true>); else launch(k_tuples_csr<TS, false, false>); }
  });
  GRB_HIP(hipGetLastError());
}

uint64_t tuples_count_bitmap(const uint8_t* pres, uint64_t n, DevBuf& offs) {
  const uint64_t nwords = tuples_tiles(n, TUPLES_VEC_WAVE);
  DevBuf counts((nwords + 1) * 4); offs.alloc((nwords + 1) * 4);
  GRB_HIP(hipMemsetAsync(counts.as<uint32_t>() + nwords, 0, 4, stream()));      // the scan's last word is the total
  hipLaunchKernelGGL(k_tuples_count, dim3(tuples_grid(tuples_tiles(n, TUPLES_VEC_TILE))), dim3(TUPLES_THREADS), 0, stream(), pres, n, nwords, counts.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  exclusive_scan_u32(counts.as<uint32_t>(), offs.as<uint32_t>(), nwords + 1);
  uint32_t* pin = (uint32_t*)pinned_scratch();
  GRB_HIP(hipMemcpyAsync(pin, offs.as<uint32_t>() + nwords, 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  return pin[0];
}

void tuples_from_bitmap(const uint8_t* pres, const void* val, size_t ts, uint64_t n, const DevBuf& offs, uint64_t* I, void* X) {
  check_value_size(ts, "extractTuples");
  if (!I && !X) return;
  const uint64_t nwords = tuples_tiles(n, TUPLES_VEC_WAVE);
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_tuples_scatter<TS>), dim3(tuples_grid(tuples_tiles(n, TUPLES_VEC_TILE))), dim3(TUPLES_THREADS), 0, stream(), pres, (const uint8_t*)val, n, nwords,
                       offs.as<uint32_t>(), I, (uint8_t*)X);
  });
  GRB_HIP(hipGetLastError());
}

void tuples_from_full(const void* val, size_t ts, uint64_t n, uint64_t* I, void* X) {
  if (I) {
    if (aligned16(I)) hipLaunchKernelGGL((k_tuples_iota<true>), dim3(grid_1d((n + 1) / 2)), dim3(256), 0, stream(), I, n);
    else hipLaunchKernelGGL((k_tuples_iota<false>), dim3(grid_1d(n)), dim3(256), 0, stream(), I, n);
    GRB_HIP(hipGetLastError());
  }
  if (X) GRB_HIP(hipMemcpyAsync(X, val, n * ts, hipMemcpyDeviceToDevice, stream()));
}

}  // namespace grb
