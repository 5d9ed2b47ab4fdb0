// grb_sort.hip — sorting by value in HBM: the rows of a CSR (behind GxB_Matrix_sort and GrBX_Matrix_select_topk) and a bitmap vector (behind GxB_Vector_sort and
// GrBX_Vector_select_topk); the routes are in grb_sort_ops.cpp, the order in grb_sort_keys.hpp.  Nothing here rebuilds a value from its key: every kernel
// sorts (key, place) pairs and hands the places on, the values are gathered through them afterwards.
//
//   csr_sort_positions  per entry place e of row r, i = e - rowptr[r]: perm[e] = the place of the row's i-th entry in sorted order, ocol[e] = i.
//     k_sort_bins       one pass over the row pointer: rows above 64 entries up to the LDS edge are appended to the LDS list, longer ones to the long list with a
//                       compact offset (one atomic each; rows up to 64 — nearly all rows of a power-law matrix — cost nothing here).  The three counts are the
//                       one read-back.
//     k_sort_wave       rows up to SORT_WAVE_MAX = 64: one wave, one element per lane, a bitonic network over lane exchanges (ds_bpermute / DPP — no LDS
//                       round trip, no barrier).  The comparison is on (key, place) pairs, so no two elements are equal and the result is the stable one; lanes
//                       past the row's end carry (all ones, all ones), above every real pair.  A wave takes four consecutive rows: when all four hold at most 16
//                       entries they are sorted together, 16 lanes each, by the 10 steps of the 16-wide network instead of four times the 21 steps of the
//                       64-wide one (one vote decides, wave-uniformly); otherwise one after the other.
//     k_sort_lds        rows above 64 up to the LDS edge (SORT_LDS_EDGE = 128 by default; at most SORT_LDS_MAX = 4096, the derived capacity): the pairs in LDS (the
//                       next power of two >= len, padded with the sentinel), the bitonic network with one barrier per step.  Two shapes: edges up to 512 run ONE
//                       WAVE per row over 6 KiB of LDS (many rows per compute unit, the barrier of a one-wave workgroup is free) — the shape the default route
//                       uses; larger edges one workgroup of four waves over 48 KiB, which measured slower than the segmented sort and is kept for comparison.
//     long rows         keys and places of just those rows packed into compact arrays (k_sort_long_keys), rocPRIM's segmented radix sort over them (stable,
//                       places ascending within a row, so ties come out right), and the result copied to perm / ocol (k_sort_long_finish).
//     prim_only         GRB_MI355X_SORT=prim: no bins; keys for every entry, the segmented sort over the row pointer itself, ocol by k_sort_rowcols.
//   csr_sort_fill       k_sort_gather: ENTRY-PARALLEL, a lane owns 4 consecutive places: one 16-byte load of perm, four gathered values stored as one pack
//                       (two for 8-byte values), four gathered columns widened to INT64 as two 16-byte stores.  Unaligned views and the tail go entry by entry.
//   topk_flags          k_topk_flags: keep[perm[e]] = ocol[e] < k.  The compaction itself is csr_compact's (grb_compact.hpp's scan), not a scan of this file.
//   vector              the present positions (present_positions / scatter_present), keys of the values there (k_vec_sort_keys), ONE device-wide
//                       radix_sort_pairs (stable, indices ascending), then k_vec_sort_fill writes the prefix 0 .. nvals - 1 and clears the rest.
// Every index read from perm / sidx is checked against the array it indexes before it is used: a place that a bug left unwritten costs a wrong answer, not a fault.
#include "grb_sort.hpp"
#include "grb_compact.hpp"
#include "grb_matops.hpp"
#include <algorithm>
#include <stdio.h>

namespace grb {

namespace {

constexpr int SORT_EPL = 4;                                                  // places per lane of the gather: 16 bytes of perm
constexpr uint64_t SORT_LDS_WAVE_MAX = 512;                                     // edges up to this: the LDS kernel runs one wave per row
constexpr uint32_t SORT_PACK_MAX = 16;                                       // four rows share a wave when each holds at most this many entries

template <int TS> struct alignas(TS * SORT_EPL > 16 ? 16 : TS * SORT_EPL) ValPack { typename WordOf<TS>::type v[SORT_EPL]; };
struct alignas(16) U32Pack { uint32_t c[SORT_EPL]; };
struct alignas(16) I64Pack { int64_t c[SORT_EPL]; };

template <class K> __device__ __forceinline__ bool pair_less(K ka, uint32_t pa, K kb, uint32_t pb) { return ka < kb || (ka == kb && pa < pb); }

// the bitonic network over W lanes (aligned groups of W lanes of the wave sort independently); ascending
template <class K, int W> __device__ __forceinline__ void bitonic_lanes(K& key, uint32_t& pos, int lane) {
#pragma unroll
  for (int k = 2; k <= W; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const K ok = shfl_xor_t<K>(key, j); const uint32_t op = shfl_xor_t<uint32_t>(pos, j);
      const bool lower = (lane & j) == 0, asc = k == W || (lane & k) == 0;
      const bool take_min = lower == asc, other_less = pair_less<K>(ok, op, key, pos);
      if (other_less == take_min) { key = ok; pos = op; }
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_sort_wave(uint32_t nrows, const uint32_t* __restrict__ rp, const T* __restrict__ kval, int gt, uint32_t wave_max, uint32_t* __restrict__ perm, uint32_t* __restrict__ ocol) {
  typedef typename SortKeyOf<T>::type K;
  const int lane = threadIdx.x & 63;
  const uint32_t pack_max = wave_max < SORT_PACK_MAX ? wave_max : SORT_PACK_MAX;      // (wave_max <= SORT_WAVE_MAX = 64: the lanes of a wave)
  const uint64_t wave = (blockIdx.x * 256ull + threadIdx.x) >> 6, nwaves = gridDim.x * 4ull, ngroups = ((uint64_t)nrows + 3) / 4;
  for (uint64_t g = wave; g < ngroups; g += nwaves) {
    const uint64_t r0 = g * 4, r = r0 + (lane >> 4);
    uint32_t lo = 0, len = 0;
    if (r < nrows) { lo = rp[r]; len = rp[r + 1] - lo; }
    if (__all(len <= pack_max)) {
      const uint32_t i = lane & 15;
      K key = ~(K)0; uint32_t pos = 0xFFFFFFFFu;
      if (i < len) { pos = lo + i; key = sort_key<T>(kval[pos], gt != 0); }
      bitonic_lanes<K, 16>(key, pos, lane);
      if (i < len) { perm[lo + i] = pos; ocol[lo + i] = i; }
    } else {
      for (int s = 0; s < 4 && r0 + s < nrows; s++) {
        const uint32_t lo2 = rp[r0 + s], len2 = rp[r0 + s + 1] - lo2;               // (wave-uniform)
        if (len2 == 0 || len2 > wave_max) continue;                  // longer rows are the other bins'
        K key = ~(K)0; uint32_t pos = 0xFFFFFFFFu;
        if ((uint32_t)lane < len2) { pos = lo2 + lane; key = sort_key<T>(kval[pos], gt != 0); }
        bitonic_lanes<K, 64>(key, pos, lane);
        if ((uint32_t)lane < len2) { perm[lo2 + lane] = pos; ocol[lo2 + lane] = (uint32_t)lane; }
      }
    }
  }
}

// NMAX elements of LDS, THREADS lanes per row: <4096, 256> one workgroup of four waves per row (the derived capacity), <512, 64> ONE WAVE per row for edges up to
// 512 — 6 KiB of LDS, so a compute unit holds many rows at once, the barrier of a one-wave workgroup costs nothing, and a row of 128 takes one pair per lane and step.
template <class T, int NMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void k_sort_lds(const uint32_t* __restrict__ rows, uint32_t nlist, const uint32_t* __restrict__ rp, const T* __restrict__ kval, int gt,
                                                      uint32_t* __restrict__ perm, uint32_t* __restrict__ ocol) {
  typedef typename SortKeyOf<T>::type K;
  static_assert(NMAX <= (int)SORT_LDS_MAX && NMAX >= 128 && (NMAX & (NMAX - 1)) == 0, "a power of two within the derived capacity");
  __shared__ K skey[NMAX];
  __shared__ uint32_t spos[NMAX];
  const uint32_t tid = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < nlist; q += gridDim.x) {
    const uint32_t r = rows[q], lo = rp[r], len = rp[r + 1] - lo;
    if (len > (uint32_t)NMAX) continue;                                              // (the bin pass sent only rows that fit: the LDS arrays' bound)
    uint32_t N = 128; while (N < len) N <<= 1;
    for (uint32_t i = tid; i < N; i += THREADS) {
      if (i < len) { skey[i] = sort_key<T>(kval[lo + i], gt != 0); spos[i] = lo + i; } else { skey[i] = ~(K)0; spos[i] = 0xFFFFFFFFu; }
    }
    __syncthreads();
    for (uint32_t k = 2; k <= N; k <<= 1) {
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t p = tid; p < N / 2; p += THREADS) {
          const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;       // i has bit j clear; i, l < N
          const bool asc = (i & k) == 0;                                             // (k == N: i < N, always ascending)
          const K ka = skey[i], kb = skey[l]; const uint32_t pa = spos[i], pb = spos[l];
          if (pair_less<K>(kb, pb, ka, pa) == asc) { skey[i] = kb; spos[i] = pb; skey[l] = ka; spos[l] = pa; }
        }
        __syncthreads();
      }
    }
    for (uint32_t i = tid; i < len; i += THREADS) { perm[lo + i] = spos[i]; ocol[lo + i] = i; }
    __syncthreads();
  }
}

// cnt[0] rows of the LDS bin, cnt[1] rows of the long bin, cnt[2] their entries.  The lists' capacities follow from the entry count (a row of the LDS bin holds
// more than wave_max entries, one of the long bin more than lds_max), so the checks below never drop a row; they bound the stores.
__global__ __launch_bounds__(256) void k_sort_bins(uint32_t nrows, const uint32_t* __restrict__ rp, uint32_t wave_max, uint32_t lds_max, uint32_t* __restrict__ cnt,
                                                   uint32_t* __restrict__ lds_rows, uint32_t cap_lds, uint32_t* __restrict__ long_rows, uint32_t* __restrict__ long_begin,
                                                   uint32_t* __restrict__ long_end, uint32_t cap_long) {
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < nrows; r += gridDim.x * 256ull) {
    const uint32_t len = rp[r + 1] - rp[r];
    if (len > lds_max) {
      const uint32_t s = atomicAdd(&cnt[1], 1u), off = atomicAdd(&cnt[2], len);
      if (s < cap_long) { long_rows[s] = (uint32_t)r; long_begin[s] = off; long_end[s] = off + len; }
    } else if (len > wave_max) {
      const uint32_t s = atomicAdd(&cnt[0], 1u);
      if (s < cap_lds) lds_rows[s] = (uint32_t)r;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_sort_long_keys(uint32_t nlong, const uint32_t* __restrict__ long_rows, const uint32_t* __restrict__ long_begin, const uint32_t* __restrict__ rp,
                                                        const T* __restrict__ kval, int gt, uint32_t total, typename SortKeyOf<T>::type* __restrict__ kin, uint32_t* __restrict__ vin) {
  for (uint32_t q = blockIdx.x; q < nlong; q += gridDim.x) {
    const uint32_t r = long_rows[q], off = long_begin[q], lo = rp[r], len = rp[r + 1] - lo;
    for (uint32_t i = threadIdx.x; i < len; i += 256) if (off + i < total) { kin[off + i] = sort_key<T>(kval[lo + i], gt != 0); vin[off + i] = lo + i; }
  }
}
__global__ __launch_bounds__(256) void k_sort_long_finish(uint32_t nlong, const uint32_t* __restrict__ long_rows, const uint32_t* __restrict__ long_begin, const uint32_t* __restrict__ rp,
                                                          uint32_t total, const uint32_t* __restrict__ vout, uint32_t* __restrict__ perm, uint32_t* __restrict__ ocol) {
  for (uint32_t q = blockIdx.x; q < nlong; q += gridDim.x) {
    const uint32_t r = long_rows[q], off = long_begin[q], lo = rp[r], len = rp[r + 1] - lo;
    for (uint32_t i = threadIdx.x; i < len; i += 256) if (off + i < total) { perm[lo + i] = vout[off + i]; ocol[lo + i] = i; }
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_sort_keys_all(uint64_t n, const T* __restrict__ kval, int gt, typename SortKeyOf<T>::type* __restrict__ kin, uint32_t* __restrict__ vin) {
  for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < n; e += gridDim.x * 256ull) { kin[e] = sort_key<T>(kval[e], gt != 0); vin[e] = (uint32_t)e; }
}
// ocol[e] = e - rowptr[row of e]: a wave per row
__global__ __launch_bounds__(256) void k_sort_rowcols(uint32_t nrows, const uint32_t* __restrict__ rp, uint32_t* __restrict__ ocol) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (blockIdx.x * 256ull + threadIdx.x) >> 6, nwaves = gridDim.x * 4ull;
  for (uint64_t r = wave; r < nrows; r += nwaves) {
    const uint32_t lo = rp[r], len = rp[r + 1] - lo;
    for (uint32_t i = lane; i < len; i += 64) ocol[lo + i] = i;
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_sort_gather(uint64_t n, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ val, const uint32_t* __restrict__ col,
                                                     uint8_t* __restrict__ oval, int64_t* __restrict__ pval, int packed) {
  typedef typename WordOf<TS>::type W;
  const W* __restrict__ src = (const W*)val; W* __restrict__ dst = (W*)oval;
  const uint64_t ngroups = (n + SORT_EPL - 1) / SORT_EPL;
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < ngroups; g += gridDim.x * 256ull) {
    const uint64_t e0 = g * SORT_EPL;
    const int nv = n - e0 >= (uint64_t)SORT_EPL ? SORT_EPL : (int)(n - e0);
    if (nv == SORT_EPL && packed) {
      const U32Pack p = *reinterpret_cast<const U32Pack*>(perm + e0);
      if (dst) {
        ValPack<TS> v;
#pragma unroll
        for (int j = 0; j < SORT_EPL; j++) v.v[j] = p.c[j] < n ? src[p.c[j]] : W(0);
        *reinterpret_cast<ValPack<TS>*>(dst + e0) = v;
      }
      if (pval) {
        I64Pack c;
#pragma unroll
        for (int j = 0; j < SORT_EPL; j++) c.c[j] = p.c[j] < n ? (int64_t)col[p.c[j]] : 0;
        *reinterpret_cast<I64Pack*>(pval + e0) = c;
      }
    } else {
      for (int j = 0; j < nv; j++) {
        const uint32_t p = perm[e0 + j]; const bool ok = p < n;
        if (dst) dst[e0 + j] = ok ? src[p] : W(0);
        if (pval) pval[e0 + j] = ok ? (int64_t)col[p] : 0;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_topk_flags(uint64_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ ocol, uint64_t k, uint8_t* __restrict__ keep) {
  for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < n; e += gridDim.x * 256ull) { const uint32_t p = perm[e]; if (p < n) keep[p] = ocol[e] < k ? 1 : 0; }
}

template <class T>
__global__ __launch_bounds__(256) void k_vec_sort_keys(uint64_t nvals, uint64_t n, const uint32_t* __restrict__ idx, const T* __restrict__ kval, int gt, typename SortKeyOf<T>::type* __restrict__ keys) {
  typedef typename SortKeyOf<T>::type K;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < nvals; i += gridDim.x * 256ull) { const uint32_t p = idx[i]; keys[i] = p < n ? sort_key<T>(kval[p], gt != 0) : ~(K)0; }
}
template <int TS>
__global__ __launch_bounds__(256) void k_vec_sort_fill(uint64_t n, uint64_t nvals, const uint32_t* __restrict__ sidx, const uint8_t* __restrict__ uval, uint8_t* __restrict__ tval, uint8_t* __restrict__ tpres,
                                                       int64_t* __restrict__ pval, uint8_t* __restrict__ ppres) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const bool present = i < nvals;
    const uint32_t p = present ? sidx[i] : 0u; const bool ok = present && p < n;
    if (tval) { ((W*)tval)[i] = ok ? ((const W*)uval)[p] : W(0); tpres[i] = present ? 1 : 0; }
    if (pval) { pval[i] = ok ? (int64_t)p : 0; ppres[i] = present ? 1 : 0; }
  }
}
__global__ __launch_bounds__(256) void k_vec_topk_flags(uint64_t keep, uint64_t n, const uint32_t* __restrict__ sidx, uint8_t* __restrict__ tpres) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < keep; i += gridDim.x * 256ull) { const uint32_t p = sidx[i]; if (p < n) tpres[p] = 1; }
}

inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }
inline unsigned blocks_for(uint64_t items, uint64_t per_cu = 8) { uint64_t b = items, cap = (uint64_t)device_cus() * per_cu; if (cap < 1) cap = 1; if (b > cap) b = cap; if (b < 1) b = 1; return (unsigned)b; }

// GRB_MI355X_SORT_EDGES="W,L": the two bin edges of this call instead of the chosen ones (read per call: the hook tools/sort_probe.py finds the edges with).
// Clamped to what the kernels hold: W <= SORT_WAVE_MAX lanes, W <= L <= SORT_LDS_MAX elements of LDS.
void sort_edges_env(uint32_t* wave_edge, uint32_t* lds_edge) {
  const char* e = getenv("GRB_MI355X_SORT_EDGES");
  unsigned w = 0, l = 0;
  if (!e || sscanf(e, "%u,%u", &w, &l) != 2) return;
  if (w > SORT_WAVE_MAX) w = (unsigned)SORT_WAVE_MAX;
  if (l > SORT_LDS_MAX) l = (unsigned)SORT_LDS_MAX;
  if (l < w) l = w;
  *wave_edge = w; *lds_edge = l;
}

template <class K> void segmented_sort(const K* kin, K* kout, const uint32_t* vin, uint32_t* vout, uint64_t n, uint32_t nseg, const uint32_t* begins, const uint32_t* ends) {
  if constexpr (sizeof(K) == 8) segmented_sort_pairs_u64(kin, kout, vin, vout, n, nseg, begins, ends, 64);
  else segmented_sort_pairs_u32(kin, kout, vin, vout, n, nseg, begins, ends, 32);
}

}  // namespace

void csr_sort_positions(const DevCSR& R, int kcode, const void* kval, bool gt, bool prim_only, DevBuf& perm, DevBuf& ocol, SortPlan& plan) {
  const uint32_t nrows = R.nrows; const uint64_t nnz = R.nnz;
  if (nnz > GRB_DIM_DEVICE_MAX) fail(GrB_PANIC, "sort: the matrix does not fit the 32-bit device layout");
  plan = SortPlan(); plan.key_bits = sort_key_is_64(kcode) ? 64 : 32;
  perm.alloc(nnz * 4 + 16); ocol.alloc(nnz * 4 + 16);
  const uint32_t* rp = R.rowptr.as<uint32_t>();
  uint32_t* pm = perm.as<uint32_t>(); uint32_t* oc = ocol.as<uint32_t>();
  const int g = gt ? 1 : 0;
  uint32_t wave_edge = (uint32_t)SORT_WAVE_EDGE, lds_edge = (uint32_t)SORT_LDS_EDGE;
  sort_edges_env(&wave_edge, &lds_edge);
  if (!nnz || !nrows) { plan.wave = prim_only ? 0 : nrows; plan.prim = prim_only ? nrows : 0; return; }
  const bool known = dispatch_type(kcode, [&]<class T>() {
    typedef typename SortKeyOf<T>::type K;
    const T* kv = (const T*)kval;
    if (prim_only) {
      DevBuf kin(nnz * sizeof(K)), kout(nnz * sizeof(K)), vin(nnz * 4);
      hipLaunchKernelGGL((k_sort_keys_all<T>), dim3(grid_1d(nnz)), dim3(256), 0, stream(), nnz, kv, g, kin.as<K>(), vin.as<uint32_t>());
      segmented_sort<K>(kin.as<K>(), kout.as<K>(), vin.as<uint32_t>(), pm, nnz, nrows, rp, rp + 1);
      hipLaunchKernelGGL(k_sort_rowcols, dim3(row_launch_blocks(nrows)), dim3(256), 0, stream(), nrows, rp, oc);
      GRB_HIP(hipGetLastError());
      GRB_HIP(hipStreamSynchronize(stream()));                                      // (the temporaries return to the pool)
      plan.prim = nrows; plan.kernels = "k_sort_keys_all segmented_radix_sort k_sort_rowcols ";
      return;
    }
    // the bins: a row of the LDS bin holds > 64 entries, one of the long bin > SORT_LDS_MAX
    const uint32_t cap_lds = (uint32_t)std::min<uint64_t>(nrows, nnz / ((uint64_t)wave_edge + 1) + 1), cap_long = (uint32_t)std::min<uint64_t>(nrows, nnz / ((uint64_t)lds_edge + 1) + 1);
    DevBuf cnt(16), lds_rows((size_t)cap_lds * 4), long_rows((size_t)cap_long * 4), long_begin((size_t)cap_long * 4), long_end((size_t)cap_long * 4);
    GRB_HIP(hipMemsetAsync(cnt.p, 0, 16, stream()));
    hipLaunchKernelGGL(k_sort_bins, dim3(grid_1d(nrows)), dim3(256), 0, stream(), nrows, rp, wave_edge, lds_edge, cnt.as<uint32_t>(), lds_rows.as<uint32_t>(), cap_lds,
                       long_rows.as<uint32_t>(), long_begin.as<uint32_t>(), long_end.as<uint32_t>(), cap_long);
    // the short rows do not wait for the counts
    hipLaunchKernelGGL((k_sort_wave<T>), dim3(row_launch_blocks(((uint64_t)nrows + 3) / 4)), dim3(256), 0, stream(), nrows, rp, kv, g, wave_edge, pm, oc);
    GRB_HIP(hipGetLastError());
    uint32_t* h = (uint32_t*)pinned_scratch();
    GRB_HIP(hipMemcpyAsync(h, cnt.p, 16, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
    const uint32_t nlds = h[0], nlong = h[1], total = h[2];
    if (nlds > cap_lds || nlong > cap_long || total > nnz) fail(GrB_PANIC, "sort: the row bins do not match the row pointer");
    plan.lds = nlds; plan.prim = nlong; plan.wave = (uint64_t)nrows - nlds - nlong;
    plan.kernels = "k_sort_bins k_sort_wave ";
    if (nlds) {
      if (lds_edge <= SORT_LDS_WAVE_MAX) hipLaunchKernelGGL((k_sort_lds<T, (int)SORT_LDS_WAVE_MAX, 64>), dim3(blocks_for(nlds, 64)), dim3(64), 0, stream(), lds_rows.as<uint32_t>(), nlds, rp, kv, g, pm, oc);
      else hipLaunchKernelGGL((k_sort_lds<T, (int)SORT_LDS_MAX, 256>), dim3(blocks_for(nlds)), dim3(256), 0, stream(), lds_rows.as<uint32_t>(), nlds, rp, kv, g, pm, oc);
      plan.kernels += "k_sort_lds ";
    }
    if (nlong) {
      DevBuf kin((size_t)total * sizeof(K)), kout((size_t)total * sizeof(K)), vin((size_t)total * 4), vout((size_t)total * 4);
      hipLaunchKernelGGL((k_sort_long_keys<T>), dim3(blocks_for(nlong)), dim3(256), 0, stream(), nlong, long_rows.as<uint32_t>(), long_begin.as<uint32_t>(), rp, kv, g, total, kin.as<K>(), vin.as<uint32_t>());
      segmented_sort<K>(kin.as<K>(), kout.as<K>(), vin.as<uint32_t>(), vout.as<uint32_t>(), total, nlong, long_begin.as<uint32_t>(), long_end.as<uint32_t>());
      hipLaunchKernelGGL(k_sort_long_finish, dim3(blocks_for(nlong)), dim3(256), 0, stream(), nlong, long_rows.as<uint32_t>(), long_begin.as<uint32_t>(), rp, total, vout.as<uint32_t>(), pm, oc);
      GRB_HIP(hipGetLastError());
      GRB_HIP(hipStreamSynchronize(stream()));                                      // (the temporaries return to the pool)
      plan.kernels += "k_sort_long_keys segmented_radix_sort k_sort_long_finish ";
    }
    GRB_HIP(hipGetLastError());
    GRB_HIP(hipStreamSynchronize(stream()));                                        // (the lists return to the pool)
  });
  if (!known) fail(GrB_DOMAIN_MISMATCH, "sort: values of this type have no order");
}

void csr_sort_fill(const DevCSR& R, size_t ts, const DevBuf& perm, const DevBuf& ocol, DevCSR* T, DevCSR* Tp) {
  check_value_size(ts, "sort");
  const uint64_t nnz = R.nnz; const size_t rpb = ((size_t)R.nrows + 1) * 4;
  for (DevCSR* out : {T, Tp}) {
    if (!out) continue;
    out->clear(); out->nrows = R.nrows; out->ncols = R.ncols; out->nnz = nnz;
    out->rowptr.alloc(rpb); out->col.alloc(nnz * 4 + 16); out->val.alloc(nnz * (out == Tp ? 8 : ts) + 32);
    GRB_HIP(hipMemcpyAsync(out->rowptr.p, R.rowptr.p, rpb, hipMemcpyDeviceToDevice, stream()));
    if (nnz) GRB_HIP(hipMemcpyAsync(out->col.p, ocol.p, nnz * 4, hipMemcpyDeviceToDevice, stream()));
    out->valid = true;
  }
  if (!nnz) return;
  const size_t pa = ts * SORT_EPL > 16 ? 16 : ts * SORT_EPL;
  const int packed = aligned_to(perm.p, 16) && (!T || aligned_to(T->val.p, pa)) && (!Tp || aligned_to(Tp->val.p, 16)) ? 1 : 0;
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_sort_gather<TS>), dim3(grid_1d((nnz + SORT_EPL - 1) / SORT_EPL)), dim3(256), 0, stream(), nnz, perm.as<uint32_t>(), R.val.as<uint8_t>(), R.col.as<uint32_t>(),
                       T ? T->val.as<uint8_t>() : nullptr, Tp ? Tp->val.as<int64_t>() : nullptr, packed);
  });
  GRB_HIP(hipGetLastError());
}

void topk_flags(uint64_t nnz, const DevBuf& perm, const DevBuf& ocol, uint64_t k, uint8_t* keep) {
  if (!nnz) return;
  hipLaunchKernelGGL(k_topk_flags, dim3(grid_1d(nnz)), dim3(256), 0, stream(), nnz, perm.as<uint32_t>(), ocol.as<uint32_t>(), k, keep);
  GRB_HIP(hipGetLastError());
}

uint64_t vec_sort_positions(int kcode, const void* kval, const uint8_t* pres, uint64_t n, bool gt, DevBuf& sidx, SortPlan& plan) {
  if (n > GRB_DIM_DEVICE_MAX) fail(GrB_PANIC, "sort: the vector does not fit the 32-bit device layout");
  plan = SortPlan(); plan.key_bits = sort_key_is_64(kcode) ? 64 : 32;
  sidx.alloc(n * 4 + 16);
  if (!n) return 0;
  DevBuf pos((n + 1) * 4 + 4), idx(n * 4 + 16);
  const uint64_t nvals = present_positions_total(pres, n, pos.as<uint32_t>());       // the one read-back
  if (nvals > n) fail(GrB_PANIC, "sort: the presence scan does not match the vector");
  plan.kernels = "present_positions ";
  if (nvals) {
    scatter_present(pres, pos.as<uint32_t>(), n, 0, COMPACT_COL_INDEX, n, idx.as<uint32_t>(), 0, nullptr, nullptr);
    const bool known = dispatch_type(kcode, [&]<class T>() {
      typedef typename SortKeyOf<T>::type K;
      DevBuf keys(nvals * sizeof(K)), keys_out(nvals * sizeof(K));
      hipLaunchKernelGGL((k_vec_sort_keys<T>), dim3(grid_1d(nvals)), dim3(256), 0, stream(), nvals, n, idx.as<uint32_t>(), (const T*)kval, gt ? 1 : 0, keys.as<K>());
      if constexpr (sizeof(K) == 8) sort_pairs_u64(keys.as<K>(), keys_out.as<K>(), idx.as<uint32_t>(), sidx.as<uint32_t>(), nvals, 64);
      else sort_pairs_u32(keys.as<K>(), keys_out.as<K>(), idx.as<uint32_t>(), sidx.as<uint32_t>(), nvals, 32);
      GRB_HIP(hipGetLastError());
      GRB_HIP(hipStreamSynchronize(stream()));                                      // (the keys return to the pool)
    });
    if (!known) fail(GrB_DOMAIN_MISMATCH, "sort: values of this type have no order");
    plan.kernels += "scatter_present k_vec_sort_keys radix_sort_pairs ";
  }
  GRB_HIP(hipStreamSynchronize(stream()));
  return nvals;
}

void vec_sort_fill(size_t ts, const void* uval, const DevBuf& sidx, uint64_t nvals, uint64_t n, void* tval, uint8_t* tpres, void* pval, uint8_t* ppres) {
  check_value_size(ts, "sort");
  if (!n) return;
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_vec_sort_fill<TS>), dim3(grid_1d(n)), dim3(256), 0, stream(), n, nvals, sidx.as<uint32_t>(), (const uint8_t*)uval, (uint8_t*)tval, tpres, (int64_t*)pval, ppres);
  });
  GRB_HIP(hipGetLastError());
}

void vec_topk_flags(const DevBuf& sidx, uint64_t keep, uint64_t n, uint8_t* tpres) {
  if (!n) return;
  GRB_HIP(hipMemsetAsync(tpres, 0, n, stream()));
  if (keep) hipLaunchKernelGGL(k_vec_topk_flags, dim3(grid_1d(keep)), dim3(256), 0, stream(), keep, n, sidx.as<uint32_t>(), tpres);
  GRB_HIP(hipGetLastError());
}

}  // namespace grb
