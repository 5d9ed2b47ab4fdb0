// grb_spmm_kernels.hpp — the value kernels of the product with a full right operand (grb_spmm.hpp), instantiated per value type in grb_spmm_inst.hip.
//
// A PIECE is a run of at most SPMM_L consecutive entries of one row of A.  In the row pass (task == nullptr) piece t is row t, skipped when the row is empty or
// long, and its sums are written into T's values; in the chunk pass piece t is scratch slot t, whose row is task[t] (~0: the slot is unused) and whose chunk
// number follows from the slot's closed form (grb_spmm_geom.hpp), and its sums go to part[t k ..].  k_spmm_fold then folds a long row's chunks in ascending order.
//   k_spmm_narrow   k <= 64: a group of G = 2^gshift lanes owns a piece, lane j of the group column j.  Every entry A(i, l) pulls row l of B as ONE contiguous read
//                   of k values; the lanes of a group load the same col / aval word (one request).
//   k_spmm_wide     k > 64: a wave owns a piece times a slab of SPMM_SLAB columns; lane t holds the slab's columns t, t + 64, ...: four coalesced 64-value reads
//                   per entry.
// The accumulator starts from the piece's FIRST product — never from an identity, so ANY and a monoid without a representable identity are right — and folds
// the others left to right; the entry loop is unrolled by SPMM_UNROLL with all loads in front of the folds.  A side the multiplier ignores is never loaded
// (sr.uses_a / sr.uses_u: PAIR neither, FIRST no B value, SECOND no A value).  No LDS, no atomics, every output word has one writer.
#pragma once
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_semiring.hpp"
#include "grb_spmm.hpp"
#include "grb_index.hpp"

namespace grb {

constexpr int SPMM_UNROLL = 4;                          // entries of A whose loads are issued together
constexpr int SPMM_WIDE_COLS = SPMM_SLAB / 64;          // columns one lane of the wide kernel holds

template <class T> struct SpmmKArgs {
  const uint32_t* arp; const uint32_t* acol; const T* aval;     // A; aval nullptr: not read
  const T* bval;                                                // B's values, row-major n x k; nullptr: not read
  uint32_t k, gshift, nslabs;
  uint64_t npieces;                                             // rows of A (row pass) or scratch slots (chunk pass)
  const uint32_t* trp; T* tval;                                 // row pass: T's row pointer and values
  const uint32_t* task; const uint32_t* lrank; T* part;         // chunk pass: the slot's row, every row's rank among the long rows, the partial sums
};

// the entries [ps, pe) of piece t and where its k sums go; false: nothing to do
template <class T> __device__ __forceinline__ bool spmm_piece(const SpmmKArgs<T>& a, uint64_t t, uint32_t& ps, uint32_t& pe, T*& dst) {
  if (!a.task) {
    const uint32_t rs = a.arp[t], re = a.arp[t + 1], len = re - rs;
    if (len == 0 || spmm_long(len)) return false;
    ps = rs; pe = re; dst = a.tval + a.trp[t];
  } else {
    const uint32_t i = a.task[t];
    if (i == 0xFFFFFFFFu) return false;
    const uint32_t rs = a.arp[i], re = a.arp[i + 1], c = (uint32_t)t - spmm_slot_base(rs, a.lrank[i]);
    ps = spmm_chunk_begin(rs, c); pe = spmm_chunk_end(rs, re, c); dst = a.part + t * a.k;
  }
  return true;
}

// acc[u] = the left-to-right fold over the entries [ps, pe) (ps < pe) of mult(A(i, l), B(l, c0 + 64 u)) for the columns the lane holds (on[u])
template <class T, class SR, int NC>
__device__ __forceinline__ void spmm_fold_piece(const SR& sr, const SpmmKArgs<T>& a, uint32_t ps, uint32_t pe, uint32_t c0, const bool (&on)[NC], T (&acc)[NC]) {
  const bool ua = sr.uses_a(), ub = sr.uses_u();
  {
    const T av = ua ? a.aval[ps] : T();
    const uint64_t brow = ub ? (uint64_t)a.acol[ps] * a.k : 0;
#pragma unroll
    for (int u = 0; u < NC; u++) acc[u] = sr.mult(av, (ub && on[u]) ? a.bval[brow + c0 + 64u * u] : T());
  }
  uint32_t p = ps + 1;
  for (; p + SPMM_UNROLL <= pe; p += SPMM_UNROLL) {
    T av[SPMM_UNROLL], bv[SPMM_UNROLL][NC]; uint64_t brow[SPMM_UNROLL];
#pragma unroll
    for (int e = 0; e < SPMM_UNROLL; e++) { av[e] = ua ? a.aval[p + e] : T(); brow[e] = ub ? (uint64_t)a.acol[p + e] * a.k : 0; }
#pragma unroll
    for (int e = 0; e < SPMM_UNROLL; e++)
#pragma unroll
      for (int u = 0; u < NC; u++) bv[e][u] = (ub && on[u]) ? a.bval[brow[e] + c0 + 64u * u] : T();
#pragma unroll
    for (int e = 0; e < SPMM_UNROLL; e++)
#pragma unroll
      for (int u = 0; u < NC; u++) acc[u] = sr.add(acc[u], sr.mult(av[e], bv[e][u]));
  }
  for (; p < pe; p++) {
    const T av = ua ? a.aval[p] : T();
    const uint64_t brow = ub ? (uint64_t)a.acol[p] * a.k : 0;
#pragma unroll
    for (int u = 0; u < NC; u++) acc[u] = sr.add(acc[u], sr.mult(av, (ub && on[u]) ? a.bval[brow + c0 + 64u * u] : T()));
  }
}

template <class T, class SR>
__global__ __launch_bounds__(SPMM_WAVES * 64) void k_spmm_narrow(SR sr, SpmmKArgs<T> a) {
  const uint32_t j = threadIdx.x & ((1u << a.gshift) - 1u);
  const uint64_t per_wg = (SPMM_WAVES * 64u) >> a.gshift;
  for (uint64_t t = blockIdx.x * per_wg + (threadIdx.x >> a.gshift); t < a.npieces; t += gridDim.x * per_wg) {
    uint32_t ps, pe; T* dst;
    if (j >= a.k || !spmm_piece(a, t, ps, pe, dst)) continue;
    const bool on[1] = {true}; T acc[1];
    spmm_fold_piece<T, SR, 1>(sr, a, ps, pe, j, on, acc);
    dst[j] = acc[0];
  }
}

template <class T, class SR>
__global__ __launch_bounds__(SPMM_WAVES * 64) void k_spmm_wide(SR sr, SpmmKArgs<T> a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwork = a.npieces * a.nslabs;
  for (uint64_t w = (uint64_t)blockIdx.x * SPMM_WAVES + (threadIdx.x >> 6); w < nwork; w += (uint64_t)gridDim.x * SPMM_WAVES) {
    const uint64_t t = w / a.nslabs; const uint32_t slab = (uint32_t)(w % a.nslabs);
    uint32_t ps, pe; T* dst;
    if (!spmm_piece(a, t, ps, pe, dst)) continue;
    const uint32_t c0 = slab * SPMM_SLAB + lane;
    bool on[SPMM_WIDE_COLS]; T acc[SPMM_WIDE_COLS];
#pragma unroll
    for (int u = 0; u < SPMM_WIDE_COLS; u++) on[u] = c0 + 64u * u < a.k;
    spmm_fold_piece<T, SR, SPMM_WIDE_COLS>(sr, a, ps, pe, c0, on, acc);
#pragma unroll
    for (int u = 0; u < SPMM_WIDE_COLS; u++) if (on[u]) dst[c0 + 64u * u] = acc[u];
  }
}

// T(i, j) of long row number q = the fold of its chunks' partial sums in ascending chunk order; one thread per (q, j), consecutive threads consecutive columns
template <class T, class SR>
__global__ __launch_bounds__(256) void k_spmm_fold(SR sr, SpmmKArgs<T> a, const uint32_t* __restrict__ lrow, uint64_t nlong) {
  const uint64_t total = nlong * a.k;
  for (uint64_t x = blockIdx.x * 256ull + threadIdx.x; x < total; x += gridDim.x * 256ull) {
    const uint32_t q = (uint32_t)(x / a.k), j = (uint32_t)(x % a.k), i = lrow[q];
    const uint32_t rs = a.arp[i], nch = spmm_chunks(a.arp[i + 1] - rs);
    const T* src = a.part + (uint64_t)spmm_slot_base(rs, q) * a.k + j;
    T acc = src[0];
    for (uint32_t c = 1; c < nch; c++) acc = sr.add(acc, src[(uint64_t)c * a.k]);
    a.tval[(uint64_t)a.trp[i] + j] = acc;
  }
}

template <class T> void run_spmm_values(const SpmmValuesCall& c, const SemiringDesc& d) {
  with_semiring<T>(d, [&](auto sr) {
    using SR = decltype(sr);
    SpmmKArgs<T> a{};
    a.arp = c.A->rowptr.as<uint32_t>(); a.acol = c.A->col.as<uint32_t>(); a.aval = (const T*)c.aval; a.bval = (const T*)c.bval;
    a.k = c.k; a.nslabs = spmm_slabs(c.k); a.trp = c.trp; a.tval = (T*)c.tval; a.lrank = c.lrank; a.part = (T*)c.part;
    const bool narrow = spmm_narrow(c.k);
    if (narrow) { const uint32_t g = spmm_group(c.k); a.gshift = 0; while ((1u << a.gshift) < g) a.gshift++; }
    auto launch = [&](uint64_t npieces, const uint32_t* task) {
      a.npieces = npieces; a.task = task;
      if (narrow) hipLaunchKernelGGL((k_spmm_narrow<T, SR>), dim3(spmm_grid(npieces, spmm_pieces_per_workgroup(c.k))), dim3(SPMM_WAVES * 64), 0, stream(), sr, a);
      else hipLaunchKernelGGL((k_spmm_wide<T, SR>), dim3(spmm_grid(npieces * a.nslabs, SPMM_WAVES)), dim3(SPMM_WAVES * 64), 0, stream(), sr, a);
    };
    launch(c.A->nrows, nullptr);
    if (c.nlong) {
      launch(c.nslots, c.task);
      a.task = c.task;
      hipLaunchKernelGGL((k_spmm_fold<T, SR>), dim3(grid_1d(c.nlong * c.k, SPMM_GRID_CAP)), dim3(256), 0, stream(), sr, a, c.lrow, c.nlong);
    }
    GRB_HIP(hipGetLastError());
  });
}

}  // namespace grb
