// grb_sddmm_kernels.hpp — the value kernel of the masked product of two full matrices (grb_sddmm.hpp), instantiated per value type in grb_sddmm_inst.hip.
//
//   k_sddmm   T(i, j) = (+)_l X(i, l) (x) Y(j, l) for every entry of the mask's pattern.  The work is cut by ENTRIES: a workgroup takes tiles of SDDMM_TILE
//             consecutive entries (grid-strided), bisects the row pointer for the rows of the tile's first and last entry — every lane the same reads: one
//             request — and each group of G = 2^gshift lanes then finds its entry's row between those two (no step while the tile lies inside one row: a hub row
//             costs nothing, and neither do empty rows, which no entry points into).  Lane g of the group loads X(i, l) and Y(j, l) for l = g, g + G, ...: the
//             group's loads are two contiguous runs.
// Fold order (a function of k alone): lane g folds its products left to right in ascending l starting from its FIRST product — never from an identity, so ANY and a
// monoid without a representable identity are right — with the loads of SDDMM_UNROLL steps issued in front of their folds; then the butterfly
// p_g = p_g (+) p_{g + s}, s = G / 2 ... 1, where lane g + s holds a partial (g + s < min(k, G)).  Every lane of the wave runs the shuffles; lanes without an
// entry or without a product load nothing and combine nothing.  A side the multiplier ignores is never loaded (sr.uses_a / sr.uses_u: PAIR neither, FIRST no Y
// value, SECOND no X value).  No LDS, no atomics, every output word has one writer (the group's lane 0).
#pragma once
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_semiring.hpp"
#include "grb_sddmm.hpp"
#include "grb_index.hpp"

namespace grb {

constexpr int SDDMM_UNROLL = 4;                         // steps of a lane's fold whose loads are issued together

template <class T> struct SddmmKArgs {
  const uint32_t* mrp; const uint32_t* mcol;            // the mask's pattern, m rows, `entries` entries in `ntiles` tiles
  const T* xval; const T* yval;                         // row-major m x k / n x k; nullptr: not read
  T* tval;                                              // one value per mask entry
  uint32_t m, k, gshift; uint64_t entries, ntiles;
};

// lane g's partial: the left-to-right fold of mult(x[l], y[l]) over l = g, g + G, ... < k (g < k)
template <class T, class SR>
__device__ __forceinline__ T sddmm_lane_fold(const SR& sr, const T* __restrict__ x, const T* __restrict__ y, uint32_t g, uint32_t G, uint32_t k) {
  const bool ua = sr.uses_a(), ub = sr.uses_u();
  uint64_t l = g;
  T acc = sr.mult(ua ? x[l] : T(), ub ? y[l] : T());
  l += G;
  for (; l + (uint64_t)(SDDMM_UNROLL - 1) * G < k; l += (uint64_t)SDDMM_UNROLL * G) {
    T xv[SDDMM_UNROLL], yv[SDDMM_UNROLL];
#pragma unroll
    for (int u = 0; u < SDDMM_UNROLL; u++) { xv[u] = ua ? x[l + (uint64_t)u * G] : T(); yv[u] = ub ? y[l + (uint64_t)u * G] : T(); }
#pragma unroll
    for (int u = 0; u < SDDMM_UNROLL; u++) acc = sr.add(acc, sr.mult(xv[u], yv[u]));
  }
  for (; l < k; l += G) acc = sr.add(acc, sr.mult(ua ? x[l] : T(), ub ? y[l] : T()));
  return acc;
}

template <class T, class SR>
__global__ __launch_bounds__(SDDMM_WAVES * 64) void k_sddmm(SR sr, SddmmKArgs<T> a) {
  const uint32_t G = 1u << a.gshift, g = threadIdx.x & (G - 1u), slot = threadIdx.x >> a.gshift, per_pass = (SDDMM_WAVES * 64u) >> a.gshift;
  const uint32_t live = a.k < G ? a.k : G;
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const uint64_t t0 = sddmm_tile_begin(t), t1 = sddmm_tile_end(t, a.entries);
    const uint32_t rlo = sddmm_row_of(a.mrp, 0u, a.m - 1u, t0), rhi = sddmm_row_of(a.mrp, rlo, a.m - 1u, t1 - 1);
    for (uint64_t e0 = t0; e0 < t1; e0 += per_pass) {              // (the same trip count in every lane of the workgroup: all lanes reach the shuffles)
      const uint64_t e = e0 + slot;
      const bool on = e < t1 && g < live;
      T p = T();
      if (on) {
        const uint32_t i = sddmm_row_of(a.mrp, rlo, rhi, e), j = a.mcol[e];
        p = sddmm_lane_fold<T, SR>(sr, a.xval + (uint64_t)i * a.k, a.yval + (uint64_t)j * a.k, g, G, a.k);
      }
      for (uint32_t s = G >> 1; s; s >>= 1) {
        const T q = shfl_down_t<T>(p, (int)s);
        if (on && g + s < live) p = sr.add(p, q);
      }
      if (on && g == 0) a.tval[e] = p;
    }
  }
}

template <class T> void run_sddmm_values(const SddmmValuesCall& c, const SemiringDesc& d) {
  with_semiring<T>(d, [&](auto sr) {
    using SR = decltype(sr);
    SddmmKArgs<T> a{};
    a.mrp = c.mrp; a.mcol = c.mcol; a.xval = (const T*)c.xval; a.yval = (const T*)c.yval; a.tval = (T*)c.tval;
    a.m = c.m; a.k = c.k; a.gshift = sddmm_gshift(c.k); a.entries = c.entries; a.ntiles = sddmm_tiles(c.entries);
    hipLaunchKernelGGL((k_sddmm<T, SR>), dim3(sddmm_grid(c.entries)), dim3(SDDMM_WAVES * 64), 0, stream(), sr, a);
    GRB_HIP(hipGetLastError());
  });
}

}  // namespace grb
