// grb_gemm_kernels.hpp — the value kernel of the product of two full matrices (grb_gemm.hpp), instantiated per value type in grb_gemm_inst.hip.
//
//   k_gemm_full<T, SR, TM, TN>   a workgroup of GEMM_WAVES waves computes a TM x TN tile of T (tiles grid-strided, row-major), thread (ty, tx) the GEMM_RM x GEMM_RN
//             register block at rows 4 ty, columns 4 tx of the tile.  k is walked in steps of GEMM_KT: a step stages the tile's TM x KT piece of op(A) and KT x TN
//             piece of op(B) in LDS as As[l][i] and Bs[l][j] — a thread's four i and four j are one contiguous LDS read each, the lanes of a wave that share ty or
//             tx read the same words — and folds the step's products from LDS into the 16 accumulators.  The loader reads the operand where it lies: consecutive
//             threads take consecutive addresses of the stored array, whichever of l or i / j that is (two run-time flags, one code path each); as [l][i] a row of
//             LDS is TM + GEMM_PAD elements, so the transposing store of consecutive l falls into different banks.
// Fold order: T(i, j) = the left-to-right fold of mult(op(A)(i, l), op(B)(l, j)) in ascending l, starting from the product l = 0 — never from an identity, so ANY
// and a monoid without a representable identity are right.  The last, ragged step folds the products that exist and nothing else; rows and columns of a tile
// beyond m or n are not loaded (their LDS words hold T()) and not stored.  A side the multiplier ignores is not staged and not read (sr.uses_a / sr.uses_u: PAIR
// neither, FIRST no B value, SECOND no A value).  No atomics, no scratch, every output word has one writer.
#pragma once
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_semiring.hpp"
#include "grb_gemm.hpp"

namespace grb {

template <class T> struct GemmKArgs {
  const T* aval; const T* bval;                         // the operands as stored; nullptr: not read
  T* tval;                                              // m x n row-major
  uint32_t m, n, k; bool ta, tb;                        // ta: A is stored k x m; tb: B is stored n x k
  uint64_t ntiles;
};

// dst[l][r] = the operand's value at row / column r0 + r of the tile's side and product l0 + l, for r < R and l < len; T() where r0 + r >= ext (nothing is loaded).
// along_l: the products of one r are contiguous in memory, src[(r0 + r) k + l0 + l]; otherwise the r of one product are, src[(l0 + l) ext + r0 + r].
template <class T, int R>
__device__ __forceinline__ void gemm_stage(T (*dst)[R + GEMM_PAD], const T* __restrict__ src, bool along_l, uint64_t r0, uint32_t ext, uint32_t l0, uint32_t len, uint32_t k) {
  if (along_l) {
    for (uint32_t e = threadIdx.x; e < (uint32_t)R * GEMM_KT; e += GEMM_WAVES * 64) {
      const uint32_t l = e % GEMM_KT, r = e / GEMM_KT;
      if (l < len) dst[l][r] = r0 + r < ext ? src[(r0 + r) * k + l0 + l] : T();
    }
  } else {
    for (uint32_t e = threadIdx.x; e < (uint32_t)R * GEMM_KT; e += GEMM_WAVES * 64) {
      const uint32_t r = e % (uint32_t)R, l = e / (uint32_t)R;
      if (l < len) dst[l][r] = r0 + r < ext ? src[(uint64_t)(l0 + l) * ext + r0 + r] : T();
    }
  }
}

template <class T, class SR, int TM, int TN>
__global__ __launch_bounds__(GEMM_WAVES * 64) void k_gemm_full(SR sr, GemmKArgs<T> a) {
  static_assert(TM * TN == (int)(GEMM_WAVES * 64 * GEMM_RM * GEMM_RN) && TM % GEMM_RM == 0 && TN % GEMM_RN == 0, "one register block per thread");
  __shared__ __attribute__((aligned(16))) T As[GEMM_KT][TM + GEMM_PAD];
  __shared__ __attribute__((aligned(16))) T Bs[GEMM_KT][TN + GEMM_PAD];
  const bool ua = sr.uses_a(), ub = sr.uses_u();
  constexpr uint32_t TX = TN / GEMM_RN;
  const uint32_t ri = threadIdx.x / TX * GEMM_RM, cj = threadIdx.x % TX * GEMM_RN;      // the thread's block inside the tile
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const uint64_t i0 = gemm_tile_i0(t, a.n), j0 = gemm_tile_j0(t, a.n);
    T acc[GEMM_RM][GEMM_RN];
    auto fold = [&](uint32_t l, bool first) {
      T av[GEMM_RM], bv[GEMM_RN];
#pragma unroll
      for (uint32_t r = 0; r < GEMM_RM; r++) av[r] = ua ? As[l][ri + r] : T();
#pragma unroll
      for (uint32_t c = 0; c < GEMM_RN; c++) bv[c] = ub ? Bs[l][cj + c] : T();
#pragma unroll
      for (uint32_t r = 0; r < GEMM_RM; r++)
#pragma unroll
        for (uint32_t c = 0; c < GEMM_RN; c++) acc[r][c] = first ? sr.mult(av[r], bv[c]) : sr.add(acc[r][c], sr.mult(av[r], bv[c]));
    };
    for (uint32_t l0 = 0; l0 < a.k; l0 += GEMM_KT) {                 // (k <= 2^32 - 17: l0 + KT does not wrap)
      const uint32_t len = gemm_step_len(a.k, l0 / GEMM_KT);
      __syncthreads();                                               // the folds of the step (or tile) before have read their LDS
      if (ua) gemm_stage<T, TM>(As, a.aval, !a.ta, i0, a.m, l0, len, a.k);
      if (ub) gemm_stage<T, TN>(Bs, a.bval, a.tb, j0, a.n, l0, len, a.k);
      __syncthreads();
      if (l0 == 0) {
        fold(0, true);
        for (uint32_t l = 1; l < len; l++) fold(l, false);
      } else if (SR::is_static && len == GEMM_KT) {
#pragma unroll
        for (uint32_t l = 0; l < GEMM_KT; l++) fold(l, false);
      } else {
        for (uint32_t l = 0; l < len; l++) fold(l, false);
      }
    }
#pragma unroll
    for (uint32_t r = 0; r < GEMM_RM; r++) {
      const uint64_t i = i0 + ri + r;
      if (i >= a.m) continue;
#pragma unroll
      for (uint32_t c = 0; c < GEMM_RN; c++) { const uint64_t j = j0 + cj + c; if (j < a.n) a.tval[i * a.n + j] = acc[r][c]; }
    }
  }
}

template <class T> void run_gemm_values(const GemmValuesCall& c, const SemiringDesc& d) {
  with_semiring<T>(d, [&](auto sr) {
    using SR = decltype(sr);
    GemmKArgs<T> a{};
    a.aval = (const T*)c.aval; a.bval = (const T*)c.bval; a.tval = (T*)c.tval; a.m = c.m; a.n = c.n; a.k = c.k; a.ta = c.ta; a.tb = c.tb;
    a.ntiles = gemm_tiles(c.m, c.n);
    const dim3 grid(gemm_grid(c.m, c.n)), block(GEMM_WAVES * 64);
    if (gemm_tall(c.n)) hipLaunchKernelGGL((k_gemm_full<T, SR, (int)GEMM_TM_TALL, (int)GEMM_TN_TALL>), grid, block, 0, stream(), sr, a);
    else hipLaunchKernelGGL((k_gemm_full<T, SR, (int)GEMM_TM_WIDE, (int)GEMM_TN_WIDE>), grid, block, 0, stream(), sr, a);
    GRB_HIP(hipGetLastError());
  });
}

}  // namespace grb
