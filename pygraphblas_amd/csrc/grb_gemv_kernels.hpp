// grb_gemv_kernels.hpp — the kernels of a full matrix times a vector (grb_gemv.hpp), instantiated per value type in grb_gemv_inst.hip.  t(o) = (+)_l M(o, l) (x) u(l),
// m outputs, k products each (those whose u(l) is absent do not exist); A's value array is read where it lies.
//
//   k_gemv_n_short   layout N, k <= GEMV_N_GROUP_MAX: a group of G lanes per row, lane g the product l = g; consecutive rows are consecutive memory, so a wave's
//                    load is one contiguous run.  The group's butterfly p_g = p_g (+) p_(g + s), s = G / 2 ... 1, takes only lanes that hold a product.
//   k_gemv_n_wave    layout N, longer rows: a wave per (row, chunk) unit.  Lane g folds the packets g, g + 64, ... of the chunk left to right (a packet: V
//                    consecutive products, one load of A — 16 bytes for 4- and 8-byte values — where the address allows, GEMV_N_UNROLL packets in flight), then the same butterfly over 64 lanes.
//   k_gemv_t         layout T: a workgroup per (slab, chunk) unit; wave w walks piece w of the chunk's rows in ascending l, every lane folding its VT columns
//                    (GEMV_T_UNROLL rows in flight).  Whether u(l) exists is the same for every lane: a scalar branch.  The waves' partials meet in LDS and
//                    wave 0 folds them in ascending piece order.
//   k_gemv_fold      an output's chunk partials in ascending chunk order, one thread per output.
// Every accumulator starts from its FIRST existing product — never from an identity — and carries a "has a value" flag through lanes, LDS and scratch slots: ANY
// and monoids without a representable identity are right, and a piece, a chunk or a lane all of whose u(l) are absent contributes nothing.  A side the
// multiplier ignores is not loaded (sr.uses_a / sr.uses_u).  No atomics; every output word and every slot has one writer.
#pragma once
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_semiring.hpp"
#include "grb_gemv.hpp"

namespace grb {

template <class T> struct GemvKArgs {
  const T* aval; const T* uval;                         // A's values as stored / u's values, in the semiring's type; nullptr: not read
  const uint8_t* upres;                                 // u's presence bytes; nullptr: every position holds an entry
  T* tval;                                              // the m results (one chunk per output)
  T* part; uint8_t* flag;                               // otherwise: the scratch slots and their "has a value" bytes
  uint64_t m, k, chunks, slabs;
};

template <class T, int V> struct alignas(V * sizeof(T)) GemvPack { T v[V]; };

// acc = acc (+) p, where either side may hold nothing
template <class T, class SR> __device__ __forceinline__ void gemv_join(const SR& sr, T& acc, bool& has, const T& p, bool phas) {
  if (phas) { acc = has ? sr.add(acc, p) : p; has = true; }
}
// the butterfly over the G lanes of a group (g: the lane's place in it); lane 0 ends up with the group's fold
template <class T, class SR> __device__ __forceinline__ void gemv_butterfly(const SR& sr, T& acc, bool& has, uint32_t g, uint32_t G) {
  for (uint32_t s = G >> 1; s; s >>= 1) {
    const T q = shfl_down_t<T>(acc, (int)s); const bool qh = __shfl_down((int)has, (int)s, 64) != 0;
    if (g + s < G) gemv_join(sr, acc, has, q, qh);
  }
}
// where a unit's result goes: the output itself, or its slot
template <class T> __device__ __forceinline__ void gemv_store(const GemvKArgs<T>& a, int layout, uint64_t o, uint64_t c, const T& acc, bool has) {
  if (a.chunks == 1) { a.tval[o] = acc; return; }
  const uint64_t s = gemv_slot(layout, o, c, a.m, a.chunks);
  a.flag[s] = has ? 1 : 0;
  if (has) a.part[s] = acc;
}

template <class T, class SR>
__global__ __launch_bounds__(GEMV_WAVES * 64) void k_gemv_n_short(SR sr, GemvKArgs<T> a, uint32_t gshift) {
  const uint32_t G = 1u << gshift, g = threadIdx.x & (G - 1u);
  const uint64_t per_wg = (GEMV_WAVES * 64u) >> gshift;
  const bool ua = sr.uses_a(), uu = sr.uses_u();
  for (uint64_t r0 = blockIdx.x * per_wg; r0 < a.m; r0 += gridDim.x * per_wg) {      // (the same trip count in every lane of a wave: all lanes reach the shuffles)
    const uint64_t i = r0 + (threadIdx.x >> gshift);
    bool has = i < a.m && g < a.k && (!a.upres || a.upres[g]);
    T acc = T();
    if (has) acc = sr.mult(ua ? a.aval[i * a.k + g] : T(), uu ? a.uval[g] : T());
    gemv_butterfly(sr, acc, has, g, G);
    if (g == 0 && i < a.m) a.tval[i] = acc;                                          // (u holds an entry: every row has a product)
  }
}

template <class T, class SR>
__global__ __launch_bounds__(GEMV_WAVES * 64) void k_gemv_n_wave(SR sr, GemvKArgs<T> a) {
  constexpr int V = (int)gemv_vec(sizeof(T));
  using Pack = GemvPack<T, V>;
  const uint32_t lane = threadIdx.x & 63u;
  const bool ua = sr.uses_a(), uu = sr.uses_u();
  const uint64_t units = a.m * a.chunks;
  for (uint64_t unit = (uint64_t)blockIdx.x * GEMV_WAVES + (threadIdx.x >> 6); unit < units; unit += (uint64_t)gridDim.x * GEMV_WAVES) {
    const uint64_t i = unit / a.chunks, c = unit % a.chunks;
    const uint64_t l0 = gemv_n_chunk_begin(c), l1 = gemv_n_chunk_end(a.k, c);
    const T* __restrict__ row = a.aval + i * a.k;                                    // (not dereferenced when aval is nullptr)
    const bool aligned = ua && ((uintptr_t)(row + l0) % sizeof(Pack)) == 0;       // the row's address decides HOW a packet is loaded, never which products it holds
    const bool ualigned = uu && ((uintptr_t)a.uval % sizeof(Pack)) == 0;                // (l0 and a packet's offset are whole packets)
    T acc = T(); bool has = false;
    auto fold_packet = [&](const Pack& av, const Pack& uv, uint64_t l, uint32_t n) { // the n <= V products from l on
#pragma unroll
      for (int e = 0; e < V; e++)
        if ((uint32_t)e < n && (!a.upres || a.upres[l + e])) gemv_join(sr, acc, has, sr.mult(av.v[e], uv.v[e]), true);
    };
    auto load = [&](const T* __restrict__ src, bool vec, bool used, uint64_t l, uint32_t n) {
      Pack p;
      if (used && vec && n == (uint32_t)V) p = *reinterpret_cast<const Pack*>(src + l);
      else {
#pragma unroll
        for (int e = 0; e < V; e++) p.v[e] = (used && (uint32_t)e < n) ? src[l + e] : T();
      }
      return p;
    };
    uint64_t l = l0 + (uint64_t)lane * V;
    constexpr uint64_t STEP = 64ull * V;
    for (; l + (GEMV_N_UNROLL - 1) * STEP + V <= l1; l += GEMV_N_UNROLL * STEP) {   // GEMV_N_UNROLL whole packets of this lane
      Pack av[GEMV_N_UNROLL], uv[GEMV_N_UNROLL];
#pragma unroll
      for (uint32_t r = 0; r < GEMV_N_UNROLL; r++) { av[r] = load(row, aligned, ua, l + r * STEP, V); uv[r] = load(a.uval, ualigned, uu, l + r * STEP, V); }
#pragma unroll
      for (uint32_t r = 0; r < GEMV_N_UNROLL; r++) fold_packet(av[r], uv[r], l + r * STEP, V);
    }
    for (; l < l1; l += STEP) {
      const uint32_t n = l1 - l < (uint64_t)V ? (uint32_t)(l1 - l) : (uint32_t)V;
      fold_packet(load(row, aligned, ua, l, n), load(a.uval, ualigned, uu, l, n), l, n);
    }
    gemv_butterfly(sr, acc, has, lane, 64u);
    if (lane == 0) gemv_store(a, GEMV_N, i, c, acc, has);
  }
}

template <class T, class SR, int VT>
__global__ __launch_bounds__(GEMV_WAVES * 64) void k_gemv_t(SR sr, GemvKArgs<T> a) {
  using Pack = GemvPack<T, VT>;
  __shared__ Pack lds_acc[GEMV_WAVES][64];
  __shared__ uint8_t lds_has[GEMV_WAVES];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const bool ua = sr.uses_a(), uu = sr.uses_u();
  const uint64_t units = a.slabs * a.chunks;
  for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const uint64_t c = unit / a.slabs, slab = unit % a.slabs;
    const uint64_t j0 = (slab * 64 + lane) * VT;                                     // the lane's first column; VT > 1 only where VT divides m: a packet is whole
    const bool on = j0 < a.m;
    const uint64_t b = gemv_t_piece_begin(a.k, c, w), e = gemv_t_piece_end(a.k, c, w);
    Pack acc; bool has = false;                                                      // `has` is the same in every lane: u(l) exists or not for the whole row
#pragma unroll
    for (int v = 0; v < VT; v++) acc.v[v] = T();
    auto fold_row = [&](const Pack& av, uint64_t l) {
      if (a.upres && !a.upres[l]) return;
      const T uv = uu ? a.uval[l] : T();
#pragma unroll
      for (int v = 0; v < VT; v++) { const T p = sr.mult(av.v[v], uv); acc.v[v] = has ? sr.add(acc.v[v], p) : p; }
      has = true;
    };
    auto load = [&](uint64_t l) {
      Pack p;
      if (ua && on) p = *reinterpret_cast<const Pack*>(a.aval + l * a.m + j0);
      else {
#pragma unroll
        for (int v = 0; v < VT; v++) p.v[v] = T();
      }
      return p;
    };
    uint64_t l = b;
    for (; l + GEMV_T_UNROLL <= e; l += GEMV_T_UNROLL) {
      Pack av[GEMV_T_UNROLL];
#pragma unroll
      for (uint32_t r = 0; r < GEMV_T_UNROLL; r++) av[r] = load(l + r);
#pragma unroll
      for (uint32_t r = 0; r < GEMV_T_UNROLL; r++) fold_row(av[r], l + r);
    }
    for (; l < e; l++) fold_row(load(l), l);
    __syncthreads();                                                                 // the unit before has read its LDS
    if (w) { lds_acc[w][lane] = acc; if (lane == 0) lds_has[w] = has ? 1 : 0; }
    __syncthreads();
    if (w == 0) {
      for (uint32_t x = 1; x < GEMV_WAVES; x++) {
        if (!lds_has[x]) continue;
        const Pack p = lds_acc[x][lane];
#pragma unroll
        for (int v = 0; v < VT; v++) acc.v[v] = has ? sr.add(acc.v[v], p.v[v]) : p.v[v];
        has = true;
      }
      if (on) {
#pragma unroll
        for (int v = 0; v < VT; v++) gemv_store(a, GEMV_T, j0 + v, c, acc.v[v], has);
      }
    }
  }
}

template <class T, class SR>
__global__ __launch_bounds__(256) void k_gemv_fold(SR sr, GemvKArgs<T> a, int layout) {
  for (uint64_t o = blockIdx.x * 256ull + threadIdx.x; o < a.m; o += gridDim.x * 256ull) {
    T acc = T(); bool has = false;
    for (uint64_t c = 0; c < a.chunks; c++) {
      const uint64_t s = gemv_slot(layout, o, c, a.m, a.chunks);
      if (a.flag[s]) gemv_join(sr, acc, has, a.part[s], true);
    }
    a.tval[o] = acc;                                                                 // (u holds an entry: some chunk has a value)
  }
}

template <class T> void run_gemv_values(const GemvValuesCall& c, const SemiringDesc& d) {
  with_semiring<T>(d, [&](auto sr) {
    using SR = decltype(sr);
    GemvKArgs<T> a{};
    a.aval = (const T*)c.aval; a.uval = (const T*)c.uval; a.upres = c.upres; a.tval = (T*)c.tval; a.part = (T*)c.part; a.flag = c.flag;
    a.m = c.m; a.k = c.k; a.chunks = c.chunks;
    const bool t_scalar = gemv_t_vt(c.m, sizeof(T)) == 1 || (uintptr_t)c.aval % GEMV_LOAD_BYTES != 0;      // (a value array that is a view into somebody's tensor may start anywhere)
    a.slabs = t_scalar ? gemv_ceil_div(c.m, 64) : gemv_t_slabs(c.m, sizeof(T));
    const dim3 block(GEMV_WAVES * 64);
    if (c.layout == GEMV_N && gemv_n_short(c.k)) {
      uint32_t gshift = 0; while ((1u << gshift) < gemv_group(c.k)) gshift++;
      hipLaunchKernelGGL((k_gemv_n_short<T, SR>), dim3(gemv_grid(c.m, gemv_rows_per_workgroup(c.k))), block, 0, stream(), sr, a, gshift);
    } else if (c.layout == GEMV_N) {
      hipLaunchKernelGGL((k_gemv_n_wave<T, SR>), dim3(gemv_grid(gemv_mul_sat(c.m, c.chunks), GEMV_WAVES)), block, 0, stream(), sr, a);
    } else {
      constexpr int V = (int)gemv_vec(sizeof(T));
      const dim3 grid(gemv_grid(gemv_mul_sat(a.slabs, c.chunks), 1));
      if (t_scalar) hipLaunchKernelGGL((k_gemv_t<T, SR, 1>), grid, block, 0, stream(), sr, a);
      else hipLaunchKernelGGL((k_gemv_t<T, SR, V>), grid, block, 0, stream(), sr, a);
    }
    if (c.chunks > 1) hipLaunchKernelGGL((k_gemv_fold<T, SR>), dim3(gemv_grid(c.m, 256)), dim3(256), 0, stream(), sr, a, c.layout);
    GRB_HIP(hipGetLastError());
  });
}

}  // namespace grb
