// grb_build.hip — GrB_Matrix_build / GrB_Vector_build in HBM: tuples (I, J, X) in any order, duplicates included, to the sorted distinct positions with the
// duplicates folded LEFT TO RIGHT IN INPUT ORDER — z = dup(dup(dup(x0, x1), x2), ...), the order SuiteSparse and the host route (build_tuples, grb_build_ops.cpp)
// define; FP PLUS / TIMES are not bit-associative and FIRST / SECOND / MINUS are not commutative, so the order is part of the result.  The routes are in
// grb_build_ops.cpp, the key arithmetic and the thresholds in grb_build_keys.hpp.  All kernels are streaming or gather passes: wave64, 256 threads, grid-stride
// (grid_1d), no LDS, plain vector stores; the only atomic is one max per wave of k_build_runmax.
//
//   k_build_keys     one pass over I, J as 64-bit values: the bounds test (on the full values, before anything is truncated), key = (i << cbits) | j as a 32- or
//                    64-bit word, payload = the input position, and "the keys are strictly increasing": a lane takes its predecessor's key from the lane below
//                    (shfl_up), lane 0 of every wave — thread 0 of a workgroup among them — packs it again from I[k - 1], J[k - 1].  Two flag words.
//   sorted input     strictly increasing keys are distinct and in order: k_build_unpack writes rows / col from the keys, X is the value array.  No sort, no fold.
//   sort             rocPRIM's stable radix sort of (key, position) over rbits + cbits bits: equal keys keep their input order in the payload.
//   k_build_heads    flag[k] = the sorted key k starts a run; an exclusive scan gives every head its output position and, in its last word, nvals.
//   k_build_starts   start[r] = the sorted position of run r's head (start[nvals] = n), rows[r] / col[r] from its key.
//   k_build_runmax   the longest run (a max per lane, a wave reduction, one atomicMax per wave): decides DUPLICATE without dup, and the fold's shape.
//   k_build_fold<T>  val[r] = the run's values X[perm[start[r] ..]] folded in that order.  A LANE PER RUN up to BUILD_RUN_SERIAL values.  Longer runs: the wave
//                    takes them one after the other (ballot over its 64 runs), 64 gathered values at a time in input order; an operator that is exactly
//                    associative on T folds the 64 by an order-preserving shfl_down tree (lane l combines [l, l + d) with [l + d, l + 2d), left operand
//                    first — never an xor butterfly, which would swap operands: FIRST / SECOND / ANY are not commutative) and carries lane 0's result from
//                    chunk to chunk; any other operator folds the 64 one by one in lane order (every lane computes the same chain from broadcasts).
//   rows -> rowptr   k_rowptr_from_sorted (grb_transpose.hip), or k_build_rowptr_search when the rows outnumber the entries BUILD_ROWPTR_SEARCH_FACTOR times.
// Three read-backs of a few bytes: the flags, nvals (for the allocation), the longest run.
#include "grb_build.hpp"
#include "grb_index.hpp"
#include "grb_matops.hpp"

namespace grb {
namespace {

static_assert(B_FIRST == 0 && B_MAX == 5 && B_PLUS == 6 && B_MINUS == 7 && B_RMINUS == 8 && B_TIMES == 9 && B_ISEQ == 13 && B_ISNE == 14 && B_LOR == 19 && B_LXOR == 21 &&
              B_EQ == 22 && B_NE == 23 && B_LXNOR == 28 && B_BOR == 29 && B_BXNOR == 32, "build_op_tree_foldable (grb_build_keys.hpp) names the opcodes by number");
static_assert(BUILD_DIM_MAX == GRB_DIM_DEVICE_MAX, "the build route's dimension limit is the device layout's");

template <class KEY>
__global__ __launch_bounds__(256) void k_build_keys(const uint64_t* __restrict__ I, const uint64_t* __restrict__ J, uint64_t n, uint64_t nrows, uint64_t ncols, int cbits,
                                                    KEY* __restrict__ keys, uint32_t* __restrict__ pos, uint32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  bool oob = false, disorder = false;
  for (uint64_t base = blockIdx.x * 256ull; base < n; base += gridDim.x * 256ull) {      // (the bound is the workgroup's: every lane of a wave makes the same trips, the shuffle below is convergent)
    const uint64_t k = base + threadIdx.x; const bool valid = k < n;
    uint64_t key = 0;
    if (valid) {
      const uint64_t i = I[k], j = J ? J[k] : 0;
      oob = oob || !build_in_bounds(i, j, nrows, ncols);
      key = build_pack(i, j, cbits);                                  // (of an out-of-bounds pair: bits are lost, and the call fails before any key is read)
      keys[k] = (KEY)key; pos[k] = (uint32_t)k;
    }
    uint64_t prev = shfl_up_t<uint64_t>(key, 1);
    if (valid && k > 0) {
      if (lane == 0) prev = build_pack(I[k - 1], J ? J[k - 1] : 0, cbits);      // the wave (and workgroup) before: from the input, not from another wave's registers
      disorder = disorder || !(prev < key);
    }
  }
  const bool any_oob = __ballot(oob) != 0, any_dis = __ballot(disorder) != 0;
  if (lane == 0) { if (any_oob) flags[0] = 1u; if (any_dis) flags[1] = 1u; }      // (every writer stores the same word)
}

template <class KEY>
__global__ __launch_bounds__(256) void k_build_unpack(const KEY* __restrict__ keys, uint64_t n, int cbits, uint32_t* __restrict__ rows, uint32_t* __restrict__ col) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n; k += gridDim.x * 256ull) {
    const uint64_t key = keys[k];
    rows[k] = build_key_row(key, cbits); if (col) col[k] = build_key_col(key, cbits);
  }
}

template <class KEY>
__global__ __launch_bounds__(256) void k_build_heads(const KEY* __restrict__ skeys, uint64_t n, uint32_t* __restrict__ flag) {      // flag[n] = 0: the scan's last word is nvals
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k <= n; k += gridDim.x * 256ull) flag[k] = (k < n && (k == 0 || skeys[k] != skeys[k - 1])) ? 1u : 0u;
}

template <class KEY>
__global__ __launch_bounds__(256) void k_build_starts(const KEY* __restrict__ skeys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ opos, uint64_t n, int cbits,
                                                      uint32_t* __restrict__ start, uint32_t* __restrict__ rows, uint32_t* __restrict__ col) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k <= n; k += gridDim.x * 256ull) {
    if (k == n) { start[opos[n]] = (uint32_t)n; continue; }
    if (!flag[k]) continue;
    const uint32_t r = opos[k]; const uint64_t key = skeys[k];        // (r < nvals: rows / col hold nvals words, start nvals + 1)
    start[r] = (uint32_t)k; rows[r] = build_key_row(key, cbits); if (col) col[r] = build_key_col(key, cbits);
  }
}

__global__ __launch_bounds__(256) void k_build_runmax(const uint32_t* __restrict__ start, uint64_t nvals, uint32_t* __restrict__ maxrun) {
  uint32_t m = 0;
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < nvals; r += gridDim.x * 256ull) { const uint32_t len = start[r + 1] - start[r]; m = len > m ? len : m; }
  m = __builtin_amdgcn_wave_reduce_max_u32(m, 0);
  if ((threadIdx.x & 63) == 0 && m > 1) atomicMax(maxrun, m);         // (maxrun starts at 1: a build without duplicates issues no atomic)
}

template <class T>
__global__ __launch_bounds__(256) void k_build_fold(int op, int tree, int have_long, const uint32_t* __restrict__ perm, const T* __restrict__ X, const uint32_t* __restrict__ start,
                                                    uint64_t nvals, T* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  for (uint64_t base = blockIdx.x * 256ull; base < nvals; base += gridDim.x * 256ull) {      // (the workgroup's bound: the wave stays convergent for the long runs below)
    const uint64_t r = base + threadIdx.x; const bool valid = r < nvals;
    uint32_t s = 0, len = 0;
    if (valid) {
      s = start[r]; len = start[r + 1] - s;
      if (len <= BUILD_RUN_SERIAL) {
        T z = X[perm[s]];
        for (uint32_t p = 1; p < len; p++) z = apply_binop<T, true, false>(op, z, X[perm[s + p]]);
        val[r] = z;
      }
    }
    if (!have_long) continue;                                         // (uniform: the longest run of the call fits a lane)
    uint64_t todo = __ballot(valid && len > BUILD_RUN_SERIAL);
    while (todo) {                                                    // the wave's long runs, one after the other, all 64 lanes on each
      const int owner = __ffsll((unsigned long long)todo) - 1; todo &= todo - 1;
      const uint32_t rs = (uint32_t)__shfl((int)s, owner, 64), rl = (uint32_t)__shfl((int)len, owner, 64);
      T z = X[perm[rs]];                                              // (overwritten by the first chunk)
      for (uint32_t c = 0; c < rl; c += 64) {
        const uint32_t cnt = rl - c < 64u ? rl - c : 64u;
        T v = X[perm[rs + c + ((uint32_t)lane < cnt ? (uint32_t)lane : 0u)]];      // input order across the lanes (a lane past the run's end re-reads its first value and is never combined)
        if (tree) {
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {                          // lane l: [l, l + d) then [l + d, l + 2d), left operand first
            const T o = shfl_down_t<T>(v, d);
            if ((uint32_t)(lane + d) < cnt) v = apply_binop<T, true, false>(op, v, o);
          }
          const T head = shfl_t<T>(v, 0);
          z = c == 0 ? head : apply_binop<T, true, false>(op, z, head);
        } else {
          for (uint32_t q = 0; q < cnt; q++) { const T x = shfl_t<T>(v, (int)q); z = (c == 0 && q == 0) ? x : apply_binop<T, true, false>(op, z, x); }
        }
      }
      if (lane == owner) val[r] = z;
    }
  }
}

__global__ __launch_bounds__(256) void k_build_rowptr_search(const uint32_t* __restrict__ rows, uint32_t nvals, uint64_t nwords, uint32_t* __restrict__ rowptr) {
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < nwords; r += gridDim.x * 256ull) rowptr[r] = lower_bound_u32(rows, nvals, (uint32_t)r);      // entries in rows before r
}

// a few device words to the host: one copy per word group, one synchronisation
void read_words(const uint32_t* dev, uint32_t* out, int nwords) {
  uint32_t* pin = (uint32_t*)pinned_scratch();
  GRB_HIP(hipMemcpyAsync(pin, dev, (size_t)nwords * 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  for (int w = 0; w < nwords; w++) out[w] = pin[w];
}

template <class KEY>
BuildResult build_keyed(int tcode, const uint64_t* I, const uint64_t* J, const void* X, uint64_t n, uint64_t nrows, uint64_t ncols, int rbits, int cbits, int dup_op,
                        DevBuf& rows, DevBuf* col, DevBuf& val) {
  BuildResult res; res.key64 = sizeof(KEY) == 8;
  const size_t ts = type_size(tcode);
  DevBuf keys(n * sizeof(KEY)), pos(n * 4), words(16);
  GRB_HIP(hipMemsetAsync(words.p, 0, 16, stream()));
  hipLaunchKernelGGL((k_build_keys<KEY>), dim3(grid_1d(n)), dim3(256), 0, stream(), I, J, n, nrows, ncols, cbits, keys.as<KEY>(), pos.as<uint32_t>(), words.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  uint32_t f[2]; read_words(words.as<uint32_t>(), f, 2);
  if (f[0]) { res.status = BUILD_OUT_OF_BOUNDS; return res; }
  if (!f[1]) {                                                         // strictly increasing: distinct and in order
    res.sorted = true; res.nvals = n;
    rows.alloc(n * 4 + 4); if (col) col->alloc(n * 4 + 4); val.alloc(n * ts + 8);
    hipLaunchKernelGGL((k_build_unpack<KEY>), dim3(grid_1d(n)), dim3(256), 0, stream(), keys.as<KEY>(), n, cbits, rows.as<uint32_t>(), col ? col->as<uint32_t>() : nullptr);
    GRB_HIP(hipGetLastError());
    GRB_HIP(hipMemcpyAsync(val.p, X, n * ts, hipMemcpyDeviceToDevice, stream()));
    return res;
  }
  DevBuf skeys(n * sizeof(KEY)), perm(n * 4);
  if constexpr (sizeof(KEY) == 8) sort_pairs_u64(keys.as<uint64_t>(), skeys.as<uint64_t>(), pos.as<uint32_t>(), perm.as<uint32_t>(), n, build_sort_bits(rbits, cbits));
  else sort_pairs_u32(keys.as<uint32_t>(), skeys.as<uint32_t>(), pos.as<uint32_t>(), perm.as<uint32_t>(), n, build_sort_bits(rbits, cbits));
  keys.reset(); pos.reset();                                           // (stream-ordered pool: what follows may reuse them)
  DevBuf flag((n + 1) * 4), opos((n + 1) * 4);
  hipLaunchKernelGGL((k_build_heads<KEY>), dim3(grid_1d(n + 1)), dim3(256), 0, stream(), skeys.as<KEY>(), n, flag.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  exclusive_scan_u32(flag.as<uint32_t>(), opos.as<uint32_t>(), n + 1);
  uint32_t nv32 = 0; read_words(opos.as<uint32_t>() + n, &nv32, 1);
  const uint64_t nvals = nv32;
  DevBuf start((nvals + 1) * 4), orow(nvals * 4 + 4), ocol;
  if (col) ocol.alloc(nvals * 4 + 4);
  hipLaunchKernelGGL((k_build_starts<KEY>), dim3(grid_1d(n + 1)), dim3(256), 0, stream(), skeys.as<KEY>(), flag.as<uint32_t>(), opos.as<uint32_t>(), n, cbits,
                     start.as<uint32_t>(), orow.as<uint32_t>(), col ? ocol.as<uint32_t>() : nullptr);
  GRB_HIP(hipGetLastError());
  GRB_HIP(hipMemsetD32Async((hipDeviceptr_t)(words.as<uint32_t>() + 2), 1, 1, stream()));
  hipLaunchKernelGGL(k_build_runmax, dim3(grid_1d(nvals)), dim3(256), 0, stream(), start.as<uint32_t>(), nvals, words.as<uint32_t>() + 2);
  GRB_HIP(hipGetLastError());
  uint32_t maxrun = 1; read_words(words.as<uint32_t>() + 2, &maxrun, 1);
  if (maxrun > 1 && dup_op < 0) { res.status = BUILD_DUPLICATE; return res; }
  const bool tree = dup_op >= 0 && build_op_tree_foldable(dup_op, tcode == T_FP32 || tcode == T_FP64, tcode == T_BOOL);
  if (maxrun > BUILD_RUN_SERIAL_MAX && !tree) { res.status = BUILD_RUN_TOO_LONG; return res; }
  const bool have_long = maxrun > BUILD_RUN_SERIAL;
  res.fold = maxrun == 1 ? "none" : (have_long && tree) ? "wave" : "serial";
  res.nvals = nvals;
  val.alloc(nvals * ts + 8);
  dispatch_type(tcode, [&]<class T>() {
    hipLaunchKernelGGL((k_build_fold<T>), dim3(grid_1d(nvals)), dim3(256), 0, stream(), dup_op < 0 ? (int)B_FIRST : dup_op, tree ? 1 : 0, have_long ? 1 : 0, perm.as<uint32_t>(),
                       (const T*)X, start.as<uint32_t>(), nvals, val.as<T>());
  });
  GRB_HIP(hipGetLastError());
  rows = std::move(orow); if (col) *col = std::move(ocol);
  return res;
}

}  // namespace

BuildResult build_from_tuples(int tcode, const uint64_t* I, const uint64_t* J, const void* X, uint64_t n, uint64_t nrows, uint64_t ncols, int dup_op,
                              DevBuf& rows, DevBuf* col, DevBuf& val) {
  if (tcode < T_BOOL || tcode > T_FP64) fail(GrB_PANIC, "build: no device route for this type");      // (the caller's route test: the kernels are instantiated for the 11 real types)
  if (nrows > BUILD_DIM_MAX || ncols > BUILD_DIM_MAX || n > BUILD_TUPLES_MAX) fail(GrB_PANIC, "build: the tuples do not fit the 32-bit device layout");
  rows.reset(); if (col) col->reset(); val.reset();
  if (!n) { BuildResult res; res.sorted = true; return res; }
  const int rbits = build_bits(nrows), cbits = J ? build_bits(ncols) : 0;
  if (build_key_is_u32(rbits, cbits)) return build_keyed<uint32_t>(tcode, I, J, X, n, nrows, J ? ncols : 1, rbits, cbits, dup_op, rows, col, val);
  return build_keyed<uint64_t>(tcode, I, J, X, n, nrows, J ? ncols : 1, rbits, cbits, dup_op, rows, col, val);
}

bool build_rowptr(const uint32_t* rows, uint64_t nvals, uint32_t nrows, uint32_t* rowptr) {
  if (nvals && (uint64_t)nrows > BUILD_ROWPTR_SEARCH_FACTOR * (nvals + 1)) {
    const uint64_t nwords = (uint64_t)nrows + 1;
    hipLaunchKernelGGL(k_build_rowptr_search, dim3(grid_1d(nwords)), dim3(256), 0, stream(), rows, (uint32_t)nvals, nwords, rowptr);
    GRB_HIP(hipGetLastError());
    return true;
  }
  rowptr_from_sorted(rows, nvals, nrows, rowptr);
  GRB_HIP(hipGetLastError());
  return false;
}

}  // namespace grb
