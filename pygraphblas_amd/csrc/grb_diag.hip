// grb_diag.hip — diagonals in HBM: a vector bitmap onto the k-th diagonal of a square CSR (behind GxB_Matrix_diag), and the k-th diagonal of a CSR as a
// bitmap (behind GxB_Vector_diag); the routes are in grb_diag_ops.cpp.  Both are streaming passes: no LDS, no atomics, every output position has one writer.
//
//   diag_to_csr         T has at most one entry per row, so its row pointer IS the exclusive scan of v's presence bytes, shifted by the |k| rows before the
//                       diagonal (k < 0, all 0) and followed by the |k| rows after it (k >= 0, all nnz(T)).  The scan (present_positions: rocPRIM, over the bytes widened to
//                       32 bits) goes straight into rowptr + row0; nnz(T) is its last word: the one read-back, for the allocation.
//     k_diag_fill       ENTRY-PARALLEL: a lane owns DIAG_EPL = 4 consecutive positions of v.  It loads their presence bytes as one 4-byte word (nothing
//                       else when that is 0), the values as one 16-byte pack (two for 8-byte values, a narrower one below 4), the scanned position of the
//                       first one, and stores column r + col0 and the value of every present position at consecutive places from there.  The same lanes
//                       then write the |k| flat words of the row pointer.  Unaligned views and the last partial group go entry by entry.
//     FULL              every position of v holds an entry (no presence bytes, or a count known equal to n): position r IS place r — no scan, no
//                       read-back; the lane's four columns, its four row-pointer words and its values leave as packs.
//   traffic             read n (1 + ts) bytes (+ 4 n for the scan), written nnz (4 + ts) + 4 (n + |k| + 1).
//
//   csr_diag_to_bitmap
//     k_diag_read       a lane owns diagonal position r = entry (r + row0, r + col0): two row-pointer words, then the row's (sorted) columns — a linear
//                       scan up to DIAG_LINEAR entries, a bisection beyond (a hub row of 10^5 entries: 17 probes) — and one presence byte and one value
//                       (0 where absent) stored.  Nothing is read back; the entry count stays unknown.
// Values move as words of their size (1, 2, 4, 8 bytes), never by type: the typecast is the write-back's.
#include "grb_diag.hpp"
#include "grb_compact.hpp"
#include <algorithm>

namespace grb {
namespace {

constexpr int DIAG_EPL = 4;                                                  // positions per lane: one presence word, 16 bytes of columns
constexpr uint32_t DIAG_LINEAR = 8;                                          // rows up to this long are scanned, longer ones bisected

template <int TS> struct alignas(TS * DIAG_EPL > 16 ? 16 : TS * DIAG_EPL) ValPack { typename WordOf<TS>::type v[DIAG_EPL]; };
struct alignas(16) U32Pack { uint32_t c[DIAG_EPL]; };
struct alignas(4) PresPack { uint8_t b[DIAG_EPL]; };

// rp = T.rowptr + row0: rp[r] is the place of position r's entry (FULL: written here; else the scan put it there).  `flat`: the |k| row-pointer words outside
// [row0, row0 + n] — T.rowptr (k < 0) or rp + n + 1 (k >= 0) — all `flat_val`.
template <int TS, bool FULL>
__global__ __launch_bounds__(256) void k_diag_fill(uint64_t n, const uint8_t* __restrict__ vval, const uint8_t* __restrict__ vpres, uint32_t col0, uint32_t* __restrict__ rp,
                                                   uint32_t* __restrict__ flat, uint64_t nflat, uint32_t flat_val, uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval, int packed) {
  typedef typename WordOf<TS>::type W;
  const W* __restrict__ src = (const W*)vval; W* __restrict__ dst = (W*)oval;
  const uint64_t ngroups = (n + DIAG_EPL - 1) / DIAG_EPL;
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < ngroups; g += gridDim.x * 256ull) {
    const uint64_t r0 = g * DIAG_EPL;
    const int nv = n - r0 >= (uint64_t)DIAG_EPL ? DIAG_EPL : (int)(n - r0);
    if constexpr (FULL) {
      if (nv == DIAG_EPL && packed) {
        U32Pack c, p;
#pragma unroll
        for (int j = 0; j < DIAG_EPL; j++) { p.c[j] = (uint32_t)r0 + j; c.c[j] = (uint32_t)r0 + j + col0; }      // (n + |k| <= GRB_DIM_DEVICE_MAX: no wrap)
        *reinterpret_cast<U32Pack*>(rp + r0) = p;
        *reinterpret_cast<U32Pack*>(ocol + r0) = c;
        *reinterpret_cast<ValPack<TS>*>(dst + r0) = *reinterpret_cast<const ValPack<TS>*>(src + r0);
      } else {
        for (int j = 0; j < nv; j++) { rp[r0 + j] = (uint32_t)(r0 + j); ocol[r0 + j] = (uint32_t)(r0 + j) + col0; dst[r0 + j] = src[r0 + j]; }
      }
    } else {
      if (nv == DIAG_EPL && packed) {
        const PresPack pr = *reinterpret_cast<const PresPack*>(vpres + r0);
        if (!(pr.b[0] | pr.b[1] | pr.b[2] | pr.b[3])) continue;
        const ValPack<TS> v = *reinterpret_cast<const ValPack<TS>*>(src + r0);
        uint32_t o = rp[r0];
#pragma unroll
        for (int j = 0; j < DIAG_EPL; j++) if (pr.b[j]) { ocol[o] = (uint32_t)r0 + j + col0; dst[o] = v.v[j]; o++; }
      } else {
        for (int j = 0; j < nv; j++) if (vpres[r0 + j]) { const uint32_t o = rp[r0 + j]; ocol[o] = (uint32_t)(r0 + j) + col0; dst[o] = src[r0 + j]; }
      }
    }
  }
  if constexpr (FULL) { if (blockIdx.x == 0 && threadIdx.x == 0) rp[n] = (uint32_t)n; }      // the row pointer's last word inside the diagonal's rows
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < nflat; i += gridDim.x * 256ull) flat[i] = flat_val;
}

template <int TS>
__global__ __launch_bounds__(256) void k_diag_read(uint64_t len, uint32_t row0, uint32_t col0, const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint8_t* __restrict__ aval,
                                                   uint8_t* __restrict__ tval, uint8_t* __restrict__ tpres) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < len; r += gridDim.x * 256ull) {
    const uint32_t i = (uint32_t)r + row0, j = (uint32_t)r + col0;           // (i < nrows, j < ncols: len is the diagonal's length)
    const uint32_t lo = rowptr[i], hi = rowptr[i + 1];
    uint32_t p = hi;                                                         // where column j is stored, or hi
    if (hi - lo <= DIAG_LINEAR) { for (uint32_t q = lo; q < hi; q++) if (col[q] == j) p = q; }
    else { const uint32_t q = lo + lower_bound_u32(col + lo, hi - lo, j); if (q < hi && col[q] == j) p = q; }
    const bool found = p < hi;
    tpres[r] = found ? 1 : 0;
    ((W*)tval)[r] = found ? ((const W*)aval)[p] : W(0);
  }
}

inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

bool diag_to_csr(int tcode, uint64_t n_v, const void* vval, const uint8_t* vpres, int64_t k, DevCSR& T, bool all_present) {
  const size_t ts = type_size(tcode); check_value_size(ts, "diag");
  uint64_t n = 0;
  if (!diag_dim(n_v, k, &n) || n > GRB_DIM_DEVICE_MAX) fail(GrB_PANIC, "diag: the matrix does not fit the 32-bit device layout");      // (the entry point checked it: the kernels' bounds depend on it)
  const uint64_t ak = diag_abs(k), row0 = diag_row0(k), col0 = diag_col0(k);
  const bool full = !vpres || all_present || n_v == 0;
  T.clear(); T.nrows = (uint32_t)n; T.ncols = (uint32_t)n;
  T.rowptr.alloc((n + 1) * 4);
  uint32_t* rp = T.rowptr.as<uint32_t>() + row0;                              // rp[0 .. n_v]: the rows of the diagonal and the word after them
  uint64_t total = n_v;
  if (!full) total = present_positions_total(vpres, n_v, rp);                 // the one read-back
  T.nnz = total; T.col.alloc(total * 4 + 4); T.val.alloc(total * ts + 8);
  uint32_t* flat = k < 0 ? T.rowptr.as<uint32_t>() : rp + n_v + 1;
  const uint32_t flat_val = k < 0 ? 0u : (uint32_t)total;
  const size_t pa = ts * DIAG_EPL > 16 ? 16 : ts * DIAG_EPL;
  const int packed = aligned_to(vval, pa) && (full ? aligned_to(rp, 16) && aligned_to(T.col.p, 16) && aligned_to(T.val.p, pa) : aligned_to(vpres, 4)) ? 1 : 0;
  const uint64_t work = std::max<uint64_t>((n_v + DIAG_EPL - 1) / DIAG_EPL, ak);
  dispatch_value_size(ts, [&]<int TS>() {
    if (full) hipLaunchKernelGGL((k_diag_fill<TS, true>), dim3(grid_1d(work)), dim3(256), 0, stream(), n_v, (const uint8_t*)vval, vpres, (uint32_t)col0, rp, flat, ak, flat_val, T.col.as<uint32_t>(), T.val.as<uint8_t>(), packed);
    else hipLaunchKernelGGL((k_diag_fill<TS, false>), dim3(grid_1d(work)), dim3(256), 0, stream(), n_v, (const uint8_t*)vval, vpres, (uint32_t)col0, rp, flat, ak, flat_val, T.col.as<uint32_t>(), T.val.as<uint8_t>(), packed);
  });
  GRB_HIP(hipGetLastError());
  T.valid = true;
  return full;
}

void csr_diag_to_bitmap(size_t ts, const DevCSR& A, int64_t k, uint64_t len, void* tval, uint8_t* tpres) {
  check_value_size(ts, "diag");
  if (len != diag_len(A.nrows, A.ncols, k)) fail(GrB_PANIC, "diag: the length does not match the matrix");      // (the entry point computed it: the kernel's bounds depend on it)
  if (!len) return;
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_diag_read<TS>), dim3(grid_1d(len)), dim3(256), 0, stream(), len, (uint32_t)diag_row0(k), (uint32_t)diag_col0(k), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), A.val.as<uint8_t>(),
                       (uint8_t*)tval, tpres);
  });
  GRB_HIP(hipGetLastError());
}

}  // namespace grb
