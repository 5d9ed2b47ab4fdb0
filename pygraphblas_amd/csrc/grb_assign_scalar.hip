// grb_assign_scalar.hip — the operand of the matrix scalar assign C<M>(I, J) = accum(C(I, J), s) in HBM (behind GrB_Matrix_assign_<T>; the route is do_assign_scalar,
// grb_matrix_ops.cpp).  T holds the scalar at every position the write-back may read; it has C's shape and sorted rows, and the write-back does the rest.
// Index arguments arrive as ExIdx (grb_extract.hpp), never expanded, with the inverse tables of assign_inverse for explicit lists (no index named twice).
//
//   scalar_from_mask      a mask that is not complemented only lets the write-back read T where M is true: T = M's true entries inside I x J.
//     k_assign_scalar_flags   ONE THREAD PER ENTRY of M (its row from csr_row_indices): row in I, column in J (idx_inv: closed form or one table word), value
//                             non-zero in M's own type (nothing read under GrB_STRUCTURE) -> one keep byte.  csr_compact then makes T's pattern.
//     k_assign_scalar_fill    <TS, false>: the scalar into T's values, a lane owns SCALAR_EPL = 4 consecutive entries: one 16-byte store (4-byte values),
//                             two (8-byte) or a narrower one.
//     traffic                 read nnz(M) (8 + ms) bytes (+ the scans of csr_row_indices and csr_compact), written nnz(T) (4 + ts).  Nothing depends on |I| |J|.
//   scalar_block          no mask, or a complemented one: T = all of I x J, in closed form.
//     rows                    one flag per row of C (idx_inv(I, r) != NONE), its exclusive scan (rocPRIM) times ncs = |J| is the row pointer.  No read-back:
//                             nnz(T) = |I| |J| is known.
//     columns                 sorted: GrB_ALL and ranges in closed form (a backwards range read from its far end), an increasing list as uploaded, any other
//                             list once per call as the compaction of its inverse table (flags over C's columns, scan, scatter) — no sort.
//     k_assign_scalar_fill    <TS, true>: entry p holds column cols[p mod ncs]: the lane divides once for its first entry and steps (wrapping) for the other
//                             three; the four columns leave as ONE 16-byte store, the values as above.  The last partial group and unaligned arrays go
//                             entry by entry.
//     traffic                 written |I| |J| (4 + ts) bytes, once, coalesced — the whole cost; read: the column list through the caches.
// No atomics, no LDS: every output position has one writer.  Values move as words of their size, never by type.
#include "grb_assign_scalar.hpp"
#include "grb_index.hpp"
#include "grb_matops.hpp"

namespace grb {
namespace {

constexpr int SCALAR_EPL = 4;                                                // entries per lane: 16 bytes of columns

template <int TS> struct alignas(TS * SCALAR_EPL > 16 ? 16 : TS * SCALAR_EPL) ValPack { typename WordOf<TS>::type v[SCALAR_EPL]; };
struct alignas(16) ColPack { uint32_t c[SCALAR_EPL]; };

__global__ void k_assign_scalar_flags(uint64_t nnz, const uint32_t* __restrict__ rowidx, const uint32_t* __restrict__ mcol, const void* __restrict__ mval, int mcode, bool mstruct, DIdx I, DIdx J,
                                      uint8_t* __restrict__ keep) {
  for (uint64_t p = blockIdx.x * 256ull + threadIdx.x; p < nnz; p += gridDim.x * 256ull)
    keep[p] = (idx_inv(I, rowidx[p]) != NONE && idx_inv(J, mcol[p]) != NONE && mask_truth_at(mval, mcode, p, mstruct)) ? 1 : 0;
}

__global__ void k_assign_scalar_rowflag(DIdx I, uint64_t nrows, uint32_t* __restrict__ out) {      // out[nrows] = 0: the scan's last word is the number of selected rows
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows; r += gridDim.x * 256ull) out[r] = (r < nrows && idx_inv(I, (uint32_t)r) != NONE) ? 1u : 0u;
}
__global__ void k_assign_scalar_rowptr(uint32_t* __restrict__ rp, uint64_t nrows, uint32_t ncs) {      // selected rows before r -> entries before row r (<= SCALAR_REGION_MAX)
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows; r += gridDim.x * 256ull) rp[r] *= ncs;
}
__global__ void k_assign_scalar_colflag(const uint32_t* __restrict__ inv, uint64_t ncols, uint32_t* __restrict__ out) {
  for (uint64_t c = blockIdx.x * 256ull + threadIdx.x; c <= ncols; c += gridDim.x * 256ull) out[c] = (c < ncols && inv[c] != NONE) ? 1u : 0u;
}
__global__ void k_assign_scalar_colscatter(const uint32_t* __restrict__ inv, const uint32_t* __restrict__ pos, uint64_t ncols, uint32_t* __restrict__ cols) {
  for (uint64_t c = blockIdx.x * 256ull + threadIdx.x; c < ncols; c += gridDim.x * 256ull) if (inv[c] != NONE) cols[pos[c]] = (uint32_t)c;      // (pos[c] < the list's length: one slot per named column)
}

// n entries (n <= SCALAR_REGION_MAX: positions fit 32 bits), every value = the low TS bytes of `sbits`.  COLS: entry p also gets the (p mod ncs)-th smallest
// selected column — cols[k], or first + k step where `cols` is nullptr.
template <int TS, bool COLS>
__global__ __launch_bounds__(256) void k_assign_scalar_fill(uint64_t n, uint64_t sbits, uint32_t ncs, uint32_t first, uint32_t step, const uint32_t* __restrict__ cols, uint32_t* __restrict__ ocol,
                                                            uint8_t* __restrict__ oval, int packed) {
  typedef typename WordOf<TS>::type W;
  W* __restrict__ dst = (W*)oval;
  const W s = (W)sbits;
  ValPack<TS> v;
#pragma unroll
  for (int j = 0; j < SCALAR_EPL; j++) v.v[j] = s;
  const uint64_t ngroups = (n + SCALAR_EPL - 1) / SCALAR_EPL;
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < ngroups; g += gridDim.x * 256ull) {
    const uint64_t p0 = g * SCALAR_EPL;
    const int nv = n - p0 >= (uint64_t)SCALAR_EPL ? SCALAR_EPL : (int)(n - p0);
    ColPack c;
    if constexpr (COLS) {
      uint32_t k = (uint32_t)p0 % ncs;                                      // the one division of the group
#pragma unroll
      for (int j = 0; j < SCALAR_EPL; j++) {
        c.c[j] = j < nv ? (cols ? cols[k] : first + k * step) : 0u;
        k = k + 1 == ncs ? 0u : k + 1;
      }
    }
    if (nv == SCALAR_EPL && packed) {
      if constexpr (COLS) *reinterpret_cast<ColPack*>(ocol + p0) = c;
      *reinterpret_cast<ValPack<TS>*>(dst + p0) = v;
    } else {
      for (int j = 0; j < nv; j++) { if constexpr (COLS) ocol[p0 + j] = c.c[j]; dst[p0 + j] = s; }
    }
  }
}

inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

template <bool COLS>
void launch_fill(size_t ts, uint64_t n, const void* scalar, uint32_t ncs, uint32_t first, uint32_t step, const uint32_t* cols, DevCSR& T) {
  uint64_t sbits = 0; memcpy(&sbits, scalar, ts);
  const size_t pa = ts * SCALAR_EPL > 16 ? 16 : ts * SCALAR_EPL;
  const int packed = aligned_to(T.col.p, 16) && aligned_to(T.val.p, pa) ? 1 : 0;
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_assign_scalar_fill<TS, COLS>), dim3(grid_1d((n + SCALAR_EPL - 1) / SCALAR_EPL)), dim3(256), 0, stream(), n, sbits, ncs, first, step, cols, T.col.as<uint32_t>(), T.val.as<uint8_t>(), packed);
  });
  GRB_HIP(hipGetLastError());
}

void empty_like(uint32_t nrows, uint32_t ncols, DevCSR& T) {
  T.clear(); T.nrows = nrows; T.ncols = ncols; T.nnz = 0;
  T.rowptr.alloc(((size_t)nrows + 1) * 4); T.col.alloc(8); T.val.alloc(8);
  GRB_HIP(hipMemsetAsync(T.rowptr.p, 0, ((size_t)nrows + 1) * 4, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));
  T.valid = true;
}

}  // namespace

void scalar_from_mask(const DevCSR& M, int mcode, bool mstruct, const ExIdx& I, const DevBuf& inv_i, const ExIdx& J, const DevBuf& inv_j, const void* scalar, size_t ts, DevCSR& T) {
  check_value_size(ts, "assign");
  if (I.kind == EX_LIST && !inv_i.p) fail(GrB_PANIC, "assign: a row list without its inverse table");      // (the caller built them: the kernel's reads depend on it)
  if (J.kind == EX_LIST && !inv_j.p) fail(GrB_PANIC, "assign: a column list without its inverse table");
  const uint64_t nnz = M.nnz;
  if (!nnz || !I.n || !J.n) { empty_like(M.nrows, M.ncols, T); return; }
  DevBuf rowidx(nnz * 4 + 4), keep(nnz + 1);
  csr_row_indices(M, rowidx.as<uint32_t>());
  hipLaunchKernelGGL(k_assign_scalar_flags, dim3(grid_1d(nnz)), dim3(256), 0, stream(), nnz, rowidx.as<uint32_t>(), M.col.as<uint32_t>(), (const void*)M.val.p, mcode, mstruct, didx(I, &inv_i), didx(J, &inv_j),
                     keep.as<uint8_t>());
  GRB_HIP(hipGetLastError());
  // the pattern alone: the compaction moves one placeholder byte per entry (the keep bytes themselves), the values are written below
  csr_compact(M, keep.p, 1, keep.as<uint8_t>(), T);                          // (synchronises: nnz(T) is read back for the allocation)
  T.val.alloc(T.nnz * ts + 8);
  if (T.nnz) launch_fill<false>(ts, T.nnz, scalar, 1u, 0u, 1u, nullptr, T);
  GRB_HIP(hipStreamSynchronize(stream()));                                   // rowidx / keep return to the pool
  T.valid = true;
}

void scalar_block(uint32_t nrows, uint32_t ncols, const ExIdx& I, const DevBuf& inv_i, const ExIdx& J, const DevBuf& inv_j, const void* scalar, size_t ts, DevCSR& T) {
  check_value_size(ts, "assign");
  if (I.n > nrows || J.n > ncols || !scalar_region_fits(I.n, J.n)) fail(GrB_PANIC, "assign: the block does not fit the 32-bit device layout");      // (the entry point checked it: the kernels' bounds depend on it)
  if (I.kind == EX_LIST && !inv_i.p) fail(GrB_PANIC, "assign: a row list without its inverse table");
  const uint64_t total = scalar_region_entries(I.n, J.n);
  if (!total) { empty_like(nrows, ncols, T); return; }
  const uint32_t ncs = (uint32_t)J.n;
  T.clear(); T.nrows = nrows; T.ncols = ncols; T.nnz = total;
  T.rowptr.alloc(((size_t)nrows + 1) * 4); T.col.alloc(total * 4 + 4); T.val.alloc(total * ts + 8);
  DevBuf flags(((size_t)nrows + 1) * 4);
  hipLaunchKernelGGL(k_assign_scalar_rowflag, dim3(grid_1d((uint64_t)nrows + 1)), dim3(256), 0, stream(), didx(I, &inv_i), (uint64_t)nrows, flags.as<uint32_t>());
  exclusive_scan_u32(flags.as<uint32_t>(), T.rowptr.as<uint32_t>(), (uint64_t)nrows + 1);
  hipLaunchKernelGGL(k_assign_scalar_rowptr, dim3(grid_1d((uint64_t)nrows + 1)), dim3(256), 0, stream(), T.rowptr.as<uint32_t>(), (uint64_t)nrows, ncs);
  // the selected columns in increasing order
  uint32_t first = 0, step = 1; const uint32_t* cols = nullptr;
  DevBuf cflags, cpos, sorted;
  if (J.kind == EX_RANGE || J.kind == EX_BACK) {
    step = J.step ? J.step : 1u;
    first = (uint32_t)scalar_range_first(J.kind == EX_BACK, J.lo, step, J.n);
  } else if (J.kind == EX_LIST) {
    if (J.increasing) cols = J.list;
    else {
      if (!inv_j.p) fail(GrB_PANIC, "assign: a column list without its inverse table");
      cflags.alloc(((size_t)ncols + 1) * 4); cpos.alloc(((size_t)ncols + 1) * 4); sorted.alloc((size_t)ncs * 4);
      hipLaunchKernelGGL(k_assign_scalar_colflag, dim3(grid_1d((uint64_t)ncols + 1)), dim3(256), 0, stream(), inv_j.as<uint32_t>(), (uint64_t)ncols, cflags.as<uint32_t>());
      exclusive_scan_u32(cflags.as<uint32_t>(), cpos.as<uint32_t>(), (uint64_t)ncols + 1);
      hipLaunchKernelGGL(k_assign_scalar_colscatter, dim3(grid_1d(ncols)), dim3(256), 0, stream(), inv_j.as<uint32_t>(), cpos.as<uint32_t>(), (uint64_t)ncols, sorted.as<uint32_t>());
      cols = sorted.as<uint32_t>();
    }
  }
  launch_fill<true>(ts, total, scalar, ncs, first, step, cols, T);
  GRB_HIP(hipStreamSynchronize(stream()));                                   // the temporaries return to the pool
  T.valid = true;
}

}  // namespace grb
