// grb_assign.hip — index-list assign in HBM: the operand moved into C's coordinates (CSR in, CSR out), the entries of C inside I x J flagged, w(I) = u on bitmaps.
//
// Index arguments arrive as ExIdx (grb_extract.hpp), never expanded: GrB_ALL and the GxB_RANGE / GxB_STRIDE / GxB_BACKWARDS triples are evaluated — and inverted —
// in closed form by the kernels; an explicit list is uploaded once (4 bytes per index) and its inverse is one table of `dim` uint32, scattered with plain stores.
// A list that names an index twice is found by reading the table back through the list (inv[I[k]] != k for the k that lost) and is left to the host route.
//
// T = A in C's coordinates (assign_relocate):
//   rows     source row a becomes row I[a]: len[I[a]] = length of row a, one exclusive scan over C's rows is T's row pointer.  The rows are a permutation, so a
//            non-increasing I needs no sort.
//   entries  ONE THREAD PER ENTRY of A (its row from csr_row_indices): dst = rowptr_T[I[a]] + (p - rowptr_A[a]), column J[col]: a hub row of 10^5 entries is
//            10^5 threads like any other 10^5 entries — no parts, no long-row path; reads and writes are contiguous within a row.
//   columns  a strictly increasing J keeps every row sorted; any other J gets the segmented row sort of the extract fill (rocPRIM, (column, position) pairs,
//            then one gather of the values).
//   traffic  (12 + ts) bytes read and (4 + ts) written per entry of A, 8 bytes per row of C.
// No atomics anywhere: every output position has exactly one writer.
#include "grb_assign.hpp"
#include "grb_compact.hpp"
#include "grb_matops.hpp"

namespace grb {
namespace {

// ---- the inverse table of a list, and the repeat test ------------------------------------------------------------------
__global__ void k_assign_inv_scatter(const uint32_t* __restrict__ list, uint64_t n, uint32_t* __restrict__ inv) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n; k += gridDim.x * 256ull) inv[list[k]] = (uint32_t)k;      // a repeated index: any writer wins
}
__global__ void k_assign_inv_check(const uint32_t* __restrict__ list, uint64_t n, const uint32_t* __restrict__ inv, uint32_t* __restrict__ repeat) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n; k += gridDim.x * 256ull) if (inv[list[k]] != (uint32_t)k) *repeat = 1u;      // (every writer stores the same value)
}

// ---- relocate -----------------------------------------------------------------------------------------------------------
__global__ void k_assign_rowlen(DIdx I, uint64_t ar, const uint32_t* __restrict__ arp, uint32_t* __restrict__ len) {
  for (uint64_t a = blockIdx.x * 256ull + threadIdx.x; a < ar; a += gridDim.x * 256ull) len[idx_at(I, a)] = arp[a + 1] - arp[a];
}
template <int TS>
__global__ void k_assign_move(uint64_t nnz, const uint32_t* __restrict__ rowidx, const uint32_t* __restrict__ arp, const uint32_t* __restrict__ acol, const uint8_t* __restrict__ aval, DIdx I, DIdx J,
                              const uint32_t* __restrict__ trp, uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t p = blockIdx.x * 256ull + threadIdx.x; p < nnz; p += gridDim.x * 256ull) {
    const uint32_t a = rowidx[p];
    const uint64_t dst = (uint64_t)trp[idx_at(I, a)] + (p - arp[a]);
    ocol[dst] = idx_at(J, acol[p]); ((W*)oval)[dst] = ((const W*)aval)[p];
  }
}

// ---- the region of C ----------------------------------------------------------------------------------------------------
__global__ void k_assign_region_keep(uint64_t nnz, const uint32_t* __restrict__ rowidx, const uint32_t* __restrict__ col, DIdx I, DIdx J, uint8_t* __restrict__ keep) {
  for (uint64_t p = blockIdx.x * 256ull + threadIdx.x; p < nnz; p += gridDim.x * 256ull)
    keep[p] = (idx_inv(I, rowidx[p]) != NONE && idx_inv(J, col[p]) != NONE) ? 0 : 1;
}

// ---- w<allow, replace>(I) = accum(w(I), u): one pass over the n positions of w --------------------------------------------
template <class T, bool MATH>
__global__ void k_assign_vector(uint64_t n, T* __restrict__ wval, uint8_t* __restrict__ wpres, const uint8_t* __restrict__ allow, DIdx I, const T* __restrict__ uval, const uint8_t* __restrict__ upres,
                                int accum, bool replace) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const bool ok = allow ? allow[i] != 0 : true;
    if (ok) {
      const uint32_t k = idx_inv(I, (uint32_t)i);
      if (k == NONE) continue;                                               // outside the region: Z == w there
      const bool up = upres[k] != 0;
      if (accum >= 0) {
        if (up) {
          if (wpres[i]) wval[i] = apply_binop<T, true, MATH>(accum, wval[i], uval[k]);
          else { wval[i] = uval[k]; wpres[i] = 1; }
        }
      } else {
        if (up) wval[i] = uval[k];
        wpres[i] = up ? 1 : 0;
      }
    } else if (replace) {
      wpres[i] = 0;
    }
  }
}

template <class D, class S>
__global__ void k_assign_cast_touched(uint64_t n, D* __restrict__ dst, const S* __restrict__ src, const uint8_t* __restrict__ allow, DIdx I, const uint8_t* __restrict__ upres) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    if (allow && !allow[i]) continue;
    const uint32_t k = idx_inv(I, (uint32_t)i);
    if (k != NONE && upres[k]) dst[i] = cast_to<D, S>(src[i]);
  }
}

// ---- a bitmap as a CSR of one row or one column ------------------------------------------------------------------------------
__global__ void k_assign_two(uint32_t* p, uint32_t total) { if (threadIdx.x == 0 && blockIdx.x == 0) { p[0] = 0; p[1] = total; } }

}  // namespace

bool assign_inverse(const ExIdx& x, uint64_t dim, DevBuf& inv) {
  if (x.kind != EX_LIST) return true;
  if (dim > ASSIGN_TABLE_MAX_DIM) return false;
  inv.alloc((dim + 1) * 4);                                                  // [dim]: the repeat flag
  GRB_HIP(hipMemsetAsync(inv.p, 0xFF, dim * 4, stream()));
  GRB_HIP(hipMemsetAsync(inv.as<uint32_t>() + dim, 0, 4, stream()));
  if (!x.n) return true;
  hipLaunchKernelGGL(k_assign_inv_scatter, dim3(grid_1d(x.n)), dim3(256), 0, stream(), x.list, x.n, inv.as<uint32_t>());
  hipLaunchKernelGGL(k_assign_inv_check, dim3(grid_1d(x.n)), dim3(256), 0, stream(), x.list, x.n, inv.as<uint32_t>(), inv.as<uint32_t>() + dim);
  uint32_t repeat = 0;
  GRB_HIP(hipMemcpyAsync(&repeat, inv.as<uint32_t>() + dim, 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  return repeat == 0;
}

void assign_relocate(const DevCSR& A, size_t ts, const ExIdx& I, const ExIdx& J, uint32_t crows, uint32_t ccols, DevCSR& T, AssignPlan& plan) {
  check_value_size(ts, "assign");
  if (A.nrows != I.n || A.ncols != J.n) fail(GrB_PANIC, "assign: operand shape does not match the index arguments");      // (the entry points checked it: the kernels' bounds depend on it)
  const uint64_t nnz = A.nnz;
  T.clear(); T.nrows = crows; T.ncols = ccols; T.nnz = nnz;
  T.rowptr.alloc(((size_t)crows + 1) * 4); T.col.alloc(nnz * 4 + 4); T.val.alloc(nnz * ts + 8);
  plan.rowsort = false;
  if (!nnz) { GRB_HIP(hipMemsetAsync(T.rowptr.p, 0, ((size_t)crows + 1) * 4, stream())); T.valid = true; return; }
  const DIdx di = didx(I), dj = didx(J);
  DevBuf len(((size_t)crows + 1) * 4), rowidx(nnz * 4 + 4);
  GRB_HIP(hipMemsetAsync(len.p, 0, ((size_t)crows + 1) * 4, stream()));
  hipLaunchKernelGGL(k_assign_rowlen, dim3(grid_1d(I.n)), dim3(256), 0, stream(), di, I.n, A.rowptr.as<uint32_t>(), len.as<uint32_t>());
  exclusive_scan_u32(len.as<uint32_t>(), T.rowptr.as<uint32_t>(), (uint64_t)crows + 1);
  csr_row_indices(A, rowidx.as<uint32_t>());
  const bool rowsort = !J.increasing && J.n > 1;
  DevBuf ucol, uval;                                                         // unsorted columns / values when the rows are sorted afterwards
  if (rowsort) { ucol.alloc(nnz * 4); uval.alloc(nnz * ts); }
  uint32_t* oc = rowsort ? ucol.as<uint32_t>() : T.col.as<uint32_t>(); uint8_t* ov = rowsort ? uval.as<uint8_t>() : T.val.as<uint8_t>();
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_assign_move<TS>), dim3(grid_1d(nnz)), dim3(256), 0, stream(), nnz, rowidx.as<uint32_t>(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), A.val.as<uint8_t>(), di, dj,
                       T.rowptr.as<uint32_t>(), oc, ov);
  });
  if (rowsort) csr_sort_rows(T, ts, ucol, uval, ccols);
  GRB_HIP(hipStreamSynchronize(stream()));                                   // temporaries are released on scope exit; the pool is stream-ordered
  plan.rowsort = rowsort;
  T.valid = true;
}

void assign_region_keep(const DevCSR& C, const ExIdx& I, const DevBuf& inv_i, const ExIdx& J, const DevBuf& inv_j, uint8_t* keep) {
  if (!C.nnz) return;
  DevBuf rowidx(C.nnz * 4 + 4);
  csr_row_indices(C, rowidx.as<uint32_t>());
  hipLaunchKernelGGL(k_assign_region_keep, dim3(grid_1d(C.nnz)), dim3(256), 0, stream(), C.nnz, rowidx.as<uint32_t>(), C.col.as<uint32_t>(), didx(I, &inv_i), didx(J, &inv_j), keep);
  GRB_HIP(hipStreamSynchronize(stream()));
}

void assign_vector(int code, uint64_t n, void* wval, uint8_t* wpres, const uint8_t* allow, const ExIdx& I, const DevBuf& inv, const void* uval, const uint8_t* upres, int accum, bool replace) {
  if (!n) return;
  const DIdx di = didx(I, &inv);
  dispatch_type(code, [&]<class T>() {
    if (accum >= 0 && binop_needs_math(accum)) hipLaunchKernelGGL((k_assign_vector<T, true>), dim3(grid_1d(n)), dim3(256), 0, stream(), n, (T*)wval, wpres, allow, di, (const T*)uval, upres, accum, replace);
    else hipLaunchKernelGGL((k_assign_vector<T, false>), dim3(grid_1d(n)), dim3(256), 0, stream(), n, (T*)wval, wpres, allow, di, (const T*)uval, upres, accum, replace);
  });
}

void assign_cast_touched(int dst_code, void* dst, int src_code, const void* src, uint64_t n, const uint8_t* allow, const ExIdx& I, const DevBuf& inv, const uint8_t* upres) {
  if (!n) return;
  const DIdx di = didx(I, &inv);
  dispatch_type(src_code, [&]<class S>() {
    dispatch_type(dst_code, [&]<class D>() {
      hipLaunchKernelGGL((k_assign_cast_touched<D, S>), dim3(grid_1d(n)), dim3(256), 0, stream(), n, (D*)dst, (const S*)src, allow, di, upres);
    });
  });
}

void assign_line_to_csr(size_t ts, uint64_t n, const void* lval, const uint8_t* lpres, bool as_row, DevCSR& T) {
  check_value_size(ts, "assign");
  T.clear(); T.nrows = as_row ? 1u : (uint32_t)n; T.ncols = as_row ? (uint32_t)n : 1u;
  DevBuf pos_buf;
  // a column's entry positions ARE its row pointer: the scan goes straight into it
  if (as_row) { pos_buf.alloc((n + 1) * 4); T.rowptr.alloc(8); } else T.rowptr.alloc((n + 1) * 4);
  uint32_t* pos = as_row ? pos_buf.as<uint32_t>() : T.rowptr.as<uint32_t>();
  const uint32_t total = present_positions_total(lpres, n, pos);
  T.nnz = total; T.col.alloc((size_t)total * 4 + 4); T.val.alloc((size_t)total * ts + 8);
  if (as_row) hipLaunchKernelGGL(k_assign_two, dim3(1), dim3(64), 0, stream(), T.rowptr.as<uint32_t>(), total);
  if (total) scatter_present(lpres, pos, n, 0, as_row ? COMPACT_COL_INDEX : COMPACT_COL_ZERO, 0, T.col.as<uint32_t>(), ts, lval, T.val.p);
  GRB_HIP(hipStreamSynchronize(stream()));
  T.valid = true;
}

}  // namespace grb
