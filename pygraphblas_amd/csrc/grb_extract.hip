// grb_extract.hip — index-list extract in HBM: T = A(I, J) (CSR in, CSR out), one row / column of a CSR as a bitmap vector, u(I) on bitmaps.
//
// Index arguments arrive as ExIdx (grb_extract.hpp): GrB_ALL and the GxB_RANGE / GxB_STRIDE / GxB_BACKWARDS triples are evaluated in closed form by the
// kernels, only an explicit list is uploaded (once per call, 4 bytes per index).
//
// T = A(I, J):
//   rows     output row k is source row I[k] (any order, repeats allowed).  The selected rows are cut into PARTS of <= 2048 entries, one wave per part (the
//            row-block idea of k_spmv_adaptive: a hub row of 10^5 entries becomes 50 parts, an ordinary row is one part); the parts are numbered row by
//            row, so an exclusive scan over the parts' hit counts is at once every part's output offset and — at a row's first part — the row pointer.
//   columns  a source column c maps to output columns
//              all     c
//              range   (c - lo) / step, or (lo - c) / step for a descending range: a compare, a subtract and a divide
//              table   perm[first[c] .. first[c + 1]): (J[k], k) sorted by J once (rocPRIM radix sort, stable), `first` = ncols + 1 offsets into the sorted list
//              bisect  the same range found by two bisections of the sorted list (operands wider than EXTRACT_TABLE_MAX_COLS columns, or on request)
//            A strictly increasing list is its own sorted list and perm is the identity (not stored).
//   passes   count (hits per part) -> exclusive scan -> fill (column, value): one kernel body, template flag.  The fill is stable within a row (a wave walks
//            its part in 64-entry chunks, hit positions by ballot / prefix), so for increasing J the output row is sorted as it is written.  Otherwise
//            each output row is sorted by column afterwards (rocPRIM segmented radix sort on (column, position), then one gather of the values).
//   traffic  2 x (4 + ts) bytes per entry of the selected rows read (column twice, value once in the fill: (8 + ts)), (4 + ts) per output entry written.
// No atomics anywhere: every output position has exactly one writer.
#include "grb_index.hpp"
#include "grb_matops.hpp"

namespace grb {
namespace {

constexpr uint32_t PART = 2048;        // entries per part (one wave)
constexpr int WAVES = 4;               // waves per workgroup

// column map on the device
enum { CM_ALL = 0, CM_RANGE = 1, CM_TABLE = 2, CM_BISECT = 3 };
struct DCols {
  int mode; bool desc, multi;            // desc: descending range; multi: a source column may have several hits (repeats in J)
  uint32_t lo, step, n;                  // range: n positions; list modes: n = length of the sorted list
  const uint32_t* sorted; const uint32_t* perm; const uint32_t* first;      // perm == nullptr: identity
};
// hits of source column c: positions [h0, h0 + nh) of the sorted list (list modes), or the output column h0 itself (all / range)
__device__ __forceinline__ void col_hits(const DCols& J, uint32_t c, uint32_t& h0, uint32_t& nh) {
  switch (J.mode) {
    case CM_ALL: h0 = c; nh = 1; return;
    case CM_RANGE: h0 = range_inv(J.desc, J.lo, J.step, J.n, c); nh = h0 != NONE ? 1u : 0u; return;
    case CM_TABLE: h0 = J.first[c]; nh = J.first[c + 1] - h0; return;
    default: {
      h0 = lower_bound_u32(J.sorted, J.n, c);
      if (J.multi) nh = (c == 0xFFFFFFFFu ? J.n : lower_bound_u32(J.sorted, J.n, c + 1)) - h0;
      else nh = (h0 < J.n && J.sorted[h0] == c) ? 1u : 0u;
      return;
    }
  }
}

// parts of every selected row: max(1, ceil(len / PART)); position nout holds 0 so that the scan's last element is the total
__global__ void k_extract_nparts(DIdx I, uint64_t nout, const uint32_t* __restrict__ rowptr, uint32_t* __restrict__ nparts) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k <= nout; k += gridDim.x * 256ull) {
    if (k == nout) { nparts[k] = 0; continue; }
    const uint32_t r = idx_at(I, k), len = rowptr[r + 1] - rowptr[r];
    nparts[k] = len <= PART ? 1u : (len + PART - 1) / PART;
  }
}
__global__ void k_extract_partmap(uint64_t nout, const uint32_t* __restrict__ partstart, uint32_t* __restrict__ part_row) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < nout; k += gridDim.x * 256ull)
    for (uint32_t p = partstart[k]; p < partstart[k + 1]; p++) part_row[p] = (uint32_t)k;
}

// One wave per part.  FILL == false: partcount[p] = hits of the part.  FILL == true: the hits are written from partoff[p] on, in the part's own order.
// part_row == nullptr: no row has more than one part (part p is output row p).
template <bool FILL, int TS>
__global__ void __launch_bounds__(64 * WAVES) k_extract_rows(DIdx I, DCols J, uint64_t nparts, const uint32_t* __restrict__ part_row, const uint32_t* __restrict__ partstart,
                                                             const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                             uint64_t* __restrict__ partcount, const uint64_t* __restrict__ partoff, uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval) {
  typedef typename WordOf<TS>::type W;
  const int lane = threadIdx.x & 63;
  const uint64_t p = blockIdx.x * (uint64_t)WAVES + (threadIdx.x >> 6);
  if (p >= nparts) return;                                                   // (whole wave)
  const uint32_t k = part_row ? part_row[p] : (uint32_t)p;
  const uint32_t r = idx_at(I, k);
  const uint32_t piece = part_row ? (uint32_t)p - partstart[k] : 0u;
  const uint64_t rb = rowptr[r], re = rowptr[r + 1];
  const uint64_t b = rb + (uint64_t)piece * PART, e = (re - b > PART) ? b + PART : re;
  uint64_t out = FILL ? partoff[p] : 0;
  for (uint64_t base = b; base < e; base += 64) {
    const uint64_t q = base + lane;
    uint32_t h0 = 0, nh = 0;
    if (q < e) col_hits(J, col[q], h0, nh);
    uint32_t before, total;                                                  // hits in the lanes below, hits of the chunk
    if (!J.multi) {
      const unsigned long long m = __ballot(nh != 0);
      before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); total = (uint32_t)__popcll(m);
    } else {
      uint32_t s = nh;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)s, d, 64); if (lane >= d) s += t; }
      before = s - nh; total = (uint32_t)__shfl((int)s, 63, 64);
    }
    if constexpr (FILL) {
      if (nh) {
        const W v = ((const W*)val)[q];
        const uint64_t o = out + before;
        for (uint32_t t = 0; t < nh; t++) { ocol[o + t] = J.perm ? J.perm[h0 + t] : h0 + t; ((W*)oval)[o + t] = v; }
      }
    }
    out += total;
  }
  if constexpr (!FILL) { if (lane == 0) partcount[p] = out; }
}

// row pointers of T from the parts' offsets: a row starts where its first part does
__global__ void k_extract_rowptr(uint64_t nout, const uint32_t* __restrict__ partstart, bool identity, const uint64_t* __restrict__ partoff, uint64_t total, uint32_t* __restrict__ orowptr) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k <= nout; k += gridDim.x * 256ull)
    orowptr[k] = k == nout ? (uint32_t)total : (uint32_t)partoff[identity ? k : partstart[k]];
}
// first[c] = position of the first element >= c of the sorted list, c = 0 .. ncols: one bisection per column (no thread depends on the gaps of the list)
__global__ void k_extract_first(const uint32_t* __restrict__ sorted, uint64_t n, uint32_t ncols, uint32_t* __restrict__ first) {
  for (uint64_t c = blockIdx.x * 256ull + threadIdx.x; c <= ncols; c += gridDim.x * 256ull) first[c] = lower_bound_u32(sorted, (uint32_t)n, (uint32_t)c);
}

// ---- one row / column of a CSR, a sub-vector ---------------------------------------------------------------------------
// row j of the CSR onto every position (I = ALL): the row's entries scattered into a zeroed bitmap
template <int TS> __global__ void k_extract_row_scatter(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint8_t* __restrict__ val, uint32_t j, uint8_t* __restrict__ tval, uint8_t* __restrict__ tpres) {
  typedef typename WordOf<TS>::type W;
  const uint64_t b = rowptr[j], e = rowptr[j + 1];
  for (uint64_t p = b + blockIdx.x * 256ull + threadIdx.x; p < e; p += gridDim.x * 256ull) { const uint32_t c = col[p]; ((W*)tval)[c] = ((const W*)val)[p]; tpres[c] = 1; }
}
// t(k) = A(j, I[k]) (row_of_csr) or A(I[k], j): one thread per k, bisection inside the row
template <int TS> __global__ void k_extract_lookup(DIdx I, uint64_t n, bool row_of_csr, uint32_t j, const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                   uint8_t* __restrict__ tval, uint8_t* __restrict__ tpres) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n; k += gridDim.x * 256ull) {
    const uint32_t x = idx_at(I, k), r = row_of_csr ? j : x, c = row_of_csr ? x : j;
    const uint32_t b = rowptr[r], len = rowptr[r + 1] - b;
    const uint32_t pos = lower_bound_u32(col + b, len, c);
    const bool hit = pos < len && col[b + pos] == c;
    ((W*)tval)[k] = hit ? ((const W*)val)[b + pos] : (W)0; tpres[k] = hit ? 1 : 0;
  }
}
template <int TS> __global__ void k_extract_vector(DIdx I, uint64_t n, const uint8_t* __restrict__ uval, const uint8_t* __restrict__ upres, uint8_t* __restrict__ tval, uint8_t* __restrict__ tpres) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n; k += gridDim.x * 256ull) {
    const uint32_t s = idx_at(I, k); const uint8_t pr = upres[s];
    ((W*)tval)[k] = pr ? ((const W*)uval)[s] : (W)0; tpres[k] = pr ? 1 : 0;
  }
}

}  // namespace

void extract_upload(ExIdx& x, DevBuf& keep) {
  if (x.kind != EX_LIST || x.host.empty()) return;
  keep.alloc(x.host.size() * 4);
  GRB_HIP(hipMemcpyAsync(keep.p, x.host.data(), x.host.size() * 4, hipMemcpyHostToDevice, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));                                   // (the staging vector may go away before the kernels ran)
  x.list = keep.as<uint32_t>();
}

void extract_csr(const DevCSR& A, size_t ts, const ExIdx& I, const ExIdx& J, bool force_bisect, DevCSR& T, ExtractPlan& plan) {
  check_value_size(ts, "extract");
  const uint64_t nout = I.n, ncout = J.n;
  T.clear(); T.nrows = (uint32_t)nout; T.ncols = (uint32_t)ncout; T.nnz = 0;
  T.rowptr.alloc((nout + 1) * 4);
  plan.rowsort = false; plan.src_entries = 0;
  if (nout == 0 || ncout == 0 || A.nnz == 0) {                               // nothing can be selected
    plan.cols = J.kind == EX_ALL ? "all" : (J.kind == EX_LIST ? "table" : "range");
    GRB_HIP(hipMemsetAsync(T.rowptr.p, 0, (nout + 1) * 4, stream())); T.valid = true; return;
  }
  // ---- the column map ----
  DCols dj{}; dj.lo = J.lo; dj.step = J.step; dj.n = (uint32_t)ncout; dj.desc = false; dj.multi = false;
  DevBuf sorted_buf, perm_buf, first_buf;
  bool rowsort = false;
  if (J.kind == EX_ALL) { dj.mode = CM_ALL; plan.cols = "all"; }
  else if (J.kind != EX_LIST) { dj.mode = CM_RANGE; dj.desc = J.kind == EX_BACK; rowsort = dj.desc; plan.cols = "range"; }
  else {
    if (J.increasing) dj.sorted = J.list;                                    // its own sorted list, perm = identity
    else {
      DevBuf iota(ncout * 4); sorted_buf.alloc(ncout * 4); perm_buf.alloc(ncout * 4);
      fill_iota_u32(iota.as<uint32_t>(), ncout);
      int bits = 1; while (bits < 32 && (1ull << bits) < (uint64_t)A.ncols) bits++;
      sort_pairs_u32(J.list, sorted_buf.as<uint32_t>(), iota.as<uint32_t>(), perm_buf.as<uint32_t>(), ncout, bits);
      GRB_HIP(hipStreamSynchronize(stream()));                               // (iota returns to the pool)
      dj.sorted = sorted_buf.as<uint32_t>(); dj.perm = perm_buf.as<uint32_t>(); dj.multi = true; rowsort = true;
    }
    if (!force_bisect && (uint64_t)A.ncols + 1 <= EXTRACT_TABLE_MAX_COLS) {
      first_buf.alloc(((size_t)A.ncols + 1) * 4);
      hipLaunchKernelGGL(k_extract_first, dim3(grid_1d((uint64_t)A.ncols + 1)), dim3(256), 0, stream(), dj.sorted, ncout, A.ncols, first_buf.as<uint32_t>());
      dj.first = first_buf.as<uint32_t>(); dj.mode = CM_TABLE; plan.cols = "table";
    } else { dj.mode = CM_BISECT; plan.cols = "bisect"; }
  }
  // ---- parts ----
  const DIdx di = didx(I);
  DevBuf nparts_buf((nout + 1) * 4), partstart((nout + 1) * 4), part_row;
  hipLaunchKernelGGL(k_extract_nparts, dim3(grid_1d(nout + 1)), dim3(256), 0, stream(), di, nout, A.rowptr.as<uint32_t>(), nparts_buf.as<uint32_t>());
  exclusive_scan_u32(nparts_buf.as<uint32_t>(), partstart.as<uint32_t>(), nout + 1);
  uint32_t nparts32 = 0;
  GRB_HIP(hipMemcpyAsync(&nparts32, partstart.as<uint32_t>() + nout, 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  const uint64_t nparts = nparts32;
  if (nparts < nout) fail(GrB_INSUFFICIENT_SPACE, "extract: more than 2^32 parts of rows");
  const bool identity = nparts == nout;
  if (!identity) { part_row.alloc(nparts * 4); hipLaunchKernelGGL(k_extract_partmap, dim3(grid_1d(nout)), dim3(256), 0, stream(), nout, partstart.as<uint32_t>(), part_row.as<uint32_t>()); }
  // ---- count -> scan -> fill ----
  DevBuf partcount((nparts + 1) * 8), partoff((nparts + 1) * 8);
  GRB_HIP(hipMemsetAsync((uint8_t*)partcount.p + nparts * 8, 0, 8, stream()));
  const dim3 grid((unsigned)((nparts + WAVES - 1) / WAVES)), block(64 * WAVES);
  hipLaunchKernelGGL((k_extract_rows<false, 1>), grid, block, 0, stream(), di, dj, nparts, part_row.as<uint32_t>(), partstart.as<uint32_t>(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(),
                     (const uint8_t*)nullptr, partcount.as<uint64_t>(), (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint8_t*)nullptr);
  exclusive_scan_u64(partcount.as<uint64_t>(), partoff.as<uint64_t>(), nparts + 1);
  uint64_t total = 0;
  GRB_HIP(hipMemcpyAsync(&total, partoff.as<uint64_t>() + nparts, 8, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  if (total > 0xFFFFFFF0ull) fail(GrB_INSUFFICIENT_SPACE, "extract: more than 2^32 entries in the result");
  hipLaunchKernelGGL(k_extract_rowptr, dim3(grid_1d(nout + 1)), dim3(256), 0, stream(), nout, partstart.as<uint32_t>(), identity, partoff.as<uint64_t>(), total, T.rowptr.as<uint32_t>());
  T.nnz = total; T.col.alloc(total * 4 + 4); T.val.alloc(total * ts + 8);
  if (total) {
    rowsort = rowsort && ncout > 1;
    DevBuf ucol, uval;                                                       // unsorted columns / values when the rows are sorted afterwards
    if (rowsort) { ucol.alloc(total * 4); uval.alloc(total * ts); }
    uint32_t* oc = rowsort ? ucol.as<uint32_t>() : T.col.as<uint32_t>(); uint8_t* ov = rowsort ? uval.as<uint8_t>() : T.val.as<uint8_t>();
    dispatch_value_size(ts, [&]<int TS>() {
      hipLaunchKernelGGL((k_extract_rows<true, TS>), grid, block, 0, stream(), di, dj, nparts, part_row.as<uint32_t>(), partstart.as<uint32_t>(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(),
                         A.val.as<uint8_t>(), (uint64_t*)nullptr, partoff.as<uint64_t>(), oc, ov);
    });
    if (rowsort) csr_sort_rows(T, ts, ucol, uval, ncout);
  }
  GRB_HIP(hipStreamSynchronize(stream()));                                   // temporaries are released on scope exit; the pool is stream-ordered
  plan.rowsort = rowsort && total != 0;
  T.valid = true;
}

void extract_line(const DevCSR& A, size_t ts, bool row_of_csr, uint32_t j, const ExIdx& I, void* tval, uint8_t* tpres) {
  check_value_size(ts, "extract");
  const uint64_t n = I.n; if (!n) return;
  if (row_of_csr && I.kind == EX_ALL) {
    GRB_HIP(hipMemsetAsync(tval, 0, n * ts, stream())); GRB_HIP(hipMemsetAsync(tpres, 0, n, stream()));
    if (A.nnz) dispatch_value_size(ts, [&]<int TS>() { hipLaunchKernelGGL((k_extract_row_scatter<TS>), dim3(64), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), A.val.as<uint8_t>(), j, (uint8_t*)tval, tpres); });
    return;
  }
  if (!A.nnz) { GRB_HIP(hipMemsetAsync(tval, 0, n * ts, stream())); GRB_HIP(hipMemsetAsync(tpres, 0, n, stream())); return; }
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_extract_lookup<TS>), dim3(grid_1d(n)), dim3(256), 0, stream(), didx(I), n, row_of_csr, j, A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), A.val.as<uint8_t>(), (uint8_t*)tval, tpres);
  });
}

void extract_vector(size_t ts, const void* uval, const uint8_t* upres, const ExIdx& I, void* tval, uint8_t* tpres) {
  check_value_size(ts, "extract");
  const uint64_t n = I.n; if (!n) return;
  dispatch_value_size(ts, [&]<int TS>() { hipLaunchKernelGGL((k_extract_vector<TS>), dim3(grid_1d(n)), dim3(256), 0, stream(), didx(I), n, (const uint8_t*)uval, upres, (uint8_t*)tval, tpres); });
}

}  // namespace grb
