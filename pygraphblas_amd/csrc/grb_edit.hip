// grb_edit.hip — element edits applied to a container in HBM (the flush of the edit queue, grb_edit_ops.cpp), and the pieces of a resize that stays there.
// The list arithmetic (classes, prefix arrays, destinations) is grb_edit_list.hpp's, shared with the host check of tests/edit_list_check.cpp.
//
//   csr_apply_edits   k edits in (row, column) order, one per coordinate.
//     k_edit_locate     a lane owns an edit: it bisects the edit's row for the column and stores pos[e] — the position of the first stored entry whose coordinate
//                       is not below the edit's — and its class (overwrite / insert / delete / nothing).  The k class bytes are the one read-back.
//     k_edit_values     no insert, no delete: the overwrites store their values in place.  Nothing else runs.
//     k_edit_rowptr     a lane owns a row r: new rowptr[r] = old + inserts - deletes among the edits of the rows before r (a bisection of the edits' rows into
//                       the two prefix arrays the host made from the classes).
//     k_edit_stream     ENTRY-PARALLEL, 256 threads, a lane owns EDIT_EPL = 4 consecutive stored entries (grb_userop's geometry): one bisection of pos[] for the
//                       first of them, a linear step for the others, and every surviving entry goes to p + inserts before it - deletes before it.  No sort of
//                       the matrix, no atomics, every output position has one writer.  A whole group leaves the aligned arrays as 16-byte loads; where none of
//                       its entries goes, the shift is one for all four and the destination is aligned as well, it is stored as packs too (an edit list is
//                       short: nearly every group).  Other groups and the last partial one go entry by entry.
//     k_edit_place      the edit lanes again, after the stream pass: an insert stores its column and value at pos + shift, an overwrite its value.
//   the edit table      four arrays by edit (pos u32, class u8, the prefixes u32 x 2 of k + 1 words), not records: the bisection touches pos[] alone, whose
//                       probes of neighbouring lanes fall into the same few cache lines (the first levels are the same words for the whole wave).  It stays
//                       in global memory — the L2 holds it; staging k words per workgroup into LDS would cost more than the 12 probes of a 4 096-edit list, and
//                       a bisection out of LDS has every lane on its own bank row.
//   traffic (structural)  read nnz (4 + ts), written nnz' (4 + ts) + 4 (nrows + 1), plus O(k log) for the edits.
//
//   vec_apply_edits   k_edit_vector: a lane owns an edit — value and presence byte stored, or presence 0 for a remove.
// Values move as words of their size (1, 2, 4, 8 bytes), never by type.
#include "grb_edit.hpp"
#include "grb_edit_list.hpp"
#include "grb_index.hpp"

namespace grb {
namespace {

constexpr int EDIT_EPL = 4;                                                  // stored entries per lane of the stream pass: 16 bytes of columns

template <int TS> struct alignas(TS * EDIT_EPL > 16 ? 16 : TS * EDIT_EPL) ValPack { typename WordOf<TS>::type v[EDIT_EPL]; };
struct alignas(16) U32Pack { uint32_t c[EDIT_EPL]; };

__global__ __launch_bounds__(256) void k_edit_locate(uint32_t k, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej, const uint8_t* __restrict__ del,
                                                     const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, uint32_t* __restrict__ pos, uint8_t* __restrict__ cls) {
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < k; e += gridDim.x * 256u) {
    const uint32_t i = ei[e], j = ej[e];                                     // (i < nrows: checked on the host)
    const uint32_t lo = rowptr[i], hi = rowptr[i + 1];
    const uint32_t q = lo + lower_bound_u32(col + lo, hi - lo, j);           // (an empty row reads nothing)
    const bool stored = q < hi && col[q] == j;
    pos[e] = q; cls[e] = edit_classify(stored, del[e] != 0);
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_edit_values(uint32_t k, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ cls, const uint8_t* __restrict__ x, uint8_t* __restrict__ val) {
  typedef typename WordOf<TS>::type W;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < k; e += gridDim.x * 256u)
    if (cls[e] == EDIT_OVERWRITE) ((W*)val)[pos[e]] = ((const W*)x)[e];
}

__global__ __launch_bounds__(256) void k_edit_rowptr(uint32_t nrows, const uint32_t* __restrict__ rowptr, uint32_t k, const uint32_t* __restrict__ ei,
                                                     const uint32_t* __restrict__ insb, const uint32_t* __restrict__ delb, uint32_t* __restrict__ out) {
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows; r += gridDim.x * 256ull) {
    const uint32_t m = lower_bound_u32(ei, k, (uint32_t)r);                  // edits in the rows before r
    out[r] = rowptr[r] + insb[m] - delb[m];
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_edit_stream(uint64_t nnz, const uint32_t* __restrict__ col, const uint8_t* __restrict__ val, uint32_t k, const uint32_t* __restrict__ pos,
                                                     const uint8_t* __restrict__ cls, const uint32_t* __restrict__ insb, const uint32_t* __restrict__ delb,
                                                     uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval, int packed) {
  typedef typename WordOf<TS>::type W;
  const W* __restrict__ src = (const W*)val; W* __restrict__ dst = (W*)oval;
  const uint64_t ngroups = (nnz + EDIT_EPL - 1) / EDIT_EPL;
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < ngroups; g += gridDim.x * 256ull) {
    const uint64_t p0 = g * EDIT_EPL;
    const int nv = nnz - p0 >= (uint64_t)EDIT_EPL ? EDIT_EPL : (int)(nnz - p0);
    const bool whole = nv == EDIT_EPL && packed;
    U32Pack c; ValPack<TS> v;
    if (whole) { c = *reinterpret_cast<const U32Pack*>(col + p0); v = *reinterpret_cast<const ValPack<TS>*>(src + p0); }
    else for (int j = 0; j < nv; j++) { c.c[j] = col[p0 + j]; v.v[j] = src[p0 + j]; }
    uint32_t t = edit_upper_bound(pos, k, (uint32_t)p0);
    uint32_t d[EDIT_EPL]; bool keep[EDIT_EPL]; bool run = whole;             // run: all four stay, at consecutive places
#pragma unroll
    for (int j = 0; j < EDIT_EPL; j++) {
      keep[j] = false; d[j] = 0;
      if (j < nv) {
        const uint32_t p = (uint32_t)p0 + j;
        if (j) while (t < k && pos[t] <= p) t++;
        keep[j] = edit_dest_at(pos, cls, insb, delb, t, p, &d[j]);
      }
      run = run && keep[j] && d[j] == d[0] + j;
    }
    if (run && (d[0] & (EDIT_EPL - 1)) == 0) {
      *reinterpret_cast<U32Pack*>(ocol + d[0]) = c;
      *reinterpret_cast<ValPack<TS>*>(dst + d[0]) = v;
    } else {
#pragma unroll
      for (int j = 0; j < EDIT_EPL; j++) if (keep[j]) { ocol[d[j]] = c.c[j]; dst[d[j]] = v.v[j]; }
    }
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_edit_place(uint32_t k, const uint32_t* __restrict__ ej, const uint8_t* __restrict__ x, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ cls,
                                                    const uint32_t* __restrict__ insb, const uint32_t* __restrict__ delb, uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval) {
  typedef typename WordOf<TS>::type W;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < k; e += gridDim.x * 256u) {
    const uint8_t c = cls[e];
    if (c != EDIT_INSERT && c != EDIT_OVERWRITE) continue;
    const uint32_t d = edit_own_dest(pos, insb, delb, e);
    if (c == EDIT_INSERT) ocol[d] = ej[e];
    ((W*)oval)[d] = ((const W*)x)[e];
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_edit_vector(uint32_t k, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ del, const uint8_t* __restrict__ x, uint8_t* __restrict__ val, uint8_t* __restrict__ pres) {
  typedef typename WordOf<TS>::type W;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < k; e += gridDim.x * 256u) {
    const uint32_t i = idx[e];                                               // (i < n: checked on the host)
    if (del[e]) pres[i] = 0;
    else { ((W*)val)[i] = ((const W*)x)[e]; pres[i] = 1; }
  }
}

__global__ __launch_bounds__(256) void k_keep_cols_below(uint64_t nnz, const uint32_t* __restrict__ col, uint32_t ncols, uint8_t* __restrict__ keep) {
  for (uint64_t p = blockIdx.x * 256ull + threadIdx.x; p < nnz; p += gridDim.x * 256ull) keep[p] = col[p] < ncols ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_resize_rowptr(const uint32_t* __restrict__ rowptr, uint32_t nrows_old, uint32_t nrows_new, uint32_t last, uint32_t* __restrict__ out) {
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows_new; r += gridDim.x * 256ull) out[r] = r <= nrows_old ? rowptr[r] : last;
}

inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

inline void upload(DevBuf& d, const void* src, size_t bytes) { d.alloc(bytes + 16); GRB_HIP(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, stream())); }

}  // namespace

EditCounts csr_apply_edits(const DevCSR& A, size_t ts, uint32_t k, const uint32_t* ei, const uint32_t* ej, const uint8_t* del, const uint8_t* x, DevCSR& out, bool* structural) {
  check_value_size(ts, "edit");
  EditCounts n; *structural = false;
  if (!k) return n;
  for (uint32_t e = 0; e < k; e++) {                                         // the kernels' bounds depend on it
    if (ei[e] >= A.nrows || ej[e] >= A.ncols) fail(GrB_PANIC, "edit: a queued coordinate lies outside the matrix");
    if (e && !(ei[e - 1] < ei[e] || (ei[e - 1] == ei[e] && ej[e - 1] < ej[e]))) fail(GrB_PANIC, "edit: the list is not normalised");
  }
  DevBuf dei, dej, ddel, dx, dpos((size_t)k * 4 + 16), dcls((size_t)k + 16);
  upload(dei, ei, (size_t)k * 4); upload(dej, ej, (size_t)k * 4); upload(ddel, del, k); upload(dx, x, (size_t)k * ts);
  hipLaunchKernelGGL(k_edit_locate, dim3(grid_1d(k)), dim3(256), 0, stream(), k, dei.as<uint32_t>(), dej.as<uint32_t>(), ddel.as<uint8_t>(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(),
                     dpos.as<uint32_t>(), dcls.as<uint8_t>());
  GRB_HIP(hipGetLastError());
  std::vector<uint8_t> cls(k);
  GRB_HIP(hipMemcpyAsync(cls.data(), dcls.p, k, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));      // the one read-back: k bytes
  for (uint32_t e = 0; e < k; e++) { n.set += cls[e] == EDIT_OVERWRITE; n.ins += cls[e] == EDIT_INSERT; n.del += cls[e] == EDIT_DELETE; }
  if (!n.ins && !n.del) {
    if (n.set) dispatch_value_size(ts, [&]<int TS>() {
      hipLaunchKernelGGL((k_edit_values<TS>), dim3(grid_1d(k)), dim3(256), 0, stream(), k, dpos.as<uint32_t>(), dcls.as<uint8_t>(), dx.as<uint8_t>(), A.val.as<uint8_t>());
    });
    GRB_HIP(hipGetLastError());
    GRB_HIP(hipStreamSynchronize(stream()));                                 // the staging buffers return to the pool
    return n;
  }
  const uint64_t nnz_new = A.nnz + n.ins - n.del;
  if (nnz_new > 0xFFFFFFF0ull) fail(GrB_INSUFFICIENT_SPACE, "more than 2^32 entries in one device matrix");
  std::vector<uint32_t> insb, delb; edit_prefixes(cls.data(), k, insb, delb);
  DevBuf dinsb, ddelb; upload(dinsb, insb.data(), insb.size() * 4); upload(ddelb, delb.data(), delb.size() * 4);
  out.clear(); out.nrows = A.nrows; out.ncols = A.ncols; out.nnz = nnz_new;
  out.rowptr.alloc(((size_t)A.nrows + 1) * 4); out.col.alloc(nnz_new * 4 + 16); out.val.alloc(nnz_new * ts + 16);
  hipLaunchKernelGGL(k_edit_rowptr, dim3(grid_1d((uint64_t)A.nrows + 1)), dim3(256), 0, stream(), A.nrows, A.rowptr.as<uint32_t>(), k, dei.as<uint32_t>(), dinsb.as<uint32_t>(), ddelb.as<uint32_t>(),
                     out.rowptr.as<uint32_t>());
  const size_t pa = ts * EDIT_EPL > 16 ? 16 : ts * EDIT_EPL;
  const int packed = aligned_to(A.col.p, 16) && aligned_to(out.col.p, 16) && aligned_to(A.val.p, pa) && aligned_to(out.val.p, pa) ? 1 : 0;
  dispatch_value_size(ts, [&]<int TS>() {
    if (A.nnz) hipLaunchKernelGGL((k_edit_stream<TS>), dim3(grid_1d((A.nnz + EDIT_EPL - 1) / EDIT_EPL)), dim3(256), 0, stream(), A.nnz, A.col.as<uint32_t>(), A.val.as<uint8_t>(), k, dpos.as<uint32_t>(),
                                  dcls.as<uint8_t>(), dinsb.as<uint32_t>(), ddelb.as<uint32_t>(), out.col.as<uint32_t>(), out.val.as<uint8_t>(), packed);
    hipLaunchKernelGGL((k_edit_place<TS>), dim3(grid_1d(k)), dim3(256), 0, stream(), k, dej.as<uint32_t>(), dx.as<uint8_t>(), dpos.as<uint32_t>(), dcls.as<uint8_t>(), dinsb.as<uint32_t>(), ddelb.as<uint32_t>(),
                       out.col.as<uint32_t>(), out.val.as<uint8_t>());
  });
  GRB_HIP(hipGetLastError());
  GRB_HIP(hipStreamSynchronize(stream()));                                   // the staging buffers and the host prefix arrays go out of scope
  out.valid = true; *structural = true;
  return n;
}

void vec_apply_edits(size_t ts, uint64_t n, uint32_t k, const uint32_t* idx, const uint8_t* del, const uint8_t* x, void* val, uint8_t* pres) {
  check_value_size(ts, "edit");
  if (!k) return;
  for (uint32_t e = 0; e < k; e++) {                                         // the kernel's bounds depend on it
    if (idx[e] >= n) fail(GrB_PANIC, "edit: a queued index lies outside the vector");
    if (e && idx[e - 1] >= idx[e]) fail(GrB_PANIC, "edit: the list is not normalised");
  }
  DevBuf di, ddel, dx;
  upload(di, idx, (size_t)k * 4); upload(ddel, del, k); upload(dx, x, (size_t)k * ts);
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_edit_vector<TS>), dim3(grid_1d(k)), dim3(256), 0, stream(), k, di.as<uint32_t>(), ddel.as<uint8_t>(), dx.as<uint8_t>(), (uint8_t*)val, pres);
  });
  GRB_HIP(hipGetLastError());
  GRB_HIP(hipStreamSynchronize(stream()));                                   // the staging buffers return to the pool
}

void csr_keep_cols_below(const DevCSR& A, uint32_t ncols, uint8_t* keep) {
  if (!A.nnz) return;
  hipLaunchKernelGGL(k_keep_cols_below, dim3(grid_1d(A.nnz)), dim3(256), 0, stream(), A.nnz, A.col.as<uint32_t>(), ncols, keep);
  GRB_HIP(hipGetLastError());
}

uint64_t csr_resize_rowptr(const DevCSR& A, uint32_t nrows_new, DevBuf& rowptr_new) {
  if (A.nnz > 0xFFFFFFF0ull) fail(GrB_PANIC, "resize: the entry count does not fit a row pointer");
  rowptr_new.alloc(((size_t)nrows_new + 1) * 4);
  hipLaunchKernelGGL(k_resize_rowptr, dim3(grid_1d((uint64_t)nrows_new + 1)), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), A.nrows, nrows_new, (uint32_t)A.nnz, rowptr_new.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  if (nrows_new >= A.nrows) return A.nnz;
  uint32_t* pin = (uint32_t*)pinned_scratch();
  GRB_HIP(hipMemcpyAsync(pin, rowptr_new.as<uint32_t>() + nrows_new, 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  return pin[0];
}

}  // namespace grb
