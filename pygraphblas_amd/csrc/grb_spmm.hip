// grb_spmm.hip — the product with a full right operand (grb_spmm.hpp): the pattern kernels, which move no values and need no type, and the driver.  The value
// kernels are grb_spmm_kernels.hpp, instantiated per type in grb_spmm_inst.hip.
//   k_spmm_rowflags    one thread per row of A: 1 / 0 words "the row holds an entry" and "the row is long" (the word behind the last row is 0: the scans' last
//                      words are the totals).
//   (scan)             exclusive_scan_u32 over each: the number of non-empty rows before a row — T's row pointer over k — and a row's rank among the long rows.
//                      Both totals reach the host in one copy: nvals(T), and whether the chunk pass runs at all.
//   k_full_pattern     T.rowptr and T.col in closed form (full_pattern_fill: GrBX_Matrix_import_Full shares it).
//   k_spmm_long_tasks  a wave per 64 rows: every long row writes its row number into the scratch slots of its chunks (the whole wave strides over one row's
//                      chunks: a hub row has thousands) and into the list of long rows.
// All kernels: wave64, 256 threads, a capped grid with a loop past the cap, plain vector stores, no LDS, no atomics.
#include "grb_spmm.hpp"
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_index.hpp"

namespace grb {
namespace {

__global__ __launch_bounds__(256) void k_spmm_rowflags(const uint32_t* __restrict__ arp, uint32_t m, uint32_t* __restrict__ nonempty, uint32_t* __restrict__ islong) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= m; i += gridDim.x * 256ull) {
    const uint32_t len = i < m ? arp[i + 1] - arp[i] : 0;
    nonempty[i] = len != 0; islong[i] = spmm_long(len);
  }
}

__global__ __launch_bounds__(256) void k_full_pattern(uint32_t nrows, uint32_t k, uint64_t nnz, const uint32_t* __restrict__ before, uint32_t* __restrict__ rowptr, uint32_t* __restrict__ col) {
  const uint64_t n = nnz > nrows ? nnz : (uint64_t)nrows + 1;
  for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < n; e += gridDim.x * 256ull) {
    if (e < nnz) col[e] = (uint32_t)(e % k);
    if (e <= nrows) rowptr[e] = (uint32_t)spmm_rowptr(before ? before[e] : e, k);
  }
}

__global__ __launch_bounds__(256) void k_spmm_long_tasks(const uint32_t* __restrict__ arp, uint32_t m, const uint32_t* __restrict__ lrank, uint32_t* __restrict__ task, uint32_t* __restrict__ lrow) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t r0 = (blockIdx.x * 4ull + (threadIdx.x >> 6)) * 64ull; r0 < m; r0 += gridDim.x * 256ull) {
    const uint64_t i = r0 + lane;
    uint32_t base = 0, nch = 0;
    if (i < m) {
      const uint32_t rs = arp[i]; nch = spmm_chunks(arp[i + 1] - rs);
      if (nch) { const uint32_t q = lrank[i]; base = spmm_slot_base(rs, q); lrow[q] = (uint32_t)i; }
    }
    unsigned long long todo = __ballot(nch != 0);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1; todo &= todo - 1;
      const uint32_t b = __shfl(base, src), n = __shfl(nch, src), row = (uint32_t)(r0 + src);
      for (uint32_t c = lane; c < n; c += 64) task[b + c] = row;
    }
  }
}

}  // namespace

void full_pattern_fill(uint32_t nrows, uint32_t k, uint64_t nnz, const uint32_t* before, uint32_t* rowptr, uint32_t* col) {
  const uint64_t n = nnz > nrows ? nnz : (uint64_t)nrows + 1;
  hipLaunchKernelGGL(k_full_pattern, dim3(grid_1d(n, 8192)), dim3(256), 0, stream(), nrows, k, nnz, before, rowptr, col);
  GRB_HIP(hipGetLastError());
}

bool spmm_full(const SpgemmCall& c, const SemiringDesc& d, DevCSR& out, SpmmPlan& plan) {
  const DevCSR& A = *c.A; const uint32_t m = A.nrows, k = c.B->ncols; const size_t ts = type_size(d.zcode);
  plan = SpmmPlan{}; plan.k = k; plan.group = spmm_narrow(k) ? spmm_group(k) : 0; plan.slabs = spmm_narrow(k) ? 1 : spmm_slabs(k);
  // the two counts: non-empty rows (T's row pointer, nvals(T)) and long rows
  DevBuf flags(((size_t)m + 1) * 8), pos(((size_t)m + 1) * 8);
  uint32_t* ne = flags.as<uint32_t>(); uint32_t* lg = ne + m + 1; uint32_t* before = pos.as<uint32_t>(); uint32_t* lrank = before + m + 1;
  hipLaunchKernelGGL(k_spmm_rowflags, dim3(grid_1d((uint64_t)m + 1)), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), m, ne, lg);
  exclusive_scan_u32(ne, before, (uint64_t)m + 1);
  const bool may_be_long = A.nnz > SPMM_L;                         // (no row is longer than the matrix)
  if (may_be_long) exclusive_scan_u32(lg, lrank, (uint64_t)m + 1);
  uint32_t* pin = (uint32_t*)pinned_scratch(); pin[1] = 0;
  GRB_HIP(hipMemcpyAsync(pin, before + m, 4, hipMemcpyDeviceToHost, stream()));
  if (may_be_long) GRB_HIP(hipMemcpyAsync(pin + 1, lrank + m, 4, hipMemcpyDeviceToHost, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));
  const uint64_t nonempty = pin[0], nlong = pin[1];
  if (spmm_overflows(nonempty, k)) return false;
  const uint64_t nnz = spmm_rowptr(nonempty, k);
  out.clear(); out.nrows = m; out.ncols = k; out.nnz = nnz;
  out.rowptr.alloc(((size_t)m + 1) * 4); out.col.alloc(nnz * 4 + 8); out.val.alloc(nnz * ts + 16);
  full_pattern_fill(m, k, nnz, before, out.rowptr.as<uint32_t>(), out.col.as<uint32_t>());
  out.valid = true; plan.nlong = nlong;
  if (!nnz) return true;
  SpmmValuesCall v{}; v.A = &A; v.aval = c.aval; v.bval = c.bval; v.k = k; v.trp = out.rowptr.as<uint32_t>(); v.tval = out.val.p; v.lrank = lrank;
  DevBuf task, lrow, part;
  if (nlong) {
    v.nlong = nlong; v.nslots = spmm_slots(A.nnz, nlong);
    task.alloc(v.nslots * 4); lrow.alloc(nlong * 4); part.alloc(v.nslots * k * ts + 16);
    GRB_HIP(hipMemsetAsync(task.p, 0xFF, v.nslots * 4, stream()));
    hipLaunchKernelGGL(k_spmm_long_tasks, dim3(grid_1d(m)), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), m, lrank, task.as<uint32_t>(), lrow.as<uint32_t>());
    v.task = task.as<uint32_t>(); v.lrow = lrow.as<uint32_t>(); v.part = part.p;
  }
  dispatch_type(d.zcode, [&]<class T>() { run_spmm_values<T>(v, d); });
  return true;
}

}  // namespace grb
