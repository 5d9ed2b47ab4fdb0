// grb_transpose.hip — CSR -> CSR of the transpose, entirely in HBM.
// Used for GrB_vxm / desc.T0 (the pull kernels want rows of the effective left operand;
// gap/prmark.py:50 stores the matrix by column for exactly this reason),
// for GrB_transpose, and cached on the matrix after the first use.
//   1. expand rowptr to a row index per entry (csr_row_indices) and take col as the sort key
//   2. stable radix sort of (col -> entry position): within one column the original row-major
//      order, i.e. ascending rows, is preserved, so the output rows are sorted
//   3. gather values / row ids through the permutation; histogram + scan gives the new rowptr
#include "grb_api.hpp"
#include "grb_index.hpp"
#include "grb_matops.hpp"
#include "grb_build.hpp"

namespace grb {
namespace {

// row pointers of the transpose from the SORTED column keys (round 6): position i starts the run of key k[i]; every key between the one before and k[i] is an
// empty row that starts there too.  (One atomicAdd per entry — 1.3e8 device-scope atomics — took 12.6 ms of the 28 ms a BFS's first run spent building the transpose of the symmetric R-MAT-22.)
__global__ void k_rowptr_from_sorted(const uint32_t* __restrict__ k, uint64_t n, uint32_t nkeys, uint32_t* __restrict__ rowptr) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= n; i += gridDim.x * 256ull) {
    if (i == n) { for (uint32_t c = (n ? k[n - 1] + 1 : 0u); c <= nkeys; c++) rowptr[c] = (uint32_t)n; continue; }
    const uint32_t cur = k[i];
    if (i == 0) { for (uint32_t c = 0; c <= cur; c++) rowptr[c] = 0; }
    else { const uint32_t prev = k[i - 1]; if (prev != cur) for (uint32_t c = prev + 1; c <= cur; c++) rowptr[c] = (uint32_t)i; }
  }
}
template <int TS> __global__ void k_gather_perm(const uint32_t* __restrict__ perm, uint64_t n, const uint32_t* __restrict__ rowidx,
                                                const uint8_t* __restrict__ val, uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const uint32_t p = perm[i];
    ocol[i] = rowidx[p];
    ((W*)oval)[i] = ((const W*)val)[p];
  }
}

}  // namespace

// (also the last step of build-from-tuples, grb_build.hip: the rows of the run heads are sorted keys too)
void rowptr_from_sorted(const uint32_t* keys, uint64_t n, uint32_t nkeys, uint32_t* rowptr) {
  if (!n) { GRB_HIP(hipMemsetAsync(rowptr, 0, ((size_t)nkeys + 1) * 4, stream())); return; }      // (no key: one thread would write every word)
  hipLaunchKernelGGL(k_rowptr_from_sorted, dim3(grid_1d(n + 1)), dim3(256), 0, stream(), keys, n, nkeys, rowptr);
}

void csr_transpose(const DevCSR& A, size_t ts, DevCSR& At) {
  At.clear();
  At.nrows = A.ncols; At.ncols = A.nrows; At.nnz = A.nnz;
  const uint64_t nnz = A.nnz;
  At.rowptr.alloc(((size_t)At.nrows + 1) * 4); At.col.alloc(nnz * 4); At.val.alloc(nnz * ts);
  GRB_HIP(hipMemsetAsync(At.rowptr.p, 0, ((size_t)At.nrows + 1) * 4, stream()));
  if (nnz) {
    DevBuf rowidx(nnz * 4 + 4), perm_in(nnz * 4), perm(nnz * 4), keys_out(nnz * 4);
    csr_row_indices(A, rowidx.as<uint32_t>());
    fill_iota_u32(perm_in.as<uint32_t>(), nnz);
    int bits = 1; while (bits < 32 && (1ull << bits) < (uint64_t)A.ncols) bits++;
    sort_pairs_u32(A.col.as<uint32_t>(), keys_out.as<uint32_t>(), perm_in.as<uint32_t>(), perm.as<uint32_t>(), nnz, bits);
    rowptr_from_sorted(keys_out.as<uint32_t>(), nnz, At.nrows, At.rowptr.as<uint32_t>());
    dispatch_value_size(ts, [&]<int TS>() {
      hipLaunchKernelGGL((k_gather_perm<TS>), dim3(grid_1d(nnz)), dim3(256), 0, stream(), perm.as<uint32_t>(), nnz, rowidx.as<uint32_t>(), A.val.as<uint8_t>(), At.col.as<uint32_t>(), At.val.as<uint8_t>());
    });
    GRB_HIP(hipStreamSynchronize(stream()));   // temporaries are released on scope exit; the pool is stream-ordered
  }
  At.valid = true;
}

}  // namespace grb
