// grb_gemm.hip — the product of two full matrices (grb_gemm.hpp): the driver.  T is full, so its pattern is the closed form GrBX_Matrix_import_Full and the
// spmm_full route write (full_pattern_fill, grb_spmm.hip: nvals is m n, no scan and no copy to the host); the value kernel is grb_gemm_kernels.hpp, instantiated
// per type in grb_gemm_inst.hip.  No kernel of its own lives here.
#include "grb_gemm.hpp"
#include "grb_spmm.hpp"
#include "grb_api.hpp"
#include "grb_device.hpp"

namespace grb {

void gemm_full(uint32_t m, uint32_t n, uint32_t k, const void* aval, bool ta, const void* bval, bool tb, const SemiringDesc& d, DevCSR& out, GemmPlan& plan) {
  const size_t ts = type_size(d.zcode); const uint64_t nnz = (uint64_t)m * n;
  plan = GemmPlan{}; plan.m = m; plan.n = n; plan.k = k; plan.tm = gemm_tm(n); plan.tn = gemm_tn(n); plan.ta = ta; plan.tb = tb;
  out.clear(); out.nrows = m; out.ncols = n; out.nnz = nnz;
  out.rowptr.alloc(((size_t)m + 1) * 4); out.col.alloc(nnz * 4 + 8); out.val.alloc(nnz * ts + 16);
  full_pattern_fill(m, n, nnz, nullptr, out.rowptr.as<uint32_t>(), out.col.as<uint32_t>());
  out.valid = true;
  GemmValuesCall v{}; v.aval = aval; v.bval = bval; v.tval = out.val.p; v.m = m; v.n = n; v.k = k; v.ta = ta; v.tb = tb;
  dispatch_type(d.zcode, [&]<class T>() { run_gemm_values<T>(v, d); });
}

}  // namespace grb
