// grb_sddmm.hip — the masked product of two full matrices (grb_sddmm.hpp): the driver.  T's pattern is the mask's, copied; the value kernel is
// grb_sddmm_kernels.hpp, instantiated per type in grb_sddmm_inst.hip.  No kernel of its own lives here: the pattern needs no computing.
#include "grb_sddmm.hpp"
#include "grb_api.hpp"
#include "grb_device.hpp"

namespace grb {

void sddmm_full(const DevCSR& M, const void* xval, const void* yval, uint32_t k, const SemiringDesc& d, DevCSR& out, SddmmPlan& plan) {
  const size_t ts = type_size(d.zcode);
  plan = SddmmPlan{}; plan.k = k; plan.group = sddmm_group(k); plan.entries = M.nnz;
  out.clear(); out.nrows = M.nrows; out.ncols = M.ncols; out.nnz = M.nnz;
  out.rowptr.alloc(((size_t)M.nrows + 1) * 4); out.col.alloc(M.nnz * 4 + 8); out.val.alloc(M.nnz * ts + 16);
  GRB_HIP(hipMemcpyAsync(out.rowptr.p, M.rowptr.p, ((size_t)M.nrows + 1) * 4, hipMemcpyDeviceToDevice, stream()));
  if (M.nnz) GRB_HIP(hipMemcpyAsync(out.col.p, M.col.p, M.nnz * 4, hipMemcpyDeviceToDevice, stream()));
  out.valid = true;
  if (!M.nnz) return;
  SddmmValuesCall v{};
  v.mrp = out.rowptr.as<uint32_t>(); v.mcol = out.col.as<uint32_t>(); v.m = M.nrows; v.entries = M.nnz;
  v.xval = xval; v.yval = yval; v.k = k; v.tval = out.val.p;
  dispatch_type(d.zcode, [&]<class T>() { run_sddmm_values<T>(v, d); });
}

}  // namespace grb
