// grb_gemv.hip — a full matrix times a vector (grb_gemv.hpp): the driver.  It sizes the scratch slots of a product whose outputs have more than one chunk
// (closed form: grb_gemv_geom.hpp) and hands over to the kernels of grb_gemv_kernels.hpp, instantiated per type in grb_gemv_inst.hip.  No kernel of its own.
#include "grb_gemv.hpp"
#include "grb_api.hpp"
#include "grb_device.hpp"

namespace grb {

void gemv_full(int layout, uint64_t m, uint64_t k, const void* aval, const void* uval, const uint8_t* upres, const SemiringDesc& d, void* tval, GemvPlan& plan) {
  const size_t ts = type_size(d.zcode);
  plan = GemvPlan{}; plan.m = m; plan.k = k; plan.layout = layout; plan.holes = upres != nullptr; plan.chunks = gemv_chunks(layout, k);
  plan.kernel = layout == GEMV_T ? "k_gemv_t" : gemv_n_short(k) ? "k_gemv_n_short" : "k_gemv_n_wave";
  DevBuf part, flag;
  if (plan.chunks > 1) { part.alloc(m * plan.chunks * ts + 16); flag.alloc(m * plan.chunks + 16); }      // (m k < 2^32: no overflow; freed in stream order)
  GemvValuesCall c{layout, m, k, plan.chunks, aval, uval, upres, tval, part.p, flag.as<uint8_t>()};
  dispatch_type(d.zcode, [&]<class T>() { run_gemv_values<T>(c, d); });
}

}  // namespace grb
