// grb_gemv_inst.hip — explicit instantiation of the kernels of a full matrix times a vector for ONE value type (-DGRB_INST_TYPE=...).
#include "grb_gemv_kernels.hpp"
namespace grb {
using std::int8_t; using std::uint8_t; using std::int16_t; using std::uint16_t; using std::int32_t; using std::uint32_t; using std::int64_t; using std::uint64_t;
template void run_gemv_values<GRB_INST_TYPE>(const GemvValuesCall&, const SemiringDesc&);
}
