// grb_gemm_inst.hip — explicit instantiation of the value kernel of the product of two full matrices for ONE value type (-DGRB_INST_TYPE=...).
#include "grb_gemm_kernels.hpp"
namespace grb {
using std::int8_t; using std::uint8_t; using std::int16_t; using std::uint16_t; using std::int32_t; using std::uint32_t; using std::int64_t; using std::uint64_t;
template void run_gemm_values<GRB_INST_TYPE>(const GemmValuesCall&, const SemiringDesc&);
}
