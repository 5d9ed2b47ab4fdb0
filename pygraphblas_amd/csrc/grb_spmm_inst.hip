// grb_spmm_inst.hip — explicit instantiation of the full-operand product's value kernels for ONE value type (-DGRB_INST_TYPE=...).
#include "grb_spmm_kernels.hpp"
namespace grb {
using std::int8_t; using std::uint8_t; using std::int16_t; using std::uint16_t; using std::int32_t; using std::uint32_t; using std::int64_t; using std::uint64_t;
template void run_spmm_values<GRB_INST_TYPE>(const SpmmValuesCall&, const SemiringDesc&);
}
