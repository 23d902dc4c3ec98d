// fa_fwd_rp16_d128w.hip -- the pipeline at d = 128 with ONE wave per SIMD: four 64-row waves per 256-row workgroup, the whole
// 512-register file per wave (fa_fwd_rp16_kernel.hpp, kWv = 4).
#include "fa_fwd_rp16_kernel.hpp"

namespace fa {

template hipError_t rp16_family<128, 4, false, false, 4>(const FwdArgs&, bool);

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids_d128w(unsigned* p) { return rp16_set_pass_ids_tu(p); }
#endif

}  // namespace fa
