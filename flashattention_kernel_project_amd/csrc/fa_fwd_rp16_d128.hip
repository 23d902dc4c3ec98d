// fa_fwd_rp16_d128.hip -- the pipeline at d = 128 on 32-row waves (256-row workgroups, with the running-max body on 16-row waves inside the same kernels) and on 16-row waves (fa_fwd_rp16_kernel.hpp).
#include "fa_fwd_rp16_kernel.hpp"

namespace fa {

template hipError_t rp16_family<128, 2, false, false>(const FwdArgs&, bool);
template hipError_t rp16_family<128, 1, false, false>(const FwdArgs&, bool);

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids_d128(unsigned* p) { return rp16_set_pass_ids_tu(p); }
#endif

}  // namespace fa
