// fa_fwd_rp16_d64.hip -- the pipeline at d = 64 on 64-row waves (512-row workgroups), its half-width running-max body inside the same kernels (fa_fwd_rp16_kernel.hpp).
#include "fa_fwd_rp16_kernel.hpp"

namespace fa {

template hipError_t rp16_family<64, 4, false, false>(const FwdArgs&, bool);
#ifdef FA_EXPERIMENTS
template hipError_t rp16_family<64, 4, true, false>(const FwdArgs&, bool);   // K/V staged by LDS-DMA
#endif

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids_d64(unsigned* p) { return rp16_set_pass_ids_tu(p); }
#endif

}  // namespace fa
