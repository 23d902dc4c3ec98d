// fa_fwd_rp16_c.hip -- the pipeline under the causal mask, d = 64 and d = 128 (fa_fwd_rp16_kernel.hpp).
#include "fa_fwd_rp16_kernel.hpp"

namespace fa {

template hipError_t rp16_family<64, 4, false, true>(const FwdArgs&, bool);
template hipError_t rp16_family<128, 2, false, true>(const FwdArgs&, bool);

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids_c(unsigned* p) { return rp16_set_pass_ids_tu(p); }
#endif

}  // namespace fa
