// fa_fwd_rp16_cw.hip -- the pipeline under the causal mask at d = 128 with ONE wave per SIMD (four 64-row waves per 256-row
// workgroup, fa_fwd_rp16_kernel.hpp, kWv = 4): the causal twin of fa_fwd_rp16_d128w.hip.
#include "fa_fwd_rp16_kernel.hpp"

namespace fa {

template hipError_t rp16_family<128, 4, false, true, 4>(const FwdArgs&, bool);

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids_cw(unsigned* p) { return rp16_set_pass_ids_tu(p); }
#endif

}  // namespace fa
