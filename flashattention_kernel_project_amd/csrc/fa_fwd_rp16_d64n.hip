// fa_fwd_rp16_d64n.hip -- the pipeline at d = 64 on 32- and 16-row waves (small grids) (fa_fwd_rp16_kernel.hpp).
#include "fa_fwd_rp16_kernel.hpp"

namespace fa {

template hipError_t rp16_family<64, 2, false, false>(const FwdArgs&, bool);
template hipError_t rp16_family<64, 1, false, false>(const FwdArgs&, bool);

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids_d64n(unsigned* p) { return rp16_set_pass_ids_tu(p); }
#endif

}  // namespace fa
