// fa_fwd_varlen_cache_fp8_logits.hip -- fa_forward_varlen_kvcache_fp8 with a sliding window, a soft-cap or attention sinks: the 32
// kLogits fp8 cache instantiations of fa_fwd_varlen_kernel.hpp (T x d x out x causal x paged), in a unit of their own so that neither
// set perturbs the other's code.  The checks are fa_fwd_varlen_cache.hip's; the reasons are DESIGN.md 7.15.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

hipError_t varlen_cache_fp8_logits_launch(const fa_varlen_kvcache_desc* d, const void* args, unsigned grid)
{
    return varlen_cache_launch<true>(d, *static_cast<const VarlenCacheFp8Args*>(args), dim3(grid));
}

}  // namespace fa
