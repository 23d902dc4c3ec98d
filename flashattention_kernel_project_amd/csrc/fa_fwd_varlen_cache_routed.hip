// fa_fwd_varlen_cache_routed.hip -- the LONG half of fa_kvcache_attend_varlen on a 16-bit cache: the 32 kRouted cache instantiations
// of fa_fwd_varlen_kernel.hpp (T x d x out x paged x kLogits, causal only), in a unit of their own so that no existing unit's code
// moves.  As in fa_forward_varlen_kvcache a call with all three options off runs the plain kernels and any other the kLogits ones,
// so the LONG rows carry that entry's bits by construction.  The checks are fa_fwd_varlen_cache.hip's; the reasons are DESIGN.md 7.20.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

hipError_t varlen_cache_routed_launch16(const fa_varlen_kvcache_desc* d, const void* args, unsigned grid, int min_rows)
{
    const VarlenCacheArgs& a = *static_cast<const VarlenCacheArgs*>(args);
    if (!d->sinks && d->window == 0 && d->softcap == 0.0f) return varlen_cache_routed_launch<false>(d, a, dim3(grid), min_rows);
    return varlen_cache_routed_launch<true>(d, a, dim3(grid), min_rows);
}

}  // namespace fa
