// fa_fwd_varlen_cache_routed_fp8.hip -- the LONG half of fa_kvcache_attend_varlen on an fp8 (OCP e4m3fn) cache: the 32 kRouted fp8
// cache instantiations of fa_fwd_varlen_kernel.hpp (T x d x out x paged x kLogits, causal only).  All options off runs the plain
// kernels and any other the kLogits ones, as in fa_forward_varlen_kvcache_fp8, whose bits the LONG rows carry.  DESIGN.md 7.15, 7.20.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

hipError_t varlen_cache_routed_launch8(const fa_varlen_kvcache_desc* d, const void* args, unsigned grid, int min_rows)
{
    const VarlenCacheFp8Args& a = *static_cast<const VarlenCacheFp8Args*>(args);
    if (!d->sinks && d->window == 0 && d->softcap == 0.0f) return varlen_cache_routed_launch<false>(d, a, dim3(grid), min_rows);
    return varlen_cache_routed_launch<true>(d, a, dim3(grid), min_rows);
}

}  // namespace fa
