// fa_fwd_varlen_cache_fp8.hip -- fa_forward_varlen_kvcache_fp8: the varlen prefill against an fp8 (OCP e4m3fn) KV cache, contiguous or
// paged, with one fp32 scale per K/V head: the cache the fp8 append writes and the fp8 decode entries read.  The contract is
// include/fa_mi355.h's; the reasons are DESIGN.md 7.15.  The kernel template is fa_fwd_varlen_kernel.hpp's (kFp8); the checks are
// fa_fwd_varlen_cache.hip's.  This unit holds the 32 plain fp8 cache instantiations (T x d x out x causal x paged); the windowed /
// soft-capped / sink ones are fa_fwd_varlen_cache_fp8_logits.hip's, as with the 16-bit entries.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

hipError_t varlen_cache_fp8_dispatch(const fa_varlen_kvcache_desc* d, const float* k_scale, const float* v_scale)
{
    VarlenCacheFp8Args a;
    dim3 grid;
    const hipError_t e = varlen_cache_check(d, a, grid);
    if (e != hipSuccess) return e;
    a.k_scale = k_scale;
    a.v_scale = v_scale;
    // all three options off: the plain kernels, as in varlen_cache_dispatch
    if (!d->sinks && d->window == 0 && d->softcap == 0.0f) return varlen_cache_launch<false>(d, a, grid);
    return varlen_cache_fp8_logits_launch(d, &a, grid.x);
}

}  // namespace fa
