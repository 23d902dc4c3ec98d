// fa_fwd_kvwindow_fp8.hip -- sliding-window decode against an fp8 (OCP e4m3fn) KV cache, contiguous (fa_forward_kvcache_fp8_window)
// and paged (fa_forward_kvcache_paged_fp8_window): fa_fwd_kvwindow.hip's entries over the streams of fa_fwd_kvfp8.hip.  The kernels
// are the WindowArgs<Fp8Args<...>> instantiations of fa_fwd_split_kernel.hpp; DESIGN.md sections 7.4 and 7.6.
#include "fa_fwd_kvwindow.hpp"

namespace fa {

hipError_t kvcache_fp8_window_dispatch(const KvCacheArgs& a, const float* k_scale, const float* v_scale, int window)
{
    if (window < 0) return hipErrorInvalidValue;
    if (window == 0) return kvcache_fp8_dispatch(a, k_scale, v_scale);
    const hipError_t bad = kvcache_check(a);
    if (bad != hipSuccess) return bad;
    WindowArgs<Fp8Args<CacheArgs>> pack;
    static_cast<CacheArgs&>(pack) = {a.seqlens, nullptr, a.Hkv, a.Nq, a.causal};
    pack.k_scale = k_scale;
    pack.v_scale = v_scale;
    pack.window = window;
    return dispatch_kvwindow(a, pack);
}

hipError_t kvpaged_fp8_window_dispatch(const KvPagedArgs& p, const float* k_scale, const float* v_scale, int window)
{
    if (window < 0) return hipErrorInvalidValue;
    if (window == 0) return kvpaged_fp8_dispatch(p, k_scale, v_scale);
    KvPagedArgs q;
    int lg_page;
    const hipError_t bad = kvpaged_check(p, q, lg_page);
    if (bad != hipSuccess) return bad;
    const KvCacheArgs& a = q.c;
    WindowArgs<Fp8Args<PagedArgs>> pack;
    static_cast<PagedArgs&>(pack) = {{a.seqlens, nullptr, a.Hkv, a.Nq, a.causal}, p.table, p.max_pages, p.num_pages, lg_page};
    pack.k_scale = k_scale;
    pack.v_scale = v_scale;
    pack.window = window;
    return dispatch_kvwindow(a, pack);
}

}  // namespace fa
