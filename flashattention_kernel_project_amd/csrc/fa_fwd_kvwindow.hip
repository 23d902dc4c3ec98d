// fa_fwd_kvwindow.hip -- sliding-window decode against a 16-bit KV cache, contiguous (fa_forward_kvcache_window) and paged
// (fa_forward_kvcache_paged_window): the streams of fa_fwd_kvcache.hip / fa_fwd_kvpaged.hip with a lower key limit per row and a
// first tile per sequence.  DESIGN.md section 7.6 has the reasoning; the kernels are the WindowArgs instantiations of
// fa_fwd_split_kernel.hpp, the merge is fa_fwd_kvcache.hip's.  The fp8 forms are in fa_fwd_kvwindow_fp8.hip.
#include "fa_fwd_kvwindow.hpp"

namespace fa {

// The longest key range one sequence can stream under a window, in keys: the window of the last row plus the Nq - 1 keys the rows
// before it add, rounded up to tiles, plus one tile because the range starts inside a tile; never more than the capacity.
int window_span_cap(int Nq, int Ncap, int window)
{
    const long long need = (long long)window + Nq - 1;
    if (need >= Ncap) return Ncap;
    const long long span = (need + kBlockN - 1) / kBlockN * kBlockN + kBlockN;
    return span < Ncap ? (int)span : Ncap;
}

size_t kvwindow_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D, int window)
{
    if (window < 0) return 0;
    if (window == 0) return kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, D);
    if (B <= 0 || Hkv <= 0 || G <= 0 || Nq <= 0 || Ncap <= 0 || (D != 64 && D != 128)) return 0;
    if ((long long)B * Hkv > 0x7FFFFFFFll || (long long)G * Nq > 0x7FFFFFFFll) return 0;
    return split_workspace_bytes(B * Hkv, G * Nq, window_span_cap(Nq, Ncap, window), D);
}

size_t kvpaged_window_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int D, int window)
{
    // the paged sizing function knows which (max_pages, page_size) the entry takes: 0 for those it rejects
    if (window < 0 || max_pages <= 0 || page_size <= 0 || (long long)max_pages * page_size > 0x7FFFFFFFll) return 0;
    if (window == 0) return kvpaged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, D);
    if (page_size < 16 || (page_size & (page_size - 1)) != 0) return 0;
    return kvwindow_workspace_bytes(B, Hkv, G, Nq, max_pages * page_size, D, window);
}

hipError_t kvcache_window_dispatch(const KvCacheArgs& a, int window)
{
    if (window < 0) return hipErrorInvalidValue;
    if (window == 0) return kvcache_dispatch(a);
    const hipError_t bad = kvcache_check(a);
    if (bad != hipSuccess) return bad;
    WindowArgs<CacheArgs> pack;
    static_cast<CacheArgs&>(pack) = {a.seqlens, nullptr, a.Hkv, a.Nq, a.causal};
    pack.window = window;
    return dispatch_kvwindow(a, pack);
}

hipError_t kvpaged_window_dispatch(const KvPagedArgs& p, int window)
{
    if (window < 0) return hipErrorInvalidValue;
    if (window == 0) return kvpaged_dispatch(p);
    KvPagedArgs q;
    int lg_page;
    const hipError_t bad = kvpaged_check(p, q, lg_page);
    if (bad != hipSuccess) return bad;
    const KvCacheArgs& a = q.c;
    WindowArgs<PagedArgs> pack;
    static_cast<PagedArgs&>(pack) = {{a.seqlens, nullptr, a.Hkv, a.Nq, a.causal}, p.table, p.max_pages, p.num_pages, lg_page};
    pack.window = window;
    return dispatch_kvwindow(a, pack);
}

}  // namespace fa
