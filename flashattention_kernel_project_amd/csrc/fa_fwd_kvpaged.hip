// fa_fwd_kvpaged.hip -- decode against a paged KV cache (fa_forward_kvcache_paged): the KV-cache stream of fa_fwd_kvcache.hip with
// every tile's rows taken from pages of a pool through a block table that is read on the device.  DESIGN.md section 7.2 has the
// reasoning; the kernels are the PagedArgs instantiations of fa_fwd_split_kernel.hpp, the merge is fa_fwd_kvcache.hip's.
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

namespace fa {

// Grid, split count and workspace are those of fa_forward_kvcache for Ncap = max_pages * page_size: nothing here reads the lengths
// or the table, so a captured launch stays valid when either changes in place.
template <typename T, int D, bool kOutF32>
static hipError_t launch_kvpaged(const KvPagedArgs& p, int BH, int rows, int lg_page)
{
    using G = TileGeom<D>;
    const KvCacheArgs& a = p.c;
    const int S = split_count(BH, rows, a.Ncap);
    const int nqb = (rows + split::kRows - 1) / split::kRows;
    const long long nwg = (long long)BH * nqb * S;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, a.Ncap, D))) return hipErrorInvalidValue;
    const uint16_t *q = static_cast<const uint16_t*>(a.Q), *k = static_cast<const uint16_t*>(a.K), *v = static_cast<const uint16_t*>(a.V);
    hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, false, true, PagedArgs>), G::kLdsBytes);
    if (attr == hipSuccess) attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, true, true, PagedArgs>), G::kLdsBytes);
    if (attr != hipSuccess) return attr;
    // the one-pass kernel stores the log-sum-exp itself; behind a split the merge does
    const PagedArgs pa = {{a.seqlens, S == 1 ? a.lse : nullptr, a.Hkv, a.Nq, a.causal}, p.table, p.max_pages, p.num_pages, lg_page};
    if (S == 1) {
        FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, false, true, PagedArgs>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                           a.stream, q, k, v, a.O, static_cast<float*>(nullptr), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pa);
        return launch_status();
    }
    FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, true, true, PagedArgs>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                       a.stream, q, k, v, a.O, static_cast<float*>(a.ws), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pa);
    hipError_t e = launch_status();
    if (e != hipSuccess) return e;
    return kvcache_combine(a.ws, a.O, a.lse, BH, rows, D, S, a.in_dtype, a.out_dtype, a.stream);
}

// log2 of a page size the kernel takes (a power of two, at least 16 keys), else -1
static int page_log2(int page_size)
{
    if (page_size < 16 || (page_size & (page_size - 1)) != 0) return -1;
    int lg = 4;
    while ((1 << lg) != page_size) ++lg;
    return lg;
}

size_t kvpaged_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int D)
{
    if (max_pages <= 0 || page_log2(page_size) < 0 || (long long)max_pages * page_size > 0x7FFFFFFFll) return 0;
    return kvcache_workspace_bytes(B, Hkv, G, Nq, max_pages * page_size, D);
}

// What the paged entries (fa_fwd_kvfp8.hip's too) reject before the device is touched.  On success q is p with the capacity
// filled in and lg_page the log2 of the page size.
hipError_t kvpaged_check(const KvPagedArgs& p, KvPagedArgs& q, int& lg_page)
{
    lg_page = page_log2(p.page_size);
    if (!p.table || lg_page < 0 || p.num_pages <= 0 || p.max_pages <= 0) return hipErrorInvalidValue;
    if ((long long)p.max_pages * p.page_size > 0x7FFFFFFFll) return hipErrorInvalidValue;   // the capacity is an int
    q = p;
    q.c.Ncap = p.max_pages * p.page_size;
    // from here on the checks of kvcache_dispatch, on that capacity.  Its bound on the byte offsets covers what is 32 bit in the
    // kernel here: a tile's byte offset before it is reduced to the page (hence the page-head block too)
    return kvcache_check(q.c);
}

hipError_t kvpaged_dispatch(const KvPagedArgs& p)
{
    KvPagedArgs q;
    int lg_page;
    const hipError_t bad = kvpaged_check(p, q, lg_page);
    if (bad != hipSuccess) return bad;
    const KvCacheArgs& a = q.c;
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq;
    if (a.D == 64)
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            return launch_kvpaged<decltype(t), 64, decltype(f32)::value>(q, BH, rows, lg_page);
        });
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        return launch_kvpaged<decltype(t), 128, decltype(f32)::value>(q, BH, rows, lg_page);
    });
}

}  // namespace fa
