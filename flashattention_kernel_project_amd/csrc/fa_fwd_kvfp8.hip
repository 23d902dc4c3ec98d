// fa_fwd_kvfp8.hip -- decode against an fp8 (OCP e4m3fn) KV cache, contiguous (fa_forward_kvcache_fp8) and paged
// (fa_forward_kvcache_paged_fp8), with a dequantisation scale per K/V head.  K and V are widened to the query's 16-bit type while a
// tile is written to LDS, so the LDS images, the MFMAs, the softmax, the splits, the merge and the masks are those of
// fa_fwd_kvcache.hip / fa_fwd_kvpaged.hip; half the bytes cross HBM.  DESIGN.md section 7.4 has the reasoning; the kernels are the
// Fp8Args instantiations of fa_fwd_split_kernel.hpp, the merge is fa_fwd_kvcache.hip's.
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

namespace fa {

// Grid, split count and workspace are those of the 16-bit entry for the same shape: nothing here reads lengths, table or scales,
// so a captured launch stays valid when any of them changes in place.  Pack: Fp8Args<CacheArgs> or Fp8Args<PagedArgs> with
// everything but the log-sum-exp pointer filled in.
template <typename T, int D, bool kOutF32, typename Pack>
static hipError_t launch_kvfp8(const KvCacheArgs& a, Pack pack, int BH, int rows)
{
    using G = TileGeom<D>;
    const int S = split_count(BH, rows, a.Ncap);
    const int nqb = (rows + split::kRows - 1) / split::kRows;
    const long long nwg = (long long)BH * nqb * S;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, a.Ncap, D))) return hipErrorInvalidValue;
    // the kernel's K/V parameters are typed for the 16-bit caches; the fp8 instantiations address them as bytes
    const uint16_t *q = static_cast<const uint16_t*>(a.Q), *k = static_cast<const uint16_t*>(a.K), *v = static_cast<const uint16_t*>(a.V);
    hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, false, true, Pack>), G::kLdsBytes);
    if (attr == hipSuccess) attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, true, true, Pack>), G::kLdsBytes);
    if (attr != hipSuccess) return attr;
    // the one-pass kernel stores the log-sum-exp itself; behind a split the merge does
    pack.lse = S == 1 ? a.lse : nullptr;
    if (S == 1) {
        FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, false, true, Pack>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                           a.stream, q, k, v, a.O, static_cast<float*>(nullptr), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pack);
        return launch_status();
    }
    FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, true, true, Pack>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                       a.stream, q, k, v, a.O, static_cast<float*>(a.ws), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pack);
    hipError_t e = launch_status();
    if (e != hipSuccess) return e;
    return kvcache_combine(a.ws, a.O, a.lse, BH, rows, D, S, a.in_dtype, a.out_dtype, a.stream);
}

template <typename Pack>
static hipError_t dispatch_kvfp8(const KvCacheArgs& a, const Pack& pack)
{
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq;
    if (a.D == 64)
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            return launch_kvfp8<decltype(t), 64, decltype(f32)::value>(a, pack, BH, rows);
        });
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        return launch_kvfp8<decltype(t), 128, decltype(f32)::value>(a, pack, BH, rows);
    });
}

hipError_t kvcache_fp8_dispatch(const KvCacheArgs& a, const float* k_scale, const float* v_scale)
{
    const hipError_t bad = kvcache_check(a);
    if (bad != hipSuccess) return bad;
    Fp8Args<CacheArgs> pack;
    static_cast<CacheArgs&>(pack) = {a.seqlens, nullptr, a.Hkv, a.Nq, a.causal};
    pack.k_scale = k_scale;
    pack.v_scale = v_scale;
    return dispatch_kvfp8(a, pack);
}

hipError_t kvpaged_fp8_dispatch(const KvPagedArgs& p, const float* k_scale, const float* v_scale)
{
    KvPagedArgs q;
    int lg_page;
    const hipError_t bad = kvpaged_check(p, q, lg_page);
    if (bad != hipSuccess) return bad;
    const KvCacheArgs& a = q.c;
    Fp8Args<PagedArgs> pack;
    static_cast<PagedArgs&>(pack) = {{a.seqlens, nullptr, a.Hkv, a.Nq, a.causal}, p.table, p.max_pages, p.num_pages, lg_page};
    pack.k_scale = k_scale;
    pack.v_scale = v_scale;
    return dispatch_kvfp8(a, pack);
}

}  // namespace fa
