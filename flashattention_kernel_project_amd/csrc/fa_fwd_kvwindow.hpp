// fa_fwd_kvwindow.hpp -- the launcher the sliding-window decode entries share (fa_fwd_kvwindow.hip: 16-bit caches,
// fa_fwd_kvwindow_fp8.hip: fp8 caches).  Private to those two translation units: it instantiates kernels.
#pragma once
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

namespace fa {

// Pack: a WindowArgs<CacheArgs | PagedArgs | Fp8Args<...>> with everything but the log-sum-exp pointer filled in.  The split count
// follows from the longest range a sequence can stream (window_span_cap), not from the capacity; grid and workspace follow from
// it and still depend on host integers only, so a captured launch stays valid when lengths, table or scales change in place.
template <typename T, int D, bool kOutF32, typename Pack>
static hipError_t launch_kvwindow(const KvCacheArgs& a, Pack pack, int BH, int rows)
{
    using G = TileGeom<D>;
    const int span = window_span_cap(a.Nq, a.Ncap, pack.window);
    const int S = split_count(BH, rows, span);
    const int nqb = (rows + split::kRows - 1) / split::kRows;
    const long long nwg = (long long)BH * nqb * S;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, span, D))) return hipErrorInvalidValue;
    // the kernel's K/V parameters are typed for the 16-bit caches; the fp8 instantiations address them as bytes
    const uint16_t *q = static_cast<const uint16_t*>(a.Q), *k = static_cast<const uint16_t*>(a.K), *v = static_cast<const uint16_t*>(a.V);
    hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, false, true, Pack>), G::kLdsBytes);
    if (attr == hipSuccess) attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, true, true, Pack>), G::kLdsBytes);
    if (attr != hipSuccess) return attr;
    // the one-pass kernel stores the log-sum-exp itself; behind a split the merge does
    pack.lse = S == 1 ? a.lse : nullptr;
    // a window that covers the capacity is "every key" for every length: the clamp keeps the kernel's int arithmetic in range
    if (pack.window > a.Ncap) pack.window = a.Ncap;
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
static hipError_t dispatch_kvwindow(const KvCacheArgs& a, const Pack& pack)
{
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq;
    if (a.D == 64)
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            return launch_kvwindow<decltype(t), 64, decltype(f32)::value>(a, pack, BH, rows);
        });
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        return launch_kvwindow<decltype(t), 128, decltype(f32)::value>(a, pack, BH, rows);
    });
}

}  // namespace fa
