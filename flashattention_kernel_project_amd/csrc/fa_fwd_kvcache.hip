// fa_fwd_kvcache.hip -- decode against a pre-allocated KV cache (fa_forward_kvcache): the split-KV stream of fa_fwd_split.hip with
// the key count of each sequence read on the device, a causal mask aligned to the end of the cache and a log-sum-exp output.
// DESIGN.md section 7 has the reasoning; the kernels are the kCache = true instantiations of fa_fwd_split_kernel.hpp.
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

namespace fa {

// ---- KV-cache decode: BH = B * Hkv K/V heads of Ncap rows, rows = G * Nq folded query rows per K/V head ----
// Grid, split count and workspace follow from the capacity alone: nothing here reads seqlens, so a captured launch stays valid
// when the lengths change in place.
template <typename T, int D, bool kOutF32>
static hipError_t launch_kvcache(const KvCacheArgs& a, int BH, int rows)
{
    using G = TileGeom<D>;
    const int S = split_count(BH, rows, a.Ncap);
    const int nqb = (rows + split::kRows - 1) / split::kRows;
    const long long nwg = (long long)BH * nqb * S;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, a.Ncap, D))) return hipErrorInvalidValue;
    const uint16_t *q = static_cast<const uint16_t*>(a.Q), *k = static_cast<const uint16_t*>(a.K), *v = static_cast<const uint16_t*>(a.V);
    hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, false, true, CacheArgs>), G::kLdsBytes);
    if (attr == hipSuccess) attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, true, true, CacheArgs>), G::kLdsBytes);
    if (attr != hipSuccess) return attr;
    // the one-pass kernel stores the log-sum-exp itself; behind a split the merge does
    const CacheArgs ca = {a.seqlens, S == 1 ? a.lse : nullptr, a.Hkv, a.Nq, a.causal};
    if (S == 1) {
        FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, false, true, CacheArgs>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                           a.stream, q, k, v, a.O, static_cast<float*>(nullptr), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), ca);
        return launch_status();
    }
    FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, true, true, CacheArgs>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                       a.stream, q, k, v, a.O, static_cast<float*>(a.ws), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), ca);
    hipError_t e = launch_status();
    if (e != hipSuccess) return e;
    const long long out_rows = (long long)BH * rows;   // one wave per output row
    if (out_rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    FA_LAUNCH((fa_split_combine_kernel<T, kOutF32, true, float*>), dim3((unsigned)out_rows), dim3(64), 0, a.stream,
                       static_cast<const float*>(a.ws), a.O, BH, rows, D, S, a.lse);
    return launch_status();
}

size_t kvcache_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D)
{
    if (B <= 0 || Hkv <= 0 || G <= 0 || Nq <= 0 || Ncap <= 0 || (D != 64 && D != 128)) return 0;
    if ((long long)B * Hkv > 0x7FFFFFFFll || (long long)G * Nq > 0x7FFFFFFFll) return 0;
    return split_workspace_bytes(B * Hkv, G * Nq, Ncap, D);
}

// What every KV-cache entry rejects before the device is touched (the fp8 entries of fa_fwd_kvfp8.hip too: their one-byte
// elements keep the 16-bit bound on the byte offsets).
hipError_t kvcache_check(const KvCacheArgs& a)
{
    if (!a.Q || !a.K || !a.V || !a.O) return hipErrorInvalidValue;
    if (a.B <= 0 || a.Hkv <= 0 || a.G <= 0 || a.Nq <= 0 || a.Ncap <= 0 || (a.D != 64 && a.D != 128)) return hipErrorInvalidValue;
    if (a.causal != 0 && a.causal != 1) return hipErrorInvalidValue;
    if (a.in_dtype != 0 && a.in_dtype != 1) return hipErrorInvalidValue;
    if (a.out_dtype != 0 && a.out_dtype != 1) return hipErrorInvalidValue;
    if ((long long)a.B * a.Hkv > 0x7FFFFFFFll || (long long)a.G * a.Nq > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const int rows = a.G * a.Nq;
    // per-head byte offsets are 32 bit: the checks of split_dispatch, on the folded rows and the capacity
    if (((unsigned long long)rows + split::kRows) * (unsigned)(a.D + 2) * 4ull >= (1ull << 32)) return hipErrorInvalidValue;
    if (((unsigned long long)a.Ncap + kBlockN) * (unsigned)a.D * 2ull >= (1ull << 32)) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t kvcache_dispatch(const KvCacheArgs& a)
{
    const hipError_t bad = kvcache_check(a);
    if (bad != hipSuccess) return bad;
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq;
    if (a.D == 64)
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            return launch_kvcache<decltype(t), 64, decltype(f32)::value>(a, BH, rows);
        });
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        return launch_kvcache<decltype(t), 128, decltype(f32)::value>(a, BH, rows);
    });
}

// The merge behind a split, for the paged entry (fa_fwd_kvpaged.hip): the kernel is instantiated in this translation unit only.
hipError_t kvcache_combine(const void* ws, void* O, float* lse, int BH, int rows, int D, int S, int in_dtype, int out_dtype,
                           hipStream_t stream)
{
    const long long out_rows = (long long)BH * rows;   // one wave per output row
    if (out_rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
        FA_LAUNCH((fa_split_combine_kernel<decltype(t), decltype(f32)::value, true, float*>), dim3((unsigned)out_rows), dim3(64), 0,
                  stream, static_cast<const float*>(ws), O, BH, rows, D, S, lse);
        return launch_status();
    });
}

}  // namespace fa
