// fa_fwd_kvcache.hip -- decode against a pre-allocated KV cache (fa_forward_kvcache): the split-KV stream of fa_fwd_split.hip with
// the key count of each sequence read on the device, a causal mask aligned to the end of the cache and a log-sum-exp output.
// DESIGN.md section 7 has the reasoning; the kernels are the CacheArgs instantiations of fa_fwd_split_kernel.hpp, launched through
// the host path of fa_fwd_kvdecode.hpp like those of the eight units beside this one.  Also here, once for all decode entries:
// the argument checks, the entry kvdecode_dispatch and the merge kernel.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

size_t kvcache_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D)
{
    if (B <= 0 || Hkv <= 0 || G <= 0 || Nq <= 0 || Ncap <= 0 || (D != 64 && D != 128)) return 0;
    if ((long long)B * Hkv > 0x7FFFFFFFll || (long long)G * Nq > 0x7FFFFFFFll) return 0;
    return split_workspace_bytes(B * Hkv, G * Nq, Ncap, D);
}

// What every KV-cache entry rejects before the device is touched (the fp8 entries too: their one-byte elements keep the 16-bit
// bound on the byte offsets).
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

// The translation unit that owns the kernels of the pack the flags name.  Window 0 is the un-windowed entry itself: it launches
// the un-windowed kernels.  With sinks or a soft-cap the LogitArgs kernels run, which wrap the windowed packs only: window 0 goes
// there as window = Ncap, which include/fa_mi355.h guarantees to be the un-windowed result bit for bit, on the same split count.
// With seqlens_q the RaggedArgs kernels run, which wrap the LogitArgs packs, under the same rule for window 0.
static hipError_t kvdecode_handover(const KvDecodeArgs& d, int lg_page)
{
    if (d.sinks || d.softcap != 0.0f || d.seqlens_q) {
        KvDecodeArgs w = d;
        if (w.window == 0) w.window = w.p.c.Ncap;
        if (w.seqlens_q) return w.fp8 ? kvragged_fp8_decode(w, lg_page) : kvragged_decode(w, lg_page);
        return w.fp8 ? kvlogits_fp8_decode(w, lg_page) : kvlogits_decode(w, lg_page);
    }
    if (d.window == 0) return d.fp8 ? kvfp8_decode(d, lg_page) : d.paged ? kvpaged_decode(d, lg_page) : kvcache_decode(d, lg_page);
    return d.fp8 ? kvwindow_fp8_decode(d, lg_page) : kvwindow_decode(d, lg_page);
}

// The one entry behind the eight fa_forward_kvcache* functions: the checks, once, then the hand-over.
hipError_t kvdecode_dispatch(const KvDecodeArgs& d)
{
    if (d.window < 0) return hipErrorInvalidValue;
    if (!(d.softcap >= 0.0f) || __builtin_isinf(d.softcap)) return hipErrorInvalidValue;   // negative, NaN or inf
    if (!d.paged) {
        const hipError_t bad = kvcache_check(d.p.c);
        return bad != hipSuccess ? bad : kvdecode_handover(d, 0);
    }
    KvDecodeArgs q = {{}, d.k_scale, d.v_scale, d.window, d.paged, d.fp8, d.sinks, d.softcap, d.seqlens_q};   // q.p: d.p with the capacity, from the check
    int lg_page;
    const hipError_t bad = kvpaged_check(d.p, q.p, lg_page);
    return bad != hipSuccess ? bad : kvdecode_handover(q, lg_page);
}

hipError_t kvcache_decode(const KvDecodeArgs& d, int lg_page) { return dispatch_kvdecode<CacheArgs>(d, lg_page); }

// The merge behind a split, for every decode entry: the kernel is instantiated in this translation unit only.
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
