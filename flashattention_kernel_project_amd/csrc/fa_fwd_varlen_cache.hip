// fa_fwd_varlen_cache.hip -- fa_forward_varlen_kvcache: the variable-length prefill with its K/V rows taken from the KV cache, a
// contiguous one [B, Hkv, Ncap, d] or page pools behind a block table that is read on the device: chunked prefill, prefix caching,
// a window across the cache boundary, in one launch.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md 7.14.  The
// kernel template is fa_fwd_varlen_kernel.hpp's; this unit holds the checks and the 32 plain cache instantiations (T x d x out x
// causal x paged); the windowed / soft-capped / sink ones are fa_fwd_varlen_cache_logits.hip's, as with the packed entries.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

// fa_forward_varlen_kvcache's checks; on success the kernel arguments (the three options included) and the grid (host integers only).
// fa_forward_varlen_kvcache_fp8 (fa_fwd_varlen_cache_fp8.hip) runs them as they are: with one-byte elements the capacity bound
// Ncap * d * 2 <= 2^32 is twice what the byte offsets need, and every limit derived from it holds unchanged
hipError_t varlen_cache_check(const fa_varlen_kvcache_desc* d, VarlenCacheArgs& a, dim3& grid)
{
    if (!d || d->size != sizeof(fa_varlen_kvcache_desc)) return hipErrorInvalidValue;
    if (!d->cu_seqlens_q || !d->seqlens_k) return hipErrorInvalidValue;
    if (d->B <= 0 || d->Hkv <= 0 || d->G <= 0 || d->total_q <= 0) return hipErrorInvalidValue;
    if (d->d != 64 && d->d != 128) return hipErrorInvalidValue;
    if (d->in_dtype != FA_DTYPE_F16 && d->in_dtype != FA_DTYPE_BF16) return hipErrorInvalidValue;
    if (d->out_dtype != FA_OUT_F32 && d->out_dtype != FA_OUT_SAME) return hipErrorInvalidValue;
    if (d->window < 0) return hipErrorInvalidValue;
    if (!(d->softcap >= 0.0f) || isinf(d->softcap)) return hipErrorInvalidValue;   // negative, NaN or inf
    const long long Hq = (long long)d->Hkv * d->G;                                          // < 2^62
    if (Hq > 0x7FFFFFFFll || (unsigned __int128)Hq * (unsigned)d->B > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // the capacity: the paged decode entries' conditions on the page geometry, or a positive Ncap
    int Ncap = d->Ncap, lg_page = 0;
    if (d->block_table) {
        lg_page = page_log2(d->page_size);
        if (lg_page < 0 || d->num_pages <= 0 || d->max_pages <= 0) return hipErrorInvalidValue;
        if ((long long)d->max_pages * d->page_size > 0x7FFFFFFFll) return hipErrorInvalidValue;   // the capacity is an int
        Ncap = d->max_pages * d->page_size;
    }
    if (Ncap <= 0) return hipErrorInvalidValue;
    const unsigned es = d->out_dtype == FA_OUT_F32 ? 4u : 2u;
    // K, V: the packed entry's check on what one descriptor spans, the Ncap rows of d elements of one (sequence, head) -- Ncap * d * 2
    // bytes fit 32 bits.  Paged, that bounds a tile's byte offset before it is reduced to the page, hence the page-head block too
    if (!varlen_tensor_ok(d->Q, d->total_q, (int)Hq, d->d, d->q_stride_t, d->q_stride_h, 2u) ||
        !varlen_tensor_ok(d->K, Ncap, 1, d->d, d->d, 0, 2u) || !varlen_tensor_ok(d->V, Ncap, 1, d->d, d->d, 0, 2u) ||
        !varlen_tensor_ok(d->O, d->total_q, (int)Hq, d->d, d->o_stride_t, d->o_stride_h, es))
        return hipErrorInvalidValue;
    // block slots: floor(total_q / BM) + B per query head, whatever the vectors hold
    const long long nslots = (long long)d->total_q / kVarlenRows + d->B;
    if (nslots * Hq > 0x7FFFFFFFll) return hipErrorInvalidValue;
    static_cast<VarlenArgs&>(a) = {static_cast<const uint16_t*>(d->Q), static_cast<const uint16_t*>(d->K),
                                   static_cast<const uint16_t*>(d->V), d->O, d->lse, d->cu_seqlens_q, nullptr, d->B, d->Hkv, d->G,
                                   d->total_q, Ncap, (unsigned)nslots, d->q_stride_t, d->q_stride_h, (long long)d->d,
                                   (long long)Ncap * d->d, (long long)d->d, (long long)Ncap * d->d, d->o_stride_t, d->o_stride_h,
                                   host_scale_log2e(d->scale)};
    a.sinks = d->sinks;
    // "no window" and every W that no sequence can feel run as total_q + Ncap, which masks nothing (lo_i <= Lk_b - W <= 0) and keeps
    // the kernel's 32-bit limits from wrapping: total_q and Ncap are below 2^26 each by the 32-bit offset checks above, so
    // |shift + 1 + row| <= 2^26 and window <= 2^27
    const long long wmax = (long long)d->total_q + Ncap;
    a.window = (int)(d->window == 0 || d->window > wmax ? wmax : d->window);
    a.cap2 = d->softcap * kLog2e;
    a.cap_rk = d->softcap > 0.0f ? 2.0f / d->softcap : 0.0f;
    a.seqlens_k = d->seqlens_k;
    a.table = d->block_table;
    a.max_pages = d->block_table ? d->max_pages : 0;
    a.num_pages = d->block_table ? d->num_pages : 0;
    a.lg_page = lg_page;
    grid = dim3((unsigned)(nslots * Hq));
    return hipSuccess;
}

hipError_t varlen_cache_dispatch(const fa_varlen_kvcache_desc* d)
{
    VarlenCacheArgs a;
    dim3 grid;
    const hipError_t e = varlen_cache_check(d, a, grid);
    if (e != hipSuccess) return e;
    // all three options off: the plain kernels, as fa_forward_varlen_ex hands such a call to fa_forward_varlen
    if (!d->sinks && d->window == 0 && d->softcap == 0.0f) return varlen_cache_launch<false>(d, a, grid);
    return varlen_cache_logits_launch(d, &a, grid.x);
}

}  // namespace fa
