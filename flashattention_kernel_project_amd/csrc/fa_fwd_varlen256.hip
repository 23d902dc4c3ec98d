// fa_fwd_varlen256.hip -- fa_forward_varlen_d256, fa_forward_varlen_kvcache_d256 and the checks of
// fa_forward_varlen_kvcache_d256_fp8 (its kernels: fa_fwd_varlen256_fp8.hip): the variable-length prefill at head dimension
// 256 (the Gemma-2 / Gemma-3 head), K/V token-packed or in the KV cache, contiguous or paged, with the causal mask, the sliding
// window and the soft-cap.  The descriptors are fa_forward_varlen_ex's and fa_forward_varlen_kvcache's as they are; the entries are
// new because those keep refusing d = 256.  The kernel template is fa_fwd_varlen256_kernel.hpp's; this unit owns the host checks and
// the 12 instantiations (type x output x {packed, contiguous, paged}).  DESIGN.md section 7.26, profiles/varlen_d256.txt.
#include "fa_fwd_varlen256_kernel.hpp"

namespace fa {

namespace {

// what the two descriptors share: the shape, the types, Q and O, the grid; on success the common kernel arguments
template <typename Desc> bool varlen256_common(const Desc* d, varlen256::Dev& a, dim3& grid)
{
    if (d->B <= 0 || d->Hkv <= 0 || d->G <= 0 || d->total_q <= 0) return false;
    if (d->d != varlen256::kD) return false;
    if (d->in_dtype != FA_DTYPE_F16 && d->in_dtype != FA_DTYPE_BF16) return false;
    if (d->out_dtype != FA_OUT_F32 && d->out_dtype != FA_OUT_SAME) return false;
    const long long Hq = (long long)d->Hkv * d->G;                                          // < 2^62
    if (Hq > 0x7FFFFFFFll || (unsigned __int128)Hq * (unsigned)d->B > 0x7FFFFFFFull) return false;
    const unsigned es = d->out_dtype == FA_OUT_F32 ? 4u : 2u;
    if (!varlen_tensor_ok(d->Q, d->total_q, (int)Hq, d->d, d->q_stride_t, d->q_stride_h, 2u) ||
        !varlen_tensor_ok(d->O, d->total_q, (int)Hq, d->d, d->o_stride_t, d->o_stride_h, es))
        return false;
    // block slots: floor(total_q / 128) + B per query head, whatever the vectors hold
    const long long nslots = (long long)d->total_q / kVarlenRows + d->B;
    if (nslots * Hq > 0x7FFFFFFFll) return false;
    a = {};
    a.Q = static_cast<const uint16_t*>(d->Q);
    a.O = d->O;
    a.lse = d->lse;
    a.K = static_cast<const char*>(d->K);
    a.V = static_cast<const char*>(d->V);
    a.cu_q = d->cu_seqlens_q;
    a.B = d->B, a.Hkv = d->Hkv, a.G = d->G, a.total_q = d->total_q;
    a.nslots = (unsigned)nslots;
    a.q_st = d->q_stride_t, a.q_sh = d->q_stride_h, a.o_st = d->o_stride_t, a.o_sh = d->o_stride_h;
    a.scale_log2e = host_scale_log2e(d->scale);
    a.causal = d->causal != 0;
    grid = dim3((unsigned)(nslots * Hq));
    return true;
}

// the two options: "no window" and every W that no sequence can feel run as total_q + total_k, which masks nothing (lo_i <= Lk_b - W
// <= 0) and keeps the kernel's 32-bit limits from wrapping: the totals are below 2^26 each by the 32-bit offset checks
bool varlen256_options(int window, float softcap, varlen256::Dev& a)
{
    if (window < 0) return false;
    if (!(softcap >= 0.0f) || __builtin_isinf(softcap)) return false;   // negative, NaN or inf
    const long long wmax = (long long)a.total_q + a.total_k;
    a.window = (int)(window == 0 || window > wmax ? wmax : window);
    a.cap2 = softcap * kLog2e;
    a.cap_rk = softcap > 0.0f ? 2.0f / softcap : 0.0f;
    return true;
}

// The cache entries' one body.  fp8: K and V address one e4m3fn byte per element (the tensor checks take an element size of 1; the
// capacity bound stays the 16-bit one, so both entries accept the same descriptors) and the scales are device pointers, null or
// 4-byte aligned.
hipError_t varlen256_cache_run(const ::fa_varlen_kvcache_desc* d, bool fp8, const float* k_scale, const float* v_scale)
{
    if (!d || d->size != sizeof(fa_varlen_kvcache_desc)) return hipErrorInvalidValue;
    if (d->sinks) return hipErrorInvalidValue;   // no sinks at d = 256
    if (!d->cu_seqlens_q || !d->seqlens_k) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3u) return hipErrorInvalidValue;
    varlen256::Dev a;
    dim3 grid;
    if (!varlen256_common(d, a, grid)) return hipErrorInvalidValue;
    // the capacity: the paged decode entries' conditions on the page geometry, or a positive Ncap
    int Ncap = d->Ncap;
    if (d->block_table) {
        a.lg_page = page_log2(d->page_size);
        if (a.lg_page < 0 || d->num_pages <= 0 || d->max_pages <= 0) return hipErrorInvalidValue;
        if ((long long)d->max_pages * d->page_size > 0x7FFFFFFFll) return hipErrorInvalidValue;   // the capacity is an int
        Ncap = d->max_pages * d->page_size;
        a.max_pages = d->max_pages;
        a.num_pages = d->num_pages;
    }
    if (Ncap <= 0) return hipErrorInvalidValue;
    // the d = 256 decode's bound on a head's bytes; it keeps every key index and limit of the kernel far inside an int
    if (((unsigned long long)Ncap + varlen256::kTile) * varlen256::kRowBytes >= (1ull << 32)) return hipErrorInvalidValue;
    const unsigned es = fp8 ? 1u : 2u;
    if (!varlen_tensor_ok(d->K, Ncap, 1, d->d, d->d, 0, es) || !varlen_tensor_ok(d->V, Ncap, 1, d->d, d->d, 0, es))
        return hipErrorInvalidValue;
    a.seqlens = d->seqlens_k;
    a.table = d->block_table;
    a.total_k = Ncap;
    a.k_scale = k_scale;
    a.v_scale = v_scale;
    if (!varlen256_options(d->window, d->softcap, a)) return hipErrorInvalidValue;
    if (fp8) return varlen256_launch_fp8(a, grid, d->in_dtype, d->out_dtype, d->block_table != nullptr, d->stream);
    return d->block_table ? varlen256_launch<varlen256::kPaged, false>(a, grid, d->in_dtype, d->out_dtype, d->stream)
                          : varlen256_launch<varlen256::kContig, false>(a, grid, d->in_dtype, d->out_dtype, d->stream);
}

}  // namespace

hipError_t varlen256_dispatch(const ::fa_varlen_desc* d, const ::fa_varlen_opts* o)
{
    if (!d || d->size != sizeof(fa_varlen_desc)) return hipErrorInvalidValue;
    if (o && (o->size != sizeof(fa_varlen_opts) || o->sinks)) return hipErrorInvalidValue;   // no sinks at d = 256
    if (!d->cu_seqlens_q || !d->cu_seqlens_k || d->total_k <= 0) return hipErrorInvalidValue;
    varlen256::Dev a;
    dim3 grid;
    if (!varlen256_common(d, a, grid)) return hipErrorInvalidValue;
    if (!varlen_tensor_ok(d->K, d->total_k, d->Hkv, d->d, d->k_stride_t, d->k_stride_h, 2u) ||
        !varlen_tensor_ok(d->V, d->total_k, d->Hkv, d->d, d->v_stride_t, d->v_stride_h, 2u))
        return hipErrorInvalidValue;
    a.cu_k = d->cu_seqlens_k;
    a.total_k = d->total_k;
    a.k_st = d->k_stride_t, a.k_sh = d->k_stride_h, a.v_st = d->v_stride_t, a.v_sh = d->v_stride_h;
    if (!varlen256_options(o ? o->window : 0, o ? o->softcap : 0.0f, a)) return hipErrorInvalidValue;
    return varlen256_launch<varlen256::kPacked, false>(a, grid, d->in_dtype, d->out_dtype, d->stream);
}

hipError_t varlen256_cache_dispatch(const ::fa_varlen_kvcache_desc* d) { return varlen256_cache_run(d, false, nullptr, nullptr); }

hipError_t varlen256_cache_dispatch_fp8(const ::fa_varlen_kvcache_desc* d, const float* k_scale, const float* v_scale)
{
    return varlen256_cache_run(d, true, k_scale, v_scale);
}

}  // namespace fa
