// fa_fwd_kv256.hip -- fa_kvcache_decode_d256: token-packed split-KV decode against a 16-bit KV cache at head dimension 256 (the
// Gemma-2 / Gemma-3 head), contiguous and paged, with the causal tail, the sliding window and the soft-cap.  The descriptor is
// fa_kvcache_decode_varlen's as it is; the entries are new because that one keeps refusing d = 256.  The kernel template, the merge
// kernel and the launcher are in fa_fwd_kv256_kernel.hpp; this unit owns the host checks and the plan and instantiates the kernels.
// fa_kvcache_decode_d256_fp8 runs the same checks and the same plan here; its kernels are fa_fwd_kv256_fp8.hip's.
// DESIGN.md sections 7.25 and 7.27, profiles/kv256_decode.txt.
#include "fa_fwd_kv256_kernel.hpp"
#include "fa_fwd_varlen_kernel.hpp"   // varlen_tensor_ok()

namespace fa {

namespace {

// What the checks leave behind: the capacity, the window the kernel takes, the split count and the grid, from host integers alone.
struct Kv256Plan {
    int cap, lg_page, window, S, nqb;
    bool paged;
};

// The number of splits for a shape: enough workgroups for two rounds of the two a CU holds on a 256-CU device, but at least four
// 64-key tiles per split.  The split stream's rule (split_count) on this kernel's 32-row blocks; span: the longest key range a
// sequence can stream.
int kv256_split_count(long long base, int span)
{
    const int tiles = (span + kv256::kTile - 1) / kv256::kTile;
    constexpr int target = 1024, min_tiles = 4;
    long long s = (target + base - 1) / base;
    if (s > tiles / min_tiles) s = tiles / min_tiles;
    if (s < 1) s = 1;
    const int chunk_tiles = (int)((tiles + s - 1) / s);   // every split holds at least one tile of a full sequence
    return (tiles + chunk_tiles - 1) / chunk_tiles;
}

// the bound of fa_kvcache_decode_varlen on one (sequence, K/V head) view: its bytes fit 32 bits with 512 to spare
bool kv256_view_ok(int max_q, int total, long long Hq, long long st, long long sh, unsigned es)
{
    const int rows = max_q < total ? max_q : total;
    const unsigned __int128 end = ((unsigned __int128)(rows - 1) * (unsigned long long)st + (unsigned __int128)Hq * (unsigned long long)sh +
                                   (unsigned)kv256::kD) * es + 512u;
    return end <= 0xFFFFFFFFull;
}

// every check that needs no workspace: fa_kvcache_decode_varlen's, with d == 256, no sinks and, for the 16-bit entry, a 16-bit cache
// without scales, for the fp8 entry an e4m3fn cache whose scales are null or 4-byte aligned; on success the plan is filled in.
// Nothing of the plan depends on `fp8`: the capacity bound stays that of 512-byte rows, and so do the splits and the workspace.
bool kv256_plan(const ::fa_kvdecode_varlen_desc* d, int num_splits, bool fp8, Kv256Plan& p)
{
    if (!d || d->size != sizeof(fa_kvdecode_varlen_desc)) return false;
    if (d->sinks) return false;
    if (!fp8 && (d->kv_dtype != FA_KV_16BIT || d->k_scale || d->v_scale)) return false;
    if (fp8 && (d->kv_dtype != FA_KV_FP8_E4M3 || ((reinterpret_cast<uintptr_t>(d->k_scale) | reinterpret_cast<uintptr_t>(d->v_scale)) & 3u)))
        return false;
    if (d->d != kv256::kD) return false;
    if (!d->Q || !d->K || !d->V || !d->O || !d->cu_seqlens_q) return false;
    if (d->B <= 0 || d->Hkv <= 0 || d->G <= 0 || d->total_q <= 0 || d->max_q <= 0) return false;
    if (d->causal != 0 && d->causal != 1) return false;
    if (d->in_dtype != FA_DTYPE_F16 && d->in_dtype != FA_DTYPE_BF16) return false;
    if (d->out_dtype != FA_OUT_F32 && d->out_dtype != FA_OUT_SAME) return false;
    if (d->window < 0) return false;
    if (!(d->softcap >= 0.0f) || __builtin_isinf(d->softcap)) return false;   // negative, NaN or inf
    const long long bh = (long long)d->B * d->Hkv, rows_seq = (long long)d->G * d->max_q, Hq = (long long)d->Hkv * d->G;
    if (bh > 0x7FFFFFFFll || rows_seq > 0x7FFFFFFFll || Hq > 0x7FFFFFFFll) return false;
    p.paged = d->block_table != nullptr;
    p.lg_page = 0;
    if (!p.paged) {
        if (d->Ncap <= 0) return false;
        p.cap = d->Ncap;
    } else {
        p.lg_page = page_log2(d->page_size);
        if (p.lg_page < 0 || d->num_pages <= 0 || d->max_pages <= 0) return false;
        if ((long long)d->max_pages * d->page_size > 0x7FFFFFFFll) return false;   // the capacity is an int
        p.cap = d->max_pages * d->page_size;
    }
    // the decode entries' bound on a head's bytes; it keeps every key index and limit of the kernel far inside an int
    if (((unsigned long long)p.cap + kv256::kTile) * kv256::kRowBytes >= (1ull << 32)) return false;
    const unsigned es = d->out_dtype == FA_OUT_F32 ? 4u : 2u;
    if (!varlen_tensor_ok(d->Q, d->total_q, (int)Hq, kv256::kD, d->q_stride_t, d->q_stride_h, 2u) ||
        !varlen_tensor_ok(d->O, d->total_q, (int)Hq, kv256::kD, d->o_stride_t, d->o_stride_h, es))
        return false;
    if (!kv256_view_ok(d->max_q, d->total_q, Hq, d->q_stride_t, d->q_stride_h, 2u) ||
        !kv256_view_ok(d->max_q, d->total_q, Hq, d->o_stride_t, d->o_stride_h, es))
        return false;
    const int tiles = (p.cap + kv256::kTile - 1) / kv256::kTile;
    if (num_splits < 0 || num_splits > tiles) return false;
    // a window that covers the capacity is "every key" for every length, and so is none: the clamp keeps the kernel's ints in range
    p.window = d->window == 0 || d->window > p.cap ? p.cap : d->window;
    const long long nqb = (rows_seq + kv256::kRows - 1) / kv256::kRows, base = bh * nqb;
    p.S = num_splits ? num_splits : kv256_split_count(base, d->window == 0 ? p.cap : window_span_cap(d->max_q, p.cap, d->window));
    if (base * p.S > 0x7FFFFFFFll || bh * rows_seq > 0x7FFFFFFFll) return false;   // the grids
    p.nqb = (int)nqb;
    return true;
}

size_t kv256_ws_bytes(const ::fa_kvdecode_varlen_desc* d, const Kv256Plan& p)
{
    return p.S <= 1 ? 0 : (size_t)d->B * d->Hkv * p.S * p.nqb * kv256::kRows * kv256::kWsRow * sizeof(float);
}

}  // namespace

size_t kv256_workspace_bytes(const ::fa_kvdecode_varlen_desc* d, int num_splits, bool fp8)
{
    Kv256Plan p;
    return kv256_plan(d, num_splits, fp8, p) ? kv256_ws_bytes(d, p) : 0;
}

hipError_t kv256_dispatch(const ::fa_kvdecode_varlen_desc* d, int num_splits, bool fp8)
{
    Kv256Plan p;
    if (!kv256_plan(d, num_splits, fp8, p)) return hipErrorInvalidValue;
    const size_t need = kv256_ws_bytes(d, p);
    if (need && (!d->workspace || d->workspace_bytes < need || (reinterpret_cast<uintptr_t>(d->workspace) & 15u)))
        return hipErrorInvalidValue;
    const kv256::Dev a = {static_cast<const uint16_t*>(d->Q), d->O, d->lse, static_cast<const char*>(d->K), static_cast<const char*>(d->V),
                          static_cast<float*>(d->workspace), d->cu_seqlens_q, d->seqlens_k, d->block_table, d->B, d->Hkv, d->G, d->total_q,
                          d->max_q, p.cap, p.paged ? d->max_pages : 0, p.paged ? d->num_pages : 0, p.lg_page, d->q_stride_t, d->q_stride_h,
                          d->o_stride_t, d->o_stride_h, host_scale_log2e(d->scale), d->softcap * kLog2e,
                          d->softcap > 0.0f ? 2.0f / d->softcap : 0.0f, d->causal, p.window, p.S, p.nqb, d->k_scale, d->v_scale};
    hipStream_t stream = static_cast<hipStream_t>(d->stream);
    if (fp8) return kv256_launch_fp8(a, d->in_dtype == FA_DTYPE_BF16, d->out_dtype == FA_OUT_F32, p.paged, stream);
    return with_types(d->in_dtype, d->out_dtype,
                      [&](auto t, auto f32) { return kv256_launch<decltype(t), decltype(f32)::value, false>(a, p.paged, stream); });
}

}  // namespace fa
