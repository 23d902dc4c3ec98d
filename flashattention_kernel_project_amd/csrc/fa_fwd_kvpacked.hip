// fa_fwd_kvpacked.hip -- token-packed (cu_seqlens) split-KV decode against a 16-bit cache, contiguous and paged
// (fa_kvcache_decode_varlen): the streams of fa_fwd_kvragged.hip with Q, O and lse in the packed layout of fa_forward_varlen_kvcache
// and each sequence's rows cut from cu_seqlens_q on the device.  DESIGN.md section 7.17 has the reasoning.  Owns the 16-bit kernels of level kPacked
// (DESIGN.md 7.21); the fp8 forms are in fa_fwd_kvpacked_fp8.hip.  Also here, for both units and for levels kTree and kRouted: the
// entry's checks.
#include "fa_fwd_kvdecode.hpp"
#include "fa_fwd_varlen_kernel.hpp"   // varlen_tensor_ok()

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kPacked, false, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kPacked, false, true>(const KvDecodeArgs&, int);

// what the descriptor alone can get wrong (the rule of fa_kvcache_decode's descriptor, with one size only)
static bool kvpacked_desc_ok(const fa_kvdecode_varlen_desc* desc)
{
    if (!desc || desc->size != sizeof(fa_kvdecode_varlen_desc)) return false;
    if (desc->kv_dtype != FA_KV_16BIT && desc->kv_dtype != FA_KV_FP8_E4M3) return false;
    return desc->kv_dtype == FA_KV_FP8_E4M3 || (!desc->k_scale && !desc->v_scale);   // a 16-bit cache has no scales
}

size_t kvpacked_workspace_bytes(const fa_kvdecode_varlen_desc* desc)
{
    if (!kvpacked_desc_ok(desc)) return 0;
    if (desc->block_table)
        return kvpaged_window_workspace_bytes(desc->B, desc->Hkv, desc->G, desc->max_q, desc->max_pages, desc->page_size, desc->d, desc->window);
    return kvwindow_workspace_bytes(desc->B, desc->Hkv, desc->G, desc->max_q, desc->Ncap, desc->d, desc->window);
}

// The kernels address one (sequence, K/V head) view -- up to max_q token rows over the G heads of a group -- through ONE descriptor
// with 32-bit offsets, and a lane past the live rows uses the view's size as its offset, plus up to 2 * d bytes of its columns.  The
// bound is taken over the whole head axis, whatever the group: (rows - 1) * stride_t + Hq * stride_h + d elements, with 512 bytes to
// spare.
static bool packed_view_ok(int max_q, int total, long long Hq, int d, long long st, long long sh, unsigned es)
{
    const int rows = max_q < total ? max_q : total;
    const unsigned __int128 end = ((unsigned __int128)(rows - 1) * (unsigned long long)st + (unsigned __int128)Hq * (unsigned long long)sh +
                                   (unsigned)d) * es + 512u;
    return end <= 0xFFFFFFFFull;
}

// The checks of kvdecode_dispatch (fa_fwd_kvcache.hip) with Nq = max_q, then the packed tensors'; the level is kPacked, or kTree with
// a tree_mask (fa_kvcache_decode_varlen_ex; null: none), which adds the mask's own checks.
// The checks stand alone (kvpacked_check) because fa_kvcache_attend_varlen runs them too, on the same descriptor.
hipError_t kvpacked_check(const fa_kvdecode_varlen_desc* desc, const unsigned long long* tree_mask, KvPackedRows& rows_of, KvDecodeArgs& d,
                          int& lg_page)
{
    if (!kvpacked_desc_ok(desc)) return hipErrorInvalidValue;
    // the words take the triangle's place, one bit per token of the step; the kernels load them as 8-byte words
    if (tree_mask && (desc->causal != 1 || desc->max_q > 64 || (reinterpret_cast<uintptr_t>(tree_mask) & 7u))) return hipErrorInvalidValue;
    if (!desc->cu_seqlens_q || desc->total_q <= 0 || desc->max_q <= 0) return hipErrorInvalidValue;
    if (desc->window < 0) return hipErrorInvalidValue;
    if (!(desc->softcap >= 0.0f) || __builtin_isinf(desc->softcap)) return hipErrorInvalidValue;   // negative, NaN or inf
    const bool paged = desc->block_table != nullptr;
    rows_of = {desc->cu_seqlens_q, desc->total_q, desc->q_stride_t, desc->q_stride_h, desc->o_stride_t, desc->o_stride_h, tree_mask};
    d = {.p = {.c = {desc->Q, desc->K, desc->V, desc->O, desc->lse, desc->seqlens_k, desc->B, desc->Hkv, desc->G, desc->max_q,
                     paged ? 0 : desc->Ncap, desc->d, desc->scale, desc->causal, desc->in_dtype, desc->out_dtype,
                     desc->workspace, desc->workspace_bytes, static_cast<hipStream_t>(desc->stream)},
               .table = desc->block_table, .num_pages = paged ? desc->num_pages : 0,
               .page_size = paged ? desc->page_size : 0, .max_pages = paged ? desc->max_pages : 0},
         .k_scale = desc->k_scale, .v_scale = desc->v_scale, .window = desc->window, .paged = paged,
         .fp8 = desc->kv_dtype == FA_KV_FP8_E4M3, .sinks = desc->sinks, .softcap = desc->softcap, .seqlens_q = nullptr,
         .packed = &rows_of, .level = tree_mask ? KvLevel::kTree : KvLevel::kPacked};
    lg_page = 0;
    if (!paged) {
        const hipError_t bad = kvcache_check(d.p.c);
        if (bad != hipSuccess) return bad;
    } else {
        KvPagedArgs with_capacity;
        const hipError_t bad = kvpaged_check(d.p, with_capacity, lg_page);
        if (bad != hipSuccess) return bad;
        d.p = with_capacity;
    }
    const long long Hq = (long long)desc->Hkv * desc->G;   // B * Hkv and G * max_q fit an int (the checks above)
    if (Hq > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const unsigned es = desc->out_dtype == FA_OUT_F32 ? 4u : 2u;
    if (!varlen_tensor_ok(desc->Q, desc->total_q, (int)Hq, desc->d, desc->q_stride_t, desc->q_stride_h, 2u) ||
        !varlen_tensor_ok(desc->O, desc->total_q, (int)Hq, desc->d, desc->o_stride_t, desc->o_stride_h, es))
        return hipErrorInvalidValue;
    if (!packed_view_ok(desc->max_q, desc->total_q, Hq, desc->d, desc->q_stride_t, desc->q_stride_h, 2u) ||
        !packed_view_ok(desc->max_q, desc->total_q, Hq, desc->d, desc->o_stride_t, desc->o_stride_h, es))
        return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t kvpacked_dispatch(const fa_kvdecode_varlen_desc* desc, const unsigned long long* tree_mask)
{
    KvPackedRows rows_of;
    KvDecodeArgs d;
    int lg_page;
    const hipError_t bad = kvpacked_check(desc, tree_mask, rows_of, d, lg_page);
    return bad != hipSuccess ? bad : kvdecode_route(d, lg_page);
}

}  // namespace fa
