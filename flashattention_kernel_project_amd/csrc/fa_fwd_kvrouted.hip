// fa_fwd_kvrouted.hip -- fa_kvcache_attend_varlen: one attention call for a batch that packs prompt chunks beside one-token decodes,
// each sequence routed ON THE DEVICE to the stream that suits its row count.  With T = max_q and span_b the clamped row count of
// sequence b: 1 <= span_b <= T is SHORT and runs on the packed split-KV stream, span_b > T is LONG and runs on the tiled varlen cache
// kernel.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md 7.20.  This unit holds the hand-over (both entries' checks
// on the one descriptor, then the launches) and owns the SHORT half's 16-bit kernels, level kRouted.  The fp8 forms of
// the SHORT half are in fa_fwd_kvrouted_fp8.hip, the LONG half's kernels in fa_fwd_varlen_cache_routed.hip and _routed_fp8.hip.
#include "fa_fwd_kvdecode.hpp"
#include "fa_fwd_varlen_kernel.hpp"   // varlen_cache_check(), the argument structures

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kRouted, false, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kRouted, false, true>(const KvDecodeArgs&, int);

// Both sets of checks once, then the parts.  The descriptor-to-VarlenCacheArgs mapping is varlen_cache_check's own: the fields go
// through the descriptor that entry takes, so what it refuses is refused here and window 0 maps as it maps it.
hipError_t kvattend_dispatch(const fa_kvdecode_varlen_desc* desc, int parts)
{
    if (parts < 1 || parts > 3) return hipErrorInvalidValue;
    KvPackedRows rows_of;
    KvDecodeArgs d;
    int lg_page;
    hipError_t bad = kvpacked_check(desc, nullptr, rows_of, d, lg_page);
    if (bad != hipSuccess) return bad;
    if (desc->causal != 1 || !desc->seqlens_k) return hipErrorInvalidValue;
    const fa_varlen_kvcache_desc vd = {sizeof(fa_varlen_kvcache_desc), desc->Q, desc->O, desc->lse, desc->K, desc->V, desc->cu_seqlens_q,
                                       desc->seqlens_k, desc->block_table, desc->B, desc->Hkv, desc->G, desc->d, desc->total_q, desc->Ncap,
                                       desc->num_pages, desc->page_size, desc->max_pages, desc->q_stride_t, desc->q_stride_h,
                                       desc->o_stride_t, desc->o_stride_h, desc->scale, desc->causal, desc->in_dtype, desc->out_dtype,
                                       desc->sinks, desc->window, desc->softcap, desc->stream};
    VarlenCacheFp8Args va;
    dim3 grid;
    bad = varlen_cache_check(&vd, va, grid);
    if (bad != hipSuccess) return bad;
    va.k_scale = desc->k_scale;
    va.v_scale = desc->v_scale;
    // what the SHORT half's launcher refuses, ahead of any launch and whichever parts run: its grid and its workspace
    const KvCacheArgs& a = d.p.c;
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq, span = kvdecode_span(d);
    const int S = split_count(BH, rows, span);
    if ((long long)BH * ((rows + split::kRows - 1) / split::kRows) * S > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, span, a.D))) return hipErrorInvalidValue;
    if (parts & FA_ATTEND_SHORT) {
        d.level = KvLevel::kRouted;
        bad = kvdecode_route(d, lg_page);
        if (bad != hipSuccess) return bad;
    }
    // with total_q <= T no sequence can be LONG: a rule on host integers, so a captured graph stays valid
    if ((parts & FA_ATTEND_LONG) && desc->total_q > desc->max_q)
        return d.fp8 ? varlen_cache_routed_launch8(&vd, &va, grid.x, desc->max_q)
                     : varlen_cache_routed_launch16(&vd, static_cast<const VarlenCacheArgs*>(&va), grid.x, desc->max_q);
    return hipSuccess;
}

}  // namespace fa
