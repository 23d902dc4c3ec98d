// fa_fwd_kvrouted.hip -- fa_kvcache_attend_varlen: one attention call for a batch that packs prompt chunks beside one-token decodes,
// each sequence routed ON THE DEVICE to the stream that suits its row count.  With T = max_q and span_b the clamped row count of
// sequence b: 1 <= span_b <= T is SHORT and runs on the packed split-KV stream, span_b > T is LONG and runs on the tiled varlen cache
// kernel.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md 7.20.  This unit holds the hand-over (both entries' checks
// on the one descriptor, then the launches), the SHORT half's 16-bit kernels -- the RoutedArgs<PackedArgs<...>> instantiations of
// fa_fwd_split_kernel.hpp, launched through fa_fwd_kvdecode.hpp -- and the RoutedLse merge of both cache types.  The fp8 forms of the
// SHORT half are in fa_fwd_kvrouted_fp8.hip, the LONG half's kernels in fa_fwd_varlen_cache_routed.hip and _routed_fp8.hip.
#include "fa_fwd_kvdecode.hpp"
#include "fa_fwd_varlen_kernel.hpp"   // varlen_cache_check(), the argument structures

namespace fa {

hipError_t kvrouted_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<RoutedArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<CacheArgs>>>>>>(d, lg_page)
                    : dispatch_kvdecode<RoutedArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<PagedArgs>>>>>>(d, lg_page);
}

// kvpacked_combine with the routed row count: the RoutedLse instantiations of the merge kernel
hipError_t kvrouted_combine(const void* ws, void* O, float* lse, const float* sinks, const KvPackedRows& rows_of, int BH, int rows,
                            int Hkv, int Nq, int D, int S, int in_dtype, int out_dtype, hipStream_t stream)
{
    const long long out_rows = (long long)BH * rows;
    if (out_rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
        FA_LAUNCH((fa_split_combine_kernel<decltype(t), decltype(f32)::value, true, RoutedLse>), dim3((unsigned)out_rows), dim3(64), 0,
                  stream, static_cast<const float*>(ws), O, BH, rows, D, S,
                  RoutedLse{{lse, sinks, rows_of.cu_q, Hkv, Nq, rows_of.total_q, rows_of.o_st, rows_of.o_sh}});
        return launch_status();
    });
}

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
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq, span = window_span_cap(a.Nq, a.Ncap, d.window);
    const int S = split_count(BH, rows, span);
    if ((long long)BH * ((rows + split::kRows - 1) / split::kRows) * S > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, span, a.D))) return hipErrorInvalidValue;
    if (parts & FA_ATTEND_SHORT) {
        bad = d.fp8 ? kvrouted_fp8_decode(d, lg_page) : kvrouted_decode(d, lg_page);
        if (bad != hipSuccess) return bad;
    }
    // with total_q <= T no sequence can be LONG: a rule on host integers, so a captured graph stays valid
    if ((parts & FA_ATTEND_LONG) && desc->total_q > desc->max_q)
        return d.fp8 ? varlen_cache_routed_launch8(&vd, &va, grid.x, desc->max_q)
                     : varlen_cache_routed_launch16(&vd, static_cast<const VarlenCacheArgs*>(&va), grid.x, desc->max_q);
    return hipSuccess;
}

}  // namespace fa
