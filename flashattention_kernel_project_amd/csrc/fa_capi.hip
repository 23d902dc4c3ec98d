// fa_capi.hip -- extern "C" launchers declared in include/fa_mi355.h.
#include <hip/hip_runtime.h>
#include "../../include/fa_mi355.h"
#include "fa_dispatch.hpp"

// The library is built with -fvisibility=hidden: only the entry points below leave it.
#define FA_EXPORT __attribute__((visibility("default")))

extern "C" {

#ifdef FA_EXPERIMENTS
// ---- libfa_mi355_exp.so only (make experimental): measurement entry points, not in the public header ----
// per-block pass ids of the fa_fwd_rp16 kernels (see g_rp16_pass_ids); nullptr switches the recording off again
FA_EXPORT int fa_lab_rp16_pass_ids(unsigned* dev_ids) { return (int)fa::rp16_set_pass_ids(dev_ids); }

// compute / stage-wait / barrier time of the interleaved kernel.
FA_EXPORT int fa_debug_il_times(const void* Q, const void* K, const void* V, void* O,
                      int BH, int N, float scale, unsigned long long* diag, int waves, void* stream)
{
    return (int)fa::il_diag_dispatch(Q, K, V, O, BH, N, scale, diag, waves, static_cast<hipStream_t>(stream));
}

#endif  // FA_EXPERIMENTS

// 1 when this build carries the experimental A/B kernels (the rows of the algo table in fa_fwd_kernels.hip under FA_EXPERIMENTS), else 0.
FA_EXPORT int fa_mi355_has_experiments(void)
{
#ifdef FA_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

FA_EXPORT int flashattn_forward_wmma(const void* Q, const void* K, const void* V, float* O,
                           int BH, int N, int D, float scale, void* stream)
{
    return (int)fa::forward_dispatch({Q, K, V, O, BH, N, D, scale, FA_DTYPE_F16, FA_OUT_F32, static_cast<hipStream_t>(stream)},
                                     FA_ALGO_AUTO);
}

FA_EXPORT int fa_forward_ex(const void* Q, const void* K, const void* V, void* O,
                  int B, int H, int N, int d, float scale,
                  int in_dtype, int out_dtype, int algo, void* stream)
{
    if (B <= 0 || H <= 0 || (long long)B * H > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    if (out_dtype != FA_OUT_F32 && out_dtype != FA_OUT_SAME) return (int)hipErrorInvalidValue;
    // (an algo id the table in fa_fwd_kernels.hip has no row for is rejected there: no range is restated here)
    return (int)fa::forward_dispatch({Q, K, V, O, B * H, N, d, scale, in_dtype, out_dtype, static_cast<hipStream_t>(stream)}, algo);
}

FA_EXPORT int fa_forward(const void* Q, const void* K, const void* V, void* O,
               int B, int H, int N, int d, float scale,
               int in_dtype, int out_dtype, void* stream)
{
    return fa_forward_ex(Q, K, V, O, B, H, N, d, scale, in_dtype, out_dtype, FA_ALGO_AUTO, stream);
}

FA_EXPORT int fa_forward_causal(const void* Q, const void* K, const void* V, void* O,
                      int B, int H, int N, int d, float scale,
                      int in_dtype, int out_dtype, int algo, void* stream)
{
    if (B <= 0 || H <= 0 || (long long)B * H > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    if (out_dtype != FA_OUT_F32 && out_dtype != FA_OUT_SAME) return (int)hipErrorInvalidValue;
    return (int)fa::forward_causal_dispatch({Q, K, V, O, B * H, N, d, scale, in_dtype, out_dtype, static_cast<hipStream_t>(stream)}, algo);
}

FA_EXPORT size_t fa_forward_splitkv_workspace_bytes(int B, int H, int Nq, int Nk, int d)
{
    if (B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0 || d <= 0 || (long long)B * H > 0x7FFFFFFFll) return 0;
    return fa::split_workspace_bytes(B * H, Nq, Nk, d);
}

FA_EXPORT int fa_forward_splitkv(const void* Q, const void* K, const void* V, void* O,
                       int B, int H, int Nq, int Nk, int d, float scale,
                       int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    if (B <= 0 || H <= 0 || (long long)B * H > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    return (int)fa::split_dispatch(Q, K, V, O, workspace, workspace_bytes, B * H, Nq, Nk, d, scale, in_dtype, out_dtype,
                                   static_cast<hipStream_t>(stream));
}

FA_EXPORT size_t fa_forward_kvcache_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int d)
{
    return fa::kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d);
}

FA_EXPORT int fa_forward_kvcache(const void* Q, const void* Kcache, const void* Vcache, void* O, float* lse, const int* seqlens_k,
                       int B, int Hkv, int G, int Nq, int Ncap, int d, float scale, int causal,
                       int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kcache, Vcache, O, lse, seqlens_k, B, Hkv, G, Nq, Ncap, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)}}});
}

FA_EXPORT size_t fa_forward_kvcache_paged_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int d)
{
    return fa::kvpaged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d);
}

FA_EXPORT int fa_forward_kvcache_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const int* seqlens_k,
                             const int* block_table, int B, int Hkv, int G, int Nq, int num_pages, int page_size, int max_pages,
                             int d, float scale, int causal, int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes,
                             void* stream)
{
    // Ncap (0 here) is set by the dispatcher once max_pages * page_size is known to fit
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kpool, Vpool, O, lse, seqlens_k, B, Hkv, G, Nq, 0, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)},
                                             .table = block_table, .num_pages = num_pages, .page_size = page_size, .max_pages = max_pages},
                                       .paged = true});
}

FA_EXPORT int fa_forward_kvcache_fp8(const void* Q, const void* Kcache, const void* Vcache, void* O, float* lse, const int* seqlens_k,
                           const float* k_scale, const float* v_scale, int B, int Hkv, int G, int Nq, int Ncap, int d, float scale,
                           int causal, int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kcache, Vcache, O, lse, seqlens_k, B, Hkv, G, Nq, Ncap, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)}},
                                       .k_scale = k_scale, .v_scale = v_scale, .fp8 = true});
}

FA_EXPORT int fa_forward_kvcache_paged_fp8(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const int* seqlens_k,
                                 const int* block_table, const float* k_scale, const float* v_scale, int B, int Hkv, int G, int Nq,
                                 int num_pages, int page_size, int max_pages, int d, float scale, int causal, int in_dtype,
                                 int out_dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kpool, Vpool, O, lse, seqlens_k, B, Hkv, G, Nq, 0, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)},
                                             .table = block_table, .num_pages = num_pages, .page_size = page_size, .max_pages = max_pages},
                                       .k_scale = k_scale, .v_scale = v_scale, .paged = true, .fp8 = true});
}

FA_EXPORT size_t fa_forward_kvcache_window_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int d, int window)
{
    return fa::kvwindow_workspace_bytes(B, Hkv, G, Nq, Ncap, d, window);
}

FA_EXPORT size_t fa_forward_kvcache_paged_window_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int d,
                                                                 int window)
{
    return fa::kvpaged_window_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d, window);
}

FA_EXPORT int fa_forward_kvcache_window(const void* Q, const void* Kcache, const void* Vcache, void* O, float* lse, const int* seqlens_k,
                              int B, int Hkv, int G, int Nq, int Ncap, int d, float scale, int causal, int window,
                              int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kcache, Vcache, O, lse, seqlens_k, B, Hkv, G, Nq, Ncap, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)}},
                                       .window = window});
}

FA_EXPORT int fa_forward_kvcache_paged_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse,
                                    const int* seqlens_k, const int* block_table, int B, int Hkv, int G, int Nq, int num_pages,
                                    int page_size, int max_pages, int d, float scale, int causal, int window, int in_dtype,
                                    int out_dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kpool, Vpool, O, lse, seqlens_k, B, Hkv, G, Nq, 0, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)},
                                             .table = block_table, .num_pages = num_pages, .page_size = page_size, .max_pages = max_pages},
                                       .window = window, .paged = true});
}

FA_EXPORT int fa_forward_kvcache_fp8_window(const void* Q, const void* Kcache, const void* Vcache, void* O, float* lse,
                                  const int* seqlens_k, const float* k_scale, const float* v_scale, int B, int Hkv, int G, int Nq,
                                  int Ncap, int d, float scale, int causal, int window, int in_dtype, int out_dtype, void* workspace,
                                  size_t workspace_bytes, void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kcache, Vcache, O, lse, seqlens_k, B, Hkv, G, Nq, Ncap, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)}},
                                       .k_scale = k_scale, .v_scale = v_scale, .window = window, .fp8 = true});
}

FA_EXPORT int fa_forward_kvcache_paged_fp8_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse,
                                        const int* seqlens_k, const int* block_table, const float* k_scale, const float* v_scale,
                                        int B, int Hkv, int G, int Nq, int num_pages, int page_size, int max_pages, int d, float scale,
                                        int causal, int window, int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes,
                                        void* stream)
{
    return (int)fa::kvdecode_dispatch({.p = {.c = {Q, Kpool, Vpool, O, lse, seqlens_k, B, Hkv, G, Nq, 0, d, scale, causal, in_dtype, out_dtype,
                                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream)},
                                             .table = block_table, .num_pages = num_pages, .page_size = page_size, .max_pages = max_pages},
                                       .k_scale = k_scale, .v_scale = v_scale, .window = window, .paged = true, .fp8 = true});
}

// The descriptor form of the eight entries above, plus sinks and softcap.  What the descriptor alone can get wrong is judged here;
// everything else by kvdecode_dispatch, as for the flat entries.
// A descriptor of the size the structure had before seqlens_q was appended is a valid one without the field.
static bool kvdecode_desc_ok(const fa_kvdecode_desc* desc)
{
    if (!desc || (desc->size != sizeof(fa_kvdecode_desc) && desc->size != offsetof(fa_kvdecode_desc, seqlens_q))) return false;
    if (desc->kv_dtype != FA_KV_16BIT && desc->kv_dtype != FA_KV_FP8_E4M3) return false;
    return desc->kv_dtype == FA_KV_FP8_E4M3 || (!desc->k_scale && !desc->v_scale);   // a 16-bit cache has no scales
}

FA_EXPORT size_t fa_kvcache_decode_workspace_bytes(const fa_kvdecode_desc* desc)
{
    if (!kvdecode_desc_ok(desc)) return 0;
    if (desc->block_table)
        return fa::kvpaged_window_workspace_bytes(desc->B, desc->Hkv, desc->G, desc->Nq, desc->max_pages, desc->page_size, desc->d, desc->window);
    return fa::kvwindow_workspace_bytes(desc->B, desc->Hkv, desc->G, desc->Nq, desc->Ncap, desc->d, desc->window);
}

FA_EXPORT int fa_kvcache_decode(const fa_kvdecode_desc* desc)
{
    if (!kvdecode_desc_ok(desc)) return (int)hipErrorInvalidValue;
    const bool paged = desc->block_table != nullptr;
    return (int)fa::kvdecode_dispatch({.p = {.c = {desc->Q, desc->K, desc->V, desc->O, desc->lse, desc->seqlens_k, desc->B, desc->Hkv, desc->G,
                                                   desc->Nq, paged ? 0 : desc->Ncap, desc->d, desc->scale, desc->causal, desc->in_dtype,
                                                   desc->out_dtype, desc->workspace, desc->workspace_bytes,
                                                   static_cast<hipStream_t>(desc->stream)},
                                             .table = desc->block_table, .num_pages = paged ? desc->num_pages : 0,
                                             .page_size = paged ? desc->page_size : 0, .max_pages = paged ? desc->max_pages : 0},
                                       .k_scale = desc->k_scale, .v_scale = desc->v_scale, .window = desc->window, .paged = paged,
                                       .fp8 = desc->kv_dtype == FA_KV_FP8_E4M3, .sinks = desc->sinks, .softcap = desc->softcap,
                                       .seqlens_q = desc->size == sizeof(fa_kvdecode_desc) ? desc->seqlens_q : nullptr});
}

FA_EXPORT int fa_kvcache_append(const void* Knew, const void* Vnew, void* Kcache, void* Vcache, const int* seqlens_k, int* seqlens_out,
                      int B, int Hkv, int Nnew, int Ncap, int d, int dtype, void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kcache, Vcache, seqlens_k, seqlens_out, nullptr, nullptr, nullptr, B, Hkv, Nnew,
                                             Ncap, d, dtype, 0, 0, 0, false, false, static_cast<hipStream_t>(stream)});
}

FA_EXPORT int fa_kvcache_append_paged(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int* seqlens_k,
                            int* seqlens_out, const int* block_table, int B, int Hkv, int Nnew, int num_pages, int page_size,
                            int max_pages, int d, int dtype, void* stream)
{
    // Ncap (0 here) follows from max_pages * page_size once that is known to fit
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kpool, Vpool, seqlens_k, seqlens_out, block_table, nullptr, nullptr, B, Hkv, Nnew,
                                             0, d, dtype, num_pages, page_size, max_pages, true, false, static_cast<hipStream_t>(stream)});
}

FA_EXPORT int fa_kvcache_append_fp8(const void* Knew, const void* Vnew, void* Kcache, void* Vcache, const int* seqlens_k, int* seqlens_out,
                          const float* k_scale, const float* v_scale, int B, int Hkv, int Nnew, int Ncap, int d, int in_dtype,
                          void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kcache, Vcache, seqlens_k, seqlens_out, nullptr, k_scale, v_scale, B, Hkv, Nnew,
                                             Ncap, d, in_dtype, 0, 0, 0, false, true, static_cast<hipStream_t>(stream)});
}

FA_EXPORT int fa_kvcache_append_paged_fp8(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int* seqlens_k,
                                int* seqlens_out, const int* block_table, const float* k_scale, const float* v_scale, int B, int Hkv,
                                int Nnew, int num_pages, int page_size, int max_pages, int d, int in_dtype, void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kpool, Vpool, seqlens_k, seqlens_out, block_table, k_scale, v_scale, B, Hkv, Nnew,
                                             0, d, in_dtype, num_pages, page_size, max_pages, true, true, static_cast<hipStream_t>(stream)});
}

// The _rope forms: the base entry's list with (Q, Qout, rope_cos, rope_sin) before B and (G, rot_dim, max_pos, interleaved) after d;
// the rope fields are the tail of KvAppendArgs.
FA_EXPORT int fa_kvcache_append_rope(const void* Knew, const void* Vnew, void* Kcache, void* Vcache, const int* seqlens_k, int* seqlens_out,
                           const void* Q, void* Qout, const float* rope_cos, const float* rope_sin, int B, int Hkv, int Nnew, int Ncap,
                           int d, int G, int rot_dim, int max_pos, int interleaved, int dtype, void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kcache, Vcache, seqlens_k, seqlens_out, nullptr, nullptr, nullptr, B, Hkv, Nnew,
                                             Ncap, d, dtype, 0, 0, 0, false, false, static_cast<hipStream_t>(stream), Q, Qout, rope_cos,
                                             rope_sin, G, rot_dim, max_pos, interleaved, true});
}

FA_EXPORT int fa_kvcache_append_paged_rope(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int* seqlens_k,
                                 int* seqlens_out, const int* block_table, const void* Q, void* Qout, const float* rope_cos,
                                 const float* rope_sin, int B, int Hkv, int Nnew, int num_pages, int page_size, int max_pages, int d,
                                 int G, int rot_dim, int max_pos, int interleaved, int dtype, void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kpool, Vpool, seqlens_k, seqlens_out, block_table, nullptr, nullptr, B, Hkv, Nnew,
                                             0, d, dtype, num_pages, page_size, max_pages, true, false, static_cast<hipStream_t>(stream),
                                             Q, Qout, rope_cos, rope_sin, G, rot_dim, max_pos, interleaved, true});
}

FA_EXPORT int fa_kvcache_append_fp8_rope(const void* Knew, const void* Vnew, void* Kcache, void* Vcache, const int* seqlens_k,
                               int* seqlens_out, const float* k_scale, const float* v_scale, const void* Q, void* Qout,
                               const float* rope_cos, const float* rope_sin, int B, int Hkv, int Nnew, int Ncap, int d, int G,
                               int rot_dim, int max_pos, int interleaved, int in_dtype, void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kcache, Vcache, seqlens_k, seqlens_out, nullptr, k_scale, v_scale, B, Hkv, Nnew,
                                             Ncap, d, in_dtype, 0, 0, 0, false, true, static_cast<hipStream_t>(stream), Q, Qout, rope_cos,
                                             rope_sin, G, rot_dim, max_pos, interleaved, true});
}

FA_EXPORT int fa_kvcache_append_paged_fp8_rope(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int* seqlens_k,
                                     int* seqlens_out, const int* block_table, const float* k_scale, const float* v_scale,
                                     const void* Q, void* Qout, const float* rope_cos, const float* rope_sin, int B, int Hkv, int Nnew,
                                     int num_pages, int page_size, int max_pages, int d, int G, int rot_dim, int max_pos,
                                     int interleaved, int in_dtype, void* stream)
{
    return (int)fa::kvcache_append_dispatch({Knew, Vnew, Kpool, Vpool, seqlens_k, seqlens_out, block_table, k_scale, v_scale, B, Hkv, Nnew,
                                             0, d, in_dtype, num_pages, page_size, max_pages, true, true, static_cast<hipStream_t>(stream),
                                             Q, Qout, rope_cos, rope_sin, G, rot_dim, max_pos, interleaved, true});
}

// The descriptor form of the eight append entries above, plus seqlens_new.  What the descriptor alone can get wrong is judged here;
// everything else by kvcache_append_dispatch, as for the flat entries.
FA_EXPORT int fa_kvcache_append_ex(const fa_kvappend_desc* desc)
{
    if (!desc || desc->size != sizeof(fa_kvappend_desc)) return (int)hipErrorInvalidValue;
    if (desc->kv_dtype != FA_KV_16BIT && desc->kv_dtype != FA_KV_FP8_E4M3) return (int)hipErrorInvalidValue;
    const bool fp8 = desc->kv_dtype == FA_KV_FP8_E4M3, paged = desc->block_table != nullptr, rope = desc->rope_cos != nullptr;
    if (!fp8 && (desc->k_scale || desc->v_scale)) return (int)hipErrorInvalidValue;   // a 16-bit cache has no scales
    if (!rope && (desc->Q || desc->Qout || desc->rope_sin)) return (int)hipErrorInvalidValue;   // arguments of the rotary forms
    return (int)fa::kvcache_append_dispatch({desc->Knew, desc->Vnew, desc->K, desc->V, desc->seqlens_k, desc->seqlens_out, desc->block_table,
                                             desc->k_scale, desc->v_scale, desc->B, desc->Hkv, desc->Nnew, paged ? 0 : desc->Ncap, desc->d,
                                             desc->dtype, paged ? desc->num_pages : 0, paged ? desc->page_size : 0,
                                             paged ? desc->max_pages : 0, paged, fp8, static_cast<hipStream_t>(desc->stream), desc->Q,
                                             desc->Qout, desc->rope_cos, desc->rope_sin, rope ? desc->G : 0, rope ? desc->rot_dim : 0,
                                             rope ? desc->max_pos : 0, rope ? desc->interleaved : 0, rope, desc->seqlens_new});
}

FA_EXPORT int fa_kvcache_append_varlen(const fa_kvappend_varlen_desc* desc) { return (int)fa::kvcache_append_varlen(desc); }
FA_EXPORT int fa_kvcache_append_varlen_ex(const fa_kvappend_varlen_desc* desc, const fa_kvappend_varlen_opts* opts)
{
    return (int)fa::kvcache_append_varlen_ex(desc, opts);
}

FA_EXPORT int fa_kvcache_commit(const fa_kvcommit_desc* desc) { return (int)fa::kvcache_commit(desc); }

FA_EXPORT size_t fa_mla_decode_workspace_bytes(const fa_mla_decode_desc* desc) { return fa::mla_decode_workspace_bytes(desc); }
FA_EXPORT int fa_mla_decode(const fa_mla_decode_desc* desc) { return (int)fa::mla_decode_dispatch(desc); }
FA_EXPORT int fa_mla_append(const fa_mla_append_desc* desc) { return (int)fa::mla_append_dispatch(desc); }
FA_EXPORT size_t fa_mla_decode_fp8_workspace_bytes(const fa_mla_decode_desc* desc) { return fa::mla_decode_workspace_bytes(desc); }
FA_EXPORT int fa_mla_decode_fp8(const fa_mla_decode_desc* desc, const float* c_scale)
{
    return (int)fa::mla_decode_fp8_dispatch(desc, c_scale);
}
FA_EXPORT int fa_mla_append_fp8(const fa_mla_append_desc* desc, const float* c_scale)
{
    return (int)fa::mla_append_fp8_dispatch(desc, c_scale);
}

FA_EXPORT int fa_merge_states(const fa_merge_desc* desc) { return (int)fa::merge_states_dispatch(desc); }

FA_EXPORT int fa_forward_varlen(const fa_varlen_desc* desc) { return (int)fa::varlen_dispatch(desc); }
FA_EXPORT int fa_forward_varlen_ex(const fa_varlen_desc* desc, const fa_varlen_opts* opts)
{
    return (int)fa::varlen_logits_dispatch(desc, opts);
}
FA_EXPORT int fa_forward_varlen_kvcache(const fa_varlen_kvcache_desc* desc) { return (int)fa::varlen_cache_dispatch(desc); }
FA_EXPORT int fa_forward_varlen_kvcache_fp8(const fa_varlen_kvcache_desc* desc, const float* k_scale, const float* v_scale)
{
    return (int)fa::varlen_cache_fp8_dispatch(desc, k_scale, v_scale);
}

FA_EXPORT size_t fa_kvcache_decode_varlen_workspace_bytes(const fa_kvdecode_varlen_desc* desc) { return fa::kvpacked_workspace_bytes(desc); }
FA_EXPORT int fa_kvcache_decode_varlen(const fa_kvdecode_varlen_desc* desc) { return (int)fa::kvpacked_dispatch(desc); }
FA_EXPORT int fa_kvcache_decode_varlen_ex(const fa_kvdecode_varlen_desc* desc, const fa_kvdecode_tree_opts* opts)
{
    return (int)fa::kvtree_dispatch(desc, opts);
}

FA_EXPORT int fa_kvcache_attend_varlen_part(const fa_kvdecode_varlen_desc* desc, int parts) { return (int)fa::kvattend_dispatch(desc, parts); }
FA_EXPORT int fa_kvcache_attend_varlen(const fa_kvdecode_varlen_desc* desc)
{
    return (int)fa::kvattend_dispatch(desc, FA_ATTEND_SHORT | FA_ATTEND_LONG);
}

FA_EXPORT int fa_debug_stage(int stage, const void* A, const void* B, void* Out, int BH, int N, int d, float scale,
                   int dtype, void* stream)
{
    return (int)fa::debug_stage_dispatch(stage, A, B, Out, BH, N, d, scale, dtype, static_cast<hipStream_t>(stream));
}

FA_EXPORT int flashattn_streaming_16x16_mw(const void* Q, const void* K, const void* V, float* O,
                                 int num_batches, int seq_len, float scale, void* stream)
{
    return (int)fa::streaming16_dispatch(Q, K, V, O, num_batches, seq_len, scale, false,
                                         static_cast<hipStream_t>(stream));
}

FA_EXPORT int flashattn_streaming_16x16_mw_kt(const void* Q, const void* K_T, const void* V, float* O,
                                    int num_batches, int seq_len, float scale, void* stream)
{
    return (int)fa::streaming16_dispatch(Q, K_T, V, O, num_batches, seq_len, scale, true,
                                         static_cast<hipStream_t>(stream));
}

FA_EXPORT int fa_selected_algo(int B, int H, int N, int d, int in_dtype)
{
    if (B <= 0 || H <= 0 || N <= 0 || d <= 0 || (long long)B * H > 0x7FFFFFFFll) return -1;
    return fa::auto_algo(B * H, N, d, in_dtype);
}

FA_EXPORT const char* fa_selected_kernel(int B, int H, int N, int d, int in_dtype, int algo)
{
    if (algo == FA_ALGO_AUTO) algo = fa_selected_algo(B, H, N, d, in_dtype);
    return algo < 0 ? "" : fa::algo_kernel_name(algo, d);
}

FA_EXPORT const char* fa_mi355_version(void) { return "fa_mi355 0.3.1 gfx950"; }

}  // extern "C"
