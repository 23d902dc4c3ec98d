// fa_dispatch.hpp -- the host side every translation unit shares: the argument structs (one per family: a forward, a KV-cache
// decode, an append), the element-type switch, and the one declaration of each host function that crosses a translation unit.
// Private to csrc/ (the public contract is include/fa_mi355.h); no device code and none of the kernels' argument packs live here
// (the decode launcher that needs both is fa_fwd_kvdecode.hpp).
#pragma once
#include "fa_common.hpp"

#include <stddef.h>
#include <type_traits>

struct fa_merge_desc;   // include/fa_mi355.h
struct fa_varlen_desc;
struct fa_varlen_opts;
struct fa_varlen_kvcache_desc;
struct fa_kvappend_varlen_desc;
struct fa_kvdecode_varlen_desc;
struct fa_kvdecode_tree_opts;
struct fa_kvappend_varlen_opts;
struct fa_kvcommit_desc;
struct fa_mla_decode_desc;
struct fa_mla_append_desc;

namespace fa {

// One self-attention forward: Q, K, V, O [BH, N, D] row-major, in_dtype FA_DTYPE_*, out_dtype FA_OUT_*.  The split-KV, debug-stage,
// streaming16 and lab entry points take other argument sets and keep their own lists.
struct FwdArgs {
    const void *Q, *K, *V;
    void* O;
    int BH, N, D;
    float scale;
    int in_dtype, out_dtype;
    hipStream_t stream;
};

// The in_dtype x out_dtype switch: f(F16{} | BF16{}, std::true_type | std::false_type) -- the element traits and "output is
// fp32" -- for the <T, kOutF32> instantiation the two ids name.  An out_dtype other than FA_OUT_F32 is the 16-bit output (the
// C entry points admit the two values only).
template <typename F>
static inline hipError_t with_types(int in_dtype, int out_dtype, F&& f)
{
    if (in_dtype == 0) return out_dtype == 0 ? f(F16{}, std::true_type{}) : f(F16{}, std::false_type{});
    if (in_dtype == 1) return out_dtype == 0 ? f(BF16{}, std::true_type{}) : f(BF16{}, std::false_type{});
    return hipErrorInvalidValue;
}

// scale * log2(e) as every kernel takes it.  The tiled, interleaved, pipeline and plain split-KV kernels mask a key by setting its
// score to -inf and form fma(score, |c|, -m): with c == 0 that is 0 * -inf, a NaN, wherever a mask applies (ragged N or Nk, the
// causal mask).  So a product of magnitude below FLT_MIN (scale 0, or a scale that underflows) goes to the device as +-FLT_MIN:
// every finite score then moves the exponent by a negligible amount (uniform weights, as scale 0 asks) and -inf stays -inf.
// A NaN scale passes through.  Host side only: the kernels are compiled as before.
static inline float host_scale_log2e(float scale)
{
    const float c = scale * kLog2e;
    if (!(__builtin_fabsf(c) < 1.17549435e-38f)) return c;
    return __builtin_copysignf(1.17549435e-38f, c);
}

// The kernel family a forward on the rolling pipeline runs on: what the algo table (fa_fwd_kernels.hip) asks rp16_dispatch() /
// rp16_causal_dispatch() (fa_fwd_rp16.hip) for.
enum class Rp16Family {
    kFull,       // 64-row waves at D = 64 (512-row workgroups), 32-row waves at D = 128 (256-row workgroups)
    kHalf,       // 32-row waves at D = 64, 16-row waves at D = 128
    kQuarter,    // 16-row waves (D = 64)
    kOneWave,    // one wave per SIMD: four 64-row waves per 256-row workgroup (D = 128)
    kKeySplit,   // 32-row waves, keys split over two groups of four waves per 128-row workgroup (D = 64, N % 128 == 0)
    kDma,        // kFull with K/V staging by LDS-DMA (D = 64, experimental build)
};

// ---- fa_fwd_kernels.hip: the algo table and the two dispatchers ----
hipError_t forward_dispatch(const FwdArgs& a, int algo);
hipError_t forward_causal_dispatch(const FwdArgs& a, int algo);
int auto_algo(int BH, int N, int D, int in_dtype);
const char* algo_kernel_name(int algo, int D);

// ---- fa_fwd_il.hip ---- waves: 8 = one 256-row workgroup per CU, 4 = two 128-row workgroups per CU
hipError_t il_dispatch(const FwdArgs& a, int waves);

// ---- fa_fwd_rp16.hip ---- fold: the folded fast pass first (else the exact passes only)
hipError_t rp16_dispatch(const FwdArgs& a, bool fold, Rp16Family family);
hipError_t rp16_causal_dispatch(const FwdArgs& a, Rp16Family family);   // kFull or kOneWave
// One (D, X, staging, mask, waves, key split) family of the pipeline, defined in fa_fwd_rp16_kernel.hpp and explicitly instantiated
// in fa_fwd_rp16_{d64,d64n,d64ks,d128,d128w,c,cw}.hip, one translation unit per group so that they compile side by side.
template <int D, int X, bool kDma, bool kCausal, int kWv = 8, int kKeySplit = 1>
hipError_t rp16_family(const FwdArgs& a, bool fold);

// ---- the split-KV stream and what else runs on it or beside it: fa_fwd_split.hip, fa_fwd_kv*.hip, fa_kvcache_*.hip, fa_debug_stages.hip, fa_streaming16.hip ----
hipError_t split_dispatch(const void* Q, const void* K, const void* V, void* O, void* ws, size_t ws_bytes,
                          int BH, int Nq, int Nk, int D, float scale, int in_dtype, int out_dtype, hipStream_t stream);
size_t split_workspace_bytes(int BH, int Nq, int Nk, int D);
int split_count(int BH, int Nq, int Nk);   // number of key splits for a shape: from the shape alone (a fixed workgroup target), no device query
// KV-cache decode (fa_forward_kvcache): Q, O [B, Hkv*G, Nq, D], K, V [B, Hkv, Ncap, D]; seqlens (device, B int32) and lse (device,
// [B, Hkv*G, Nq] fp32) may be null; ws as for split_dispatch, sized by kvcache_workspace_bytes().
struct KvCacheArgs {
    const void *Q, *K, *V;
    void* O;
    float* lse;
    const int* seqlens;
    int B, Hkv, G, Nq, Ncap, D;
    float scale;
    int causal, in_dtype, out_dtype;
    void* ws;
    size_t ws_bytes;
    hipStream_t stream;
};
// Paged KV-cache decode (fa_forward_kvcache_paged): the KvCacheArgs with K, V as page pools [num_pages, Hkv, page_size, D],
// Ncap = max_pages * page_size, and the device block table [B, max_pages] int32.
struct KvPagedArgs {
    KvCacheArgs c;
    const int* table;
    int num_pages, page_size, max_pages;
};
// Where the rows of a token-packed call live (fa_kvcache_decode_varlen): Q and O are packed (total_q, Hkv*G, d) tensors behind these
// strides (elements), lse is [Hkv*G, total_q], and the counts come from cu_q on the device.  tree_mask (fa_kvcache_decode_varlen_ex
// alone, else null): one 64-bit ancestor word per token row on the device.
struct KvPackedRows {
    const int* cu_q;
    int total_q;
    long long q_st, q_sh, o_st, o_sh;
    const unsigned long long* tree_mask;
};
// The features of the decode stream form a line, each level holding every one below it; kTree and kRouted both stand on kPacked.  A
// call runs the kernels of the lowest level that has what it asks for.
enum class KvLevel {
    kPlain,    // key counts, causal tail, lse
    kWindow,   // window >= 1
    kLogits,   // sinks or softcap; from here up window 0 runs as window = capacity
    kRagged,   // seqlens_q
    kPacked,   // packed rows (fa_kvcache_decode_varlen)
    kTree,     // packed rows under a tree mask (fa_kvcache_decode_varlen_ex)
    kRouted,   // packed rows, sequences above max_q left out (the SHORT half of fa_kvcache_attend_varlen)
};
// One decode call, every entry's: p.c alone for a contiguous cache, all of p with `paged` (the checks fill in Ncap).  fp8: K, V hold
// one-byte e4m3fn elements, and k_scale, v_scale are device pointers to Hkv fp32 each, or null (1.0).  window: 0 none, < 0 rejected.
// sinks: a device pointer to Hkv * G fp32 logits, or null; softcap: 0 off (negative, NaN or inf: rejected); seqlens_q: a device
// pointer to B int32 query counts, or null; packed: null but for the token-packed entries, where p.c.Nq is max_q and seqlens_q null.
// The fields from sinks on come last so that the flat entries' initialisers leave them zero.  level: set by the entry's checker.
struct KvDecodeArgs {
    KvPagedArgs p;
    const float *k_scale, *v_scale;
    int window;
    bool paged, fp8;
    const float* sinks;
    float softcap;
    const int* seqlens_q;
    const KvPackedRows* packed;
    KvLevel level;
};
// The kernels of one (level, fp8, paged) cell launched on checked arguments, with the merge behind a split; lg_page: log2 of the page
// size (paged only).  Defined in fa_fwd_kvdecode.hpp and explicitly instantiated in the fa_fwd_kv*.hip unit that owns the cell.
template <KvLevel kLevel, bool kFp8, bool kPaged> hipError_t kvdecode_unit(const KvDecodeArgs& a, int lg_page);
// fa_fwd_kvcache.hip: the flat and descriptor entries' checks (levels kPlain to kRagged); the router every checker hands its checked
// arguments to; the merge behind a split, for all of them
hipError_t kvdecode_dispatch(const KvDecodeArgs& a);
hipError_t kvdecode_route(const KvDecodeArgs& a, int lg_page);
hipError_t kvdecode_combine(const KvDecodeArgs& a, int S);
// fa_fwd_kvpacked.hip: fa_kvcache_decode_varlen (tree_mask null) and, through kvtree_dispatch (fa_fwd_kvtree.hip, the options' checks),
// fa_kvcache_decode_varlen_ex.  kvpacked_check is the checks alone: on success `d` holds the checked arguments (the capacity filled
// in, the level set, d.packed pointing at `rows_of`, which the caller keeps alive) and lg_page the paged check's
hipError_t kvpacked_dispatch(const ::fa_kvdecode_varlen_desc* desc, const unsigned long long* tree_mask = nullptr);
size_t kvpacked_workspace_bytes(const ::fa_kvdecode_varlen_desc* desc);
hipError_t kvtree_dispatch(const ::fa_kvdecode_varlen_desc* desc, const ::fa_kvdecode_tree_opts* opts);
hipError_t kvpacked_check(const ::fa_kvdecode_varlen_desc* desc, const unsigned long long* tree_mask, KvPackedRows& rows_of, KvDecodeArgs& d,
                          int& lg_page);
// fa_kvcache_attend_varlen[_part] (fa_fwd_kvrouted.hip): kvpacked_check and varlen_cache_check on the one descriptor, then the parts
// that were asked for -- FA_ATTEND_SHORT: level kRouted; FA_ATTEND_LONG: the routed varlen cache kernels of
// fa_fwd_varlen_cache_routed.hip or _routed_fp8.hip
hipError_t kvattend_dispatch(const ::fa_kvdecode_varlen_desc* desc, int parts);
// args: the checked VarlenCacheArgs (16-bit) or VarlenCacheFp8Args; min_rows: sequences of at most as many rows are skipped
hipError_t varlen_cache_routed_launch16(const ::fa_varlen_kvcache_desc* desc, const void* args, unsigned grid, int min_rows);
hipError_t varlen_cache_routed_launch8(const ::fa_varlen_kvcache_desc* desc, const void* args, unsigned grid, int min_rows);
// The argument checks alone: the append runs them too, so it accepts exactly the caches the decode accepts.  kvpaged_check fills
// in the capacity and returns page_log2(page_size): log2 of a page size the kernels take, else -1.
hipError_t kvcache_check(const KvCacheArgs& a);
hipError_t kvpaged_check(const KvPagedArgs& p, KvPagedArgs& with_capacity, int& lg_page);
int page_log2(int page_size);
int window_span_cap(int Nq, int Ncap, int window);   // the longest key range a sequence can stream, in keys (window >= 1)
size_t kvcache_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D);
size_t kvpaged_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int D);
size_t kvwindow_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D, int window);
size_t kvpaged_window_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int D, int window);
// KV-cache append (fa_kvcache_append and its paged / fp8 forms) -- fa_kvcache_append.hip: Knew, Vnew [B, Hkv, Nnew, D] of `dtype` go
// behind each sequence's length into K, V (a cache [B, Hkv, Ncap, D], or with `paged` a pool [num_pages, Hkv, page_size, D] through
// `table`; with `fp8` one e4m3fn byte per element, quantised by k_scale / v_scale).  seqlens (null: all empty), seqlens_out (null:
// not written), table and the scales are device pointers.
struct KvAppendArgs {
    const void *Knew, *Vnew;
    void *K, *V;
    const int* seqlens;
    int* seqlens_out;
    const int* table;
    const float *k_scale, *v_scale;
    int B, Hkv, Nnew, Ncap, D, dtype;
    int num_pages, page_size, max_pages;
    bool paged, fp8;
    hipStream_t stream;
    // the _rope entries (fa_kvcache_append_padded.hip), at the end so that the plain entries' initialisers leave them zero: K is rotated
    // at its position on the way into the cache, and Q [B, Hkv*G, Nnew, D] of `dtype` into Qout (the same buffer, a disjoint one, or
    // both null: K only).  rope_cos, rope_sin: device fp32 [max_pos, rot_dim / 2].
    const void* Q;
    void* Qout;
    const float *rope_cos, *rope_sin;
    int G, rot_dim, max_pos, interleaved;
    bool rope;
    // fa_kvcache_append_ex alone (fa_kvcache_append_padded.hip): a device pointer to B int32 token counts, m_b = min(max(., 0), Nnew);
    // null: every sequence appends Nnew tokens, and the call is the flat entry's
    const int* seqlens_new;
};
hipError_t kvcache_append_dispatch(const KvAppendArgs& a);
// what kvcache_append_dispatch hands a checked call with `rope` or seqlens_new to (fa_kvcache_append_padded.hip); Ncap: the checked
// capacity, lg_page: log2 of the page size (paged only)
hipError_t kvcache_append_padded(const KvAppendArgs& a, int Ncap, int lg_page);
// What the write side shares on the host (fa_kvcache_append.hip).  The cache of an append, append_varlen or commit call with the rows
// that go into it (commit: the caches themselves): kvwrite_check runs the decode entries' checks on it (kvcache_check, kvpaged_check),
// the rows standing in for Q and O, and returns the checked capacity and log2 of the page size (0: contiguous).
struct KvWriteCache {
    const void *src_k, *src_v, *K, *V;
    const int *seqlens, *table;
    int B, Hkv, Ncap, D, dtype, num_pages, page_size, max_pages;
    bool paged;
};
hipError_t kvwrite_check(const KvWriteCache& w, int& Ncap, int& lg_page);
// the rotary arguments' checks, short of what Q and Qout add; heads: B * Hkv
hipError_t kvappend_rope_check(const float* cos, const float* sin, int rot_dim, int D, int max_pos, int G, int interleaved, long long heads);
// The lengths kernel behind every append's copy, out[i] = min(clamp(in[i], 0, cap) + m_i, cap): m_i is the clamped cu[i + 1] - cu[i]
// with a cu (n: the total), else cnt[i] clamped into [0, n], else n.  Nothing is launched without an `out`.
hipError_t kvappend_lens(const int* in, const int* cnt, const int* cu, int* out, int B, int n, int cap, hipStream_t stream);
// fa_kvcache_append_varlen (fa_kvcache_append_varlen.hip): the checks and the one or two launches; the descriptor is the public one, as it is
hipError_t kvcache_append_varlen(const ::fa_kvappend_varlen_desc* desc);
// fa_kvcache_append_varlen_ex: the options' checks, then the same; positions (device, total_new int32, or null) are the rotary table
// rows of the tokens in place of their slots
hipError_t kvcache_append_varlen_ex(const ::fa_kvappend_varlen_desc* desc, const ::fa_kvappend_varlen_opts* opts);
// fa_kvcache_commit (fa_kvcache_commit.hip): the checks and the one or two launches; the descriptor is the public one, as it is
hipError_t kvcache_commit(const ::fa_kvcommit_desc* desc);
// fa_mla_decode (fa_mla_decode.hip) and fa_mla_append (fa_mla_append.hip): the checks and the launches on the public descriptors;
// mla_geometry is the capacity and page check the two share (cap: Ncap or max_pages * page_size; lg_page: 0 when contiguous)
hipError_t mla_decode_dispatch(const ::fa_mla_decode_desc* desc);
size_t mla_decode_workspace_bytes(const ::fa_mla_decode_desc* desc);
hipError_t mla_append_dispatch(const ::fa_mla_append_desc* desc);
// fa_mla_decode_fp8 and fa_mla_append_fp8: the same checks on the same descriptors, C then addresses rows of 576 e4m3fn codes;
// c_scale is the cache's one fp32 scale on the device (4-byte aligned), or null (1.0).  The fp8 decode kernels live in
// fa_mla_decode_fp8.hip, the fp8 append kernels beside the copy in fa_mla_append.hip.
hipError_t mla_decode_fp8_dispatch(const ::fa_mla_decode_desc* desc, const float* c_scale);
hipError_t mla_append_fp8_dispatch(const ::fa_mla_append_desc* desc, const float* c_scale);
bool mla_geometry(const int* block_table, int Ncap, int num_pages, int page_size, int max_pages, int& cap, int& lg_page);
// fa_merge_states (fa_merge_states.hip): the checks and the one launch; the descriptor is the public one, as it is
hipError_t merge_states_dispatch(const ::fa_merge_desc* desc);
// fa_forward_varlen (fa_fwd_varlen.hip): the checks and the one launch; the descriptor is the public one, as it is
hipError_t varlen_dispatch(const ::fa_varlen_desc* desc);
// fa_forward_varlen_ex (fa_fwd_varlen_logits.hip): the options' checks, then varlen_dispatch (no options, or all off) or the one launch
hipError_t varlen_logits_dispatch(const ::fa_varlen_desc* desc, const ::fa_varlen_opts* opts);
// fa_forward_varlen_kvcache (fa_fwd_varlen_cache.hip): the checks and the one launch; the descriptor is the public one, as it is
hipError_t varlen_cache_dispatch(const ::fa_varlen_kvcache_desc* desc);
// ... what it hands a checked call with an option on to (fa_fwd_varlen_cache_logits.hip); args: the checked VarlenCacheArgs
hipError_t varlen_cache_logits_launch(const ::fa_varlen_kvcache_desc* desc, const void* args, unsigned grid);
// fa_forward_varlen_kvcache_fp8 (fa_fwd_varlen_cache_fp8.hip): the 16-bit entry's checks and the one launch on an e4m3fn cache;
// k_scale, v_scale: device pointers to Hkv fp32 each, or null (1.0)
hipError_t varlen_cache_fp8_dispatch(const ::fa_varlen_kvcache_desc* desc, const float* k_scale, const float* v_scale);
// ... what it hands a checked call with an option on to (fa_fwd_varlen_cache_fp8_logits.hip); args: the checked VarlenCacheFp8Args
hipError_t varlen_cache_fp8_logits_launch(const ::fa_varlen_kvcache_desc* desc, const void* args, unsigned grid);
hipError_t debug_stage_dispatch(int stage, const void* A, const void* B, void* Out, int BH, int N, int D, float scale,
                                int dtype, hipStream_t stream);
hipError_t streaming16_dispatch(const void* Q, const void* K, const void* V, float* O,
                                int num_batches, int seq_len, float scale, bool k_transposed,
                                hipStream_t stream);

#ifdef FA_EXPERIMENTS
// ---- the A/B kernel of the experimental build: fa_fwd_rp.hip ----
hipError_t rp_dispatch(const FwdArgs& a, int fold);      // fold: 1 = folded fast pass where it exists (fp16, d = 64)
// ---- ... and its measurement entry points ----
hipError_t il_diag_dispatch(const void* Q, const void* K, const void* V, void* O,
                            int BH, int N, float scale, unsigned long long* diag, int waves, hipStream_t stream);
// the per-block pass-id recorder is a device variable of each pipeline translation unit: one setter per unit, and all of them
hipError_t rp16_set_pass_ids(unsigned* dev_ptr);
hipError_t rp16_set_pass_ids_d64(unsigned*);
hipError_t rp16_set_pass_ids_d64n(unsigned*);
hipError_t rp16_set_pass_ids_d64ks(unsigned*);
hipError_t rp16_set_pass_ids_d128(unsigned*);
hipError_t rp16_set_pass_ids_d128w(unsigned*);
hipError_t rp16_set_pass_ids_c(unsigned*);
hipError_t rp16_set_pass_ids_cw(unsigned*);
#endif

}  // namespace fa
