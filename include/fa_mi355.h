/*
 * fa_mi355.h -- C ABI of libfa_mi355.so: FlashAttention forward for AMD Instinct MI355X (gfx950).
 *
 * The reference (jeehun98/FlashAttention_Kernel_Project) has no library and nothing `extern "C"`:
 * every kernel is a C++ `__global__` launched with <<<grid,block[,smem]>>> from its own main().
 * What the reference fixes is each kernel's ARGUMENT LIST, tensor layouts, dtypes and grid
 * convention.  Each entry point below keeps one of those argument lists in the same order and
 * adds a trailing stream handle (the reference always uses the null stream: pass NULL).
 *
 * All pointers are DEVICE pointers owned by the caller; nothing is allocated or freed here; O is
 * fully overwritten (no need to pre-zero).  Launches are asynchronous with respect to the host.
 * Return value: a hipError_t as int (0 = hipSuccess).  Unsupported shapes return
 * hipErrorInvalidValue (1) -- the reference kernels silently `return` instead
 * (flashattn_forward_wmma.cu:59-63); the library never calls exit().
 *
 * `stream` is a hipStream_t passed as void*.
 */
#ifndef FA_MI355_H
#define FA_MI355_H

#include <stddef.h>   /* size_t (split-KV workspace) */

#ifdef __cplusplus
extern "C" {
#endif

#define FA_DTYPE_F16  0
#define FA_DTYPE_BF16 1
#define FA_OUT_F32    0   /* the reference's output type */
#define FA_OUT_SAME   1   /* output in the input's 16-bit type */

/* Kernel selection for fa_forward_ex().  Ids present in the product library: */
#define FA_ALGO_AUTO            0 /* d=64, N > 256 and d=128: RP16_FOLD on the widest waves whose grid still covers the device
                                     (24, else _HALF 26, else _QUARTER 27 / _KS2 29, by rounds x rows / efficiency); d=64, N <= 256:
                                     INTERLEAVED / _2WG; else GENERIC -- fa_selected_algo() */
#define FA_ALGO_GENERIC         1 /* single 16x16 MFMA fragment per wave, any D % 16 == 0, D <= 256 */
#define FA_ALGO_TILED           2 /* LDS-staged 256-row workgroups, QK^T -> softmax -> PV per tile, D in {64,128} */
#define FA_ALGO_INTERLEAVED     5 /* QK^T one tile ahead, PV one tile behind, one MFMA per slice of softmax VALU, D = 64 */
#define FA_ALGO_INTERLEAVED_2WG 6 /* the same with 128-row workgroups, two per CU, D = 64 */
#define FA_ALGO_RP16           23 /* rolling half-tile pipeline on v_mfma_f32_16x16x32 (four 16-row blocks per wave at D = 64, two at D = 128),
                                     branch-free steady state, single-instruction fp32 vector work, exact passes */
#define FA_ALGO_RP16_FOLD      24 /* RP16 with the folded fast pass: scale folded into a rounded Q, the wave's reference max as the
                                     accumulators' start value (bf16: K converted to fp16 while it is staged), row sums on the matrix
                                     pipe; per-workgroup fallback chain: exact optimistic pass, then the tracked pass */
#define FA_ALGO_RP16_FOLD_HALF 26 /* RP16_FOLD on half-width waves (256-row workgroups at D = 64, 128-row at D = 128): grids too
                                     small to cover the device with the full-width ones */
#define FA_ALGO_RP16_FOLD_QUARTER 27 /* ... on quarter-width waves (128-row workgroups), D = 64 */
#define FA_ALGO_RP16_FOLD_KS2  29 /* RP16_FOLD, D = 64, 128-row workgroups: two groups of four 32-row waves, each on half the keys, merged through LDS
                                     (N % 128 == 0; other N run _QUARTER); AUTO for few heads and N >= 2048 */
#define FA_ALGO_RP16_FOLD_1W   28 /* RP16_FOLD at D = 128 with ONE wave per SIMD: four 64-row waves per 256-row workgroup, 512 registers each,
                                     every LDS fragment feeding four matrix instructions; AUTO at D = 128 from N = 4096; also accepted by fa_forward_causal (D = 128; AUTO there from N = 8192 on grids of >= 4 rounds) */
/* Only in the experimental build (`make experimental`, fa_mi355_has_experiments() == 1; hipErrorInvalidValue otherwise):
 * A/B kernels that AUTO never selects. */
#define FA_ALGO_RP             21 /* the rolling pipeline on 32x32x16 (two 32-row blocks per wave), exact passes */
#define FA_ALGO_RP_FOLD        22 /* RP with the folded fast pass (fp16, D = 64) */
#define FA_ALGO_RP16_DMA       25 /* RP16_FOLD with K/V staged by LDS-DMA (buffer_load ... lds) instead of through registers */
/* 3, 4 and 7-20 (round 1 / 2 A/B kernels two generations stale) were retired: hipErrorInvalidValue in both builds. */

/* General-shape forward.  Replaces
 *   flashattn_forward_wmma_kernel(const half* Q, const half* K, const half* V, float* O,
 *                                 int BH, int N, int D, float scale)
 *   FlashAttention/flashattn_forward_wmma/flashattn_forward_wmma.cu:49-58 (and _v2.cu:53, _v3.cu:52,
 *   _v4.cu:52, flashattn_forward_memory_bound/flashattn_forward_wmma_v5_cp_async.cu:99,
 *   flashattn_forward_wmma_memprofile.cu:60), launched as <<<(ceil(N/BLOCK_M), BH), block, smem>>>
 *   (flashattn_forward_wmma.cu:389-413).
 * Q,K,V [BH,N,D] row-major fp16, O [BH,N,D] fp32, self-attention, no mask.
 * D % 16 == 0 (as the reference requires, :63), D <= 256; any N >= 1 (tail rows/keys handled). */
int flashattn_forward_wmma(const void* Q, const void* K, const void* V, float* O,
                           int BH, int N, int D, float scale, void* stream);

/* The same operation with the dtype / output / kernel choices BASELINE's configs need
 * (bf16 inputs, 16-bit outputs, B and H separate).  BH = B*H.  Same layouts as above.
 * scale, here and in every entry point below: the logits are scale * q.k.  Any finite value is valid; a negative one negates
 * the logits.  scale = 0 -- any scale with |scale * log2(e)| < FLT_MIN -- gives every key a row sees the same weight: O is the
 * mean of their V rows (lse = ln of their number), never NaN, under every mask and at ragged sizes.  (The library hands the
 * kernels +-FLT_MIN in its place, so that a masked score of -inf is never multiplied by 0.) */
int fa_forward(const void* Q, const void* K, const void* V, void* O,
               int B, int H, int N, int d, float scale,
               int in_dtype, int out_dtype, void* stream);
int fa_forward_ex(const void* Q, const void* K, const void* V, void* O,
                  int B, int H, int N, int d, float scale,
                  int in_dtype, int out_dtype, int algo, void* stream);

/* Causal (lower-triangular) self-attention: query row i attends to keys 0..i.  Same layouts and
 * dtypes as fa_forward.  NOT a reference entry point: the reference has no mask; this is the first
 * "next" row of SURVEY.md 8(f) (cf. the runtime-M tail masking of
 * flashattn_warp_spc/flashattn_streaming_16x16_mw_v12d.cu:100-135).  algo: FA_ALGO_AUTO,
 * FA_ALGO_GENERIC, FA_ALGO_TILED (256-row workgroups), 6 (the tiled kernel with 128-row workgroups, two
 * per CU), FA_ALGO_RP16_FOLD (the pipeline under the mask; AUTO's choice whenever the grid gives every CU a
 * workgroup) or FA_ALGO_RP16_FOLD_1W (the same with one wave per SIMD, D = 128 only; AUTO's choice there from N = 8192 on
 * grids of >= 4 rounds); all but the first two need D in {64,128}. */
int fa_forward_causal(const void* Q, const void* K, const void* V, void* O,
                      int B, int H, int N, int d, float scale,
                      int in_dtype, int out_dtype, int algo, void* stream);

/* Nq != Nk with a split over the keys ("flash-decoding"): Q [B*H,Nq,d], K,V [B*H,Nk,d], O [B*H,Nq,d],
 * no mask, d in {64,128}.  Meant for few query rows against a long K/V, where one workgroup per
 * (head, query block) cannot fill the chip: the keys are cut into S chunks (S chosen by the library
 * from B*H, Nq, Nk), each chunk leaves an unnormalised partial result in `workspace`, and a second
 * small kernel merges them.  The caller owns the workspace (size from
 * fa_forward_splitkv_workspace_bytes(); 0 means S = 1 and `workspace` may be NULL).
 * Grouped-query attention needs no separate entry: with Q [B,Hq,Nq,d] and K,V [B,Hkv,Nk,d], the
 * G = Hq/Hkv query heads of a group are contiguous, so pass H = Hkv and Nq = G*Nq -- the group's K/V is
 * then streamed once for all G heads.
 * NOT a reference entry point (cf. the single-query experiment
 * flashattn_warp_spc_2/flashattn_streaming_16x16_mw_v7_5*.cu). */
size_t fa_forward_splitkv_workspace_bytes(int B, int H, int Nq, int Nk, int d);
int fa_forward_splitkv(const void* Q, const void* K, const void* V, void* O,
                       int B, int H, int Nq, int Nk, int d, float scale,
                       int in_dtype, int out_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Decode against a pre-allocated KV cache: fa_forward_splitkv with a key count PER SEQUENCE that is read on
 * the device, an optional causal mask aligned to the end of the cache, and an optional log-sum-exp output.
 *   Q, O            [B, Hkv*G, Nq, d]; query head hkv*G + g uses K/V head hkv (G = 1: plain multi-head)
 *   Kcache, Vcache  [B, Hkv, Ncap, d] contiguous, fp16 or bf16; d in {64,128}
 *   seqlens_k       device, B int32, or NULL (every sequence holds Ncap keys).  L_b = min(max(seqlens_k[b], 0), Ncap):
 *                   a bad length is clamped and never becomes an out-of-range read.  Rows at and past L_b are not read.
 *   causal = 0      row i of batch b attends to the keys [0, L_b)
 *   causal = 1      row i attends to [0, c_i), c_i = max(0, L_b - Nq + 1 + i): the LAST query row sees the whole
 *                   cache (i counts within the row's own head)
 *   lse             device, [B, Hkv*G, Nq] fp32, or NULL: ln sum_j exp(scale * q.k_j) over the keys the row sees
 * A row that sees no key (L_b = 0 or c_i = 0) gets O = 0 and lse = -inf, never NaN.  With lse, results over
 * disjoint key ranges (another chunk, another device) merge exactly: O = sum_r O_r exp(lse_r - lse), lse = ln sum_r exp(lse_r).
 * Nothing on the host reads seqlens_k: grid, split count and workspace size depend on (B, Hkv, G, Nq, Ncap, d) only,
 * so a call captured into a HIP graph replays correctly after the lengths were changed in place.  The keys of a
 * sequence are divided among its splits by L_b, not by Ncap: a cache filled to a fraction still uses every split.
 * Workspace as for fa_forward_splitkv (size from fa_forward_kvcache_workspace_bytes(); 0: `workspace` may be NULL).
 * Sliding windows are not part of this entry (they are fa_forward_kvcache_window's, below); a paged (block-table) cache goes through fa_forward_kvcache_paged below, an fp8 cache
 * through fa_forward_kvcache_fp8; fa_kvcache_append and its forms write the new token's K/V into any of them.
 * NOT a reference entry point. */
size_t fa_forward_kvcache_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int d);
int fa_forward_kvcache(const void* Q, const void* Kcache, const void* Vcache, void* O,
                       float* lse,            /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                       const int* seqlens_k,  /* device, B int32, may be NULL (= Ncap for all) */
                       int B, int Hkv, int G, int Nq, int Ncap, int d, float scale, int causal,
                       int in_dtype, int out_dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/* fa_forward_kvcache against a PAGED cache: a pool of fixed-size pages and, per sequence, a table of page numbers that is read
 * on the device.
 *   Kpool, Vpool    [num_pages, Hkv, page_size, d] contiguous, fp16 or bf16; d in {64,128}: one head of one page is a contiguous
 *                   block of page_size rows.  The token-major page layout [num_pages, page_size, Hkv, d] is NOT supported.
 *   block_table     device, [B, max_pages] int32 contiguous: key j of sequence b is row j % page_size of page
 *                   block_table[b][j / page_size]
 *   page_size       a power of two, at least 16 (16, 32, 64, 128, 256, ...); the capacity is Ncap = max_pages * page_size
 *   seqlens_k       as in fa_forward_kvcache: clamped to [0, Ncap]; NULL means every sequence holds Ncap keys
 * Q, O, lse, G, causal, rows without a key (O = 0, lse = -inf, never NaN) and the workspace contract are those of
 * fa_forward_kvcache, and so are the splits, the tile order and the arithmetic: on the same keys the two entries return the
 * same bits.
 * Nothing on the host reads seqlens_k or block_table.  Grid, split count and workspace depend on (B, Hkv, G, Nq, Ncap, d) only and
 * are what fa_forward_kvcache computes for that Ncap: fa_forward_kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size,
 * d) == fa_forward_kvcache_workspace_bytes(B, Hkv, G, Nq, max_pages * page_size, d).  A captured call follows a table and lengths
 * that are later rewritten in place.
 * What is read: table entries at or past ceil(L_b / page_size) are never read; rows of the last live page at or past L_b are
 * never used and may hold anything; a live table entry outside [0, num_pages) is never dereferenced -- such a page reads as
 * page_size rows of zeros (clamp, never fault, as for seqlens_k).  Page addresses are 64 bit: a pool may exceed 4 GiB.
 * hipErrorInvalidValue, before the device is touched: a null Q, Kpool, Vpool, O or block_table; a page_size that is not a power of
 * two or is below 16; num_pages <= 0 or max_pages <= 0; max_pages * page_size beyond int or beyond the 32-bit byte offsets
 * fa_forward_kvcache allows for its Ncap; everything else fa_forward_kvcache rejects.
 * Sliding windows are not part of this entry (they are fa_forward_kvcache_paged_window's, below); fp8 pools go through fa_forward_kvcache_paged_fp8 below, the new token's K/V is written
 * by fa_kvcache_append_paged.  NOT a reference entry point. */
size_t fa_forward_kvcache_paged_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int d);
int fa_forward_kvcache_paged(const void* Q, const void* Kpool, const void* Vpool, void* O,
                             float* lse,              /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                             const int* seqlens_k,    /* device, B int32, may be NULL (= Ncap for all) */
                             const int* block_table,  /* device, [B,max_pages] int32 */
                             int B, int Hkv, int G, int Nq,
                             int num_pages, int page_size, int max_pages, int d,
                             float scale, int causal, int in_dtype, int out_dtype,
                             void* workspace, size_t workspace_bytes, void* stream);

/* fa_forward_kvcache and fa_forward_kvcache_paged against an fp8 cache with one dequantisation scale per K/V head.
 *   Kcache, Vcache  [B, Hkv, Ncap, d], resp. Kpool, Vpool [num_pages, Hkv, page_size, d]: ONE byte per element, OCP e4m3fn (the gfx950
 *                   format: bias 7, 3 mantissa bits, no infinities, 0x7F / 0xFF NaN) -- not MI300X's e4m3fnuz, not e5m2.
 *   Q, O            as in the 16-bit entries; in_dtype is Q's type, and the type K and V are widened to on the way into the kernel.
 *                   Every e4m3fn value is exactly representable in fp16 and in bf16, so widening adds no error.
 *   k_scale, v_scale  device, Hkv fp32 each, or NULL (1.0 for every head).  The logits are scale * k_scale[hkv] * q.k8, the output is
 *                   v_scale[hkv] * softmax.v8, and lse is that of the scaled logits.  A scale must be finite and > 0.  Scales only
 *                   enter arithmetic: a bad one gives a meaningless result, never an out-of-range access.
 * Codes 0x7F and 0xFF behave as a NaN in a 16-bit cache does; rows at or past L_b and pages that are not live are never read and may
 * hold them.
 * Everything else is the 16-bit entries' contract: d in {64,128}; the length clamp; rows without a key (O = 0, lse = -inf); causal;
 * page_size a power of two >= 16, bad live table entries read as zeros, 64-bit page addresses; the same hipErrorInvalidValue cases
 * before the device is touched (the bound on Ncap is the 16-bit entries', although a row is half as long).  The workspace is exactly
 * what the 16-bit entry takes for the same shape: size it with fa_forward_kvcache_workspace_bytes() /
 * fa_forward_kvcache_paged_workspace_bytes().
 * Nothing on the host reads seqlens_k, block_table, k_scale or v_scale: a captured call follows all of them when they are rewritten in
 * place.  scale = 0 keeps its meaning (uniform weights, never NaN) for every k_scale: |scale * log2(e) * k_scale| is clamped to FLT_MIN
 * on the device, after the product.
 * Splits, tile order and arithmetic are the 16-bit entries': with all scales 1, O and lse equal fa_forward_kvcache[_paged] on the
 * widened cache bit for bit; a power-of-two k_scale equals that entry called with scale * k_scale, a power-of-two v_scale multiplies
 * its fp32 result exactly.
 * fp8 Q, e5m2 and per-token or per-block scales are not part of these entries; fa_kvcache_append_fp8 / _paged_fp8 write such a cache;
 * sliding windows are fa_forward_kvcache_fp8_window's and fa_forward_kvcache_paged_fp8_window's, below.
 * NOT reference entry points. */
int fa_forward_kvcache_fp8(const void* Q, const void* Kcache, const void* Vcache, void* O,
                           float* lse,            /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                           const int* seqlens_k,  /* device, B int32, may be NULL (= Ncap for all) */
                           const float* k_scale,  /* device, Hkv fp32, may be NULL (= 1.0) */
                           const float* v_scale,  /* device, Hkv fp32, may be NULL (= 1.0) */
                           int B, int Hkv, int G, int Nq, int Ncap, int d, float scale, int causal,
                           int in_dtype, int out_dtype,
                           void* workspace, size_t workspace_bytes, void* stream);
int fa_forward_kvcache_paged_fp8(const void* Q, const void* Kpool, const void* Vpool, void* O,
                                 float* lse,              /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                                 const int* seqlens_k,    /* device, B int32, may be NULL (= Ncap for all) */
                                 const int* block_table,  /* device, [B,max_pages] int32 */
                                 const float* k_scale,    /* device, Hkv fp32, may be NULL (= 1.0) */
                                 const float* v_scale,    /* device, Hkv fp32, may be NULL (= 1.0) */
                                 int B, int Hkv, int G, int Nq,
                                 int num_pages, int page_size, int max_pages, int d,
                                 float scale, int causal, int in_dtype, int out_dtype,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Sliding-window attention on the four KV-cache decode entries above.  Each _window entry takes the argument list of its base entry
 * with ONE more host integer, `window` = W, directly after `causal`.  Write L_b for the clamped length, Nq for the rows per query head
 * and c_i for row i's upper limit as the base entry defines it (L_b without causal, max(0, L_b - Nq + 1 + i) with it).
 *   W >= 1   row i attends to the keys [lo_i, c_i), lo_i = max(0, L_b - Nq + 1 + i - W).  The lower limit is the same with and without
 *            causal.  With causal a row sees its own position and the W - 1 before it (flash-attn's window_size = (W - 1, 0)); without
 *            causal it sees those and every later key (window_size = (W - 1, -1)).  With Nq = 1 the row sees the last W keys.
 *   W == 0   no window: the entry calls its base entry and returns its bits.
 *   W < 0    hipErrorInvalidValue, before the device is touched -- as is everything the base entry rejects.
 * A row with c_i = 0 still gets O = 0 and lse = -inf, never NaN; lo_i < c_i whenever c_i >= 1.  lse is taken over the keys the row
 * sees, so the merge rule over disjoint key ranges (fa_forward_kvcache) still holds.
 * What is read.  start_b = max(0, L_b - Nq + 1 - W) is row 0's lower limit: no row of the sequence sees a key below it.  Cache and
 * page rows below start_b are never used and may hold anything, NaN bit patterns included (they reach the arithmetic as zeros, not
 * as masked scores: a weight of 0 times a NaN would be a NaN).  On the paged entries a page that lies wholly below start_b is never
 * dereferenced and its block_table entry is never read, so it may hold garbage: the pages behind the window can be freed and reused.
 * Unchanged from the base entries: the clamp of seqlens_k, rows at and past L_b, bad live table entries reading as zeros, 64-bit page
 * addresses, the meaning of scale = 0, the fp8 scales, the folding of the G query heads of a group, and "nothing on the host reads
 * seqlens_k, block_table, k_scale or v_scale".  `window` is a host argument and is baked into a captured call; the lengths are still
 * followed on the device.
 * Splits and workspace.  The split count follows from the longest range one sequence can stream, not from the capacity:
 *   span_cap = min(Ncap, roundup64(W + Nq - 1) + 64)      (Ncap when W + Nq - 1 >= Ncap)
 * takes the place of Ncap in the base entry's rule, so grid and workspace still depend on host integers only:
 * fa_forward_kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W) resp. fa_forward_kvcache_paged_window_workspace_bytes(B, Hkv,
 * G, Nq, max_pages, page_size, d, W) size the workspace of the 16-bit and of the fp8 entries (0: `workspace` may be NULL; also 0 for
 * W < 0).  With W = 0 and with W + Nq - 1 >= Ncap they return the base function's value; otherwise the value may be SMALLER OR
 * LARGER than the base function's (the split count is not monotone in the key count): size a windowed call with these functions.
 * Per sequence the tiles from start_b rounded down to a multiple of 64 up to L_b are dealt out to the splits; nothing below that tile
 * is touched.  With W >= Ncap the result equals the base entry's bit for bit; with Nq = 1 and (L_b - W) % 64 == 0 it equals
 * fa_forward_kvcache on a cache of capacity W + 64 that holds the last W keys.  The paged entries return the bits of the contiguous
 * ones on the same keys, the fp8 entries with all scales 1 those of the 16-bit ones on the widened cache.
 * Not part of these entries: a ring-buffer (rolling) cache layout, a window on the prefill entries (fa_forward*), a window per
 * sequence or per head.  Attention sinks and soft-capping of the logits are fa_kvcache_decode's, below.  NOT reference entry points. */
size_t fa_forward_kvcache_window_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int d, int window);
size_t fa_forward_kvcache_paged_window_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int d, int window);
int fa_forward_kvcache_window(const void* Q, const void* Kcache, const void* Vcache, void* O,
                              float* lse,            /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                              const int* seqlens_k,  /* device, B int32, may be NULL (= Ncap for all) */
                              int B, int Hkv, int G, int Nq, int Ncap, int d, float scale, int causal, int window,
                              int in_dtype, int out_dtype,
                              void* workspace, size_t workspace_bytes, void* stream);
int fa_forward_kvcache_paged_window(const void* Q, const void* Kpool, const void* Vpool, void* O,
                                    float* lse,              /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                                    const int* seqlens_k,    /* device, B int32, may be NULL (= Ncap for all) */
                                    const int* block_table,  /* device, [B,max_pages] int32 */
                                    int B, int Hkv, int G, int Nq,
                                    int num_pages, int page_size, int max_pages, int d,
                                    float scale, int causal, int window, int in_dtype, int out_dtype,
                                    void* workspace, size_t workspace_bytes, void* stream);
int fa_forward_kvcache_fp8_window(const void* Q, const void* Kcache, const void* Vcache, void* O,
                                  float* lse,            /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                                  const int* seqlens_k,  /* device, B int32, may be NULL (= Ncap for all) */
                                  const float* k_scale,  /* device, Hkv fp32, may be NULL (= 1.0) */
                                  const float* v_scale,  /* device, Hkv fp32, may be NULL (= 1.0) */
                                  int B, int Hkv, int G, int Nq, int Ncap, int d, float scale, int causal, int window,
                                  int in_dtype, int out_dtype,
                                  void* workspace, size_t workspace_bytes, void* stream);
int fa_forward_kvcache_paged_fp8_window(const void* Q, const void* Kpool, const void* Vpool, void* O,
                                        float* lse,              /* device, [B,Hkv*G,Nq] fp32, may be NULL */
                                        const int* seqlens_k,    /* device, B int32, may be NULL (= Ncap for all) */
                                        const int* block_table,  /* device, [B,max_pages] int32 */
                                        const float* k_scale,    /* device, Hkv fp32, may be NULL (= 1.0) */
                                        const float* v_scale,    /* device, Hkv fp32, may be NULL (= 1.0) */
                                        int B, int Hkv, int G, int Nq,
                                        int num_pages, int page_size, int max_pages, int d,
                                        float scale, int causal, int window, int in_dtype, int out_dtype,
                                        void* workspace, size_t workspace_bytes, void* stream);

/* KV-cache decode by descriptor: the one-call form of the eight decode entries above, with two options on the logits that the
 * model families with local-attention layers use next to the window -- soft-capped logits (Gemma-2 style) and one learned attention
 * sink per query head (gpt-oss style).  Which of the eight forms a call is follows from the descriptor: block_table (NULL: a
 * contiguous cache of Ncap rows; else pools with num_pages, page_size, max_pages, and Ncap is ignored), kv_dtype (FA_KV_16BIT:
 * K, V elements of in_dtype, k_scale and v_scale must be NULL; FA_KV_FP8_E4M3: one e4m3fn byte per element) and window (0: none).
 * Every field means what the argument of that name means in the flat entries.  `size` must equal sizeof(fa_kvdecode_desc).
 * With sinks == NULL, softcap == 0 and seqlens_q == NULL the call IS the flat entry the descriptor names: same checks, same kernels, same bits.
 * Terms, for row i of query head hq = hkv*G + g: s_j = scale * q.k_j is the logit of key j (scale * k_scale[hkv] * q.k8_j on an
 * fp8 cache), and [lo_i, c_i) are the keys the row sees under the length clamp, the causal flag and the window, as above.
 * softcap   a host float, baked into a captured call like `window`.  0: off.  > 0 and finite: the logit becomes
 *           t_j = softcap * tanh(s_j / softcap) (flash-attn's softcap).  Negative, NaN or inf: hipErrorInvalidValue.  The masks apply
 *           AFTER the cap: a key outside [lo_i, c_i) has weight exactly 0 (tanh(-inf) = -1 never makes a masked key a finite logit).
 *           scale = 0 keeps its meaning (uniform weights over the visible keys, never NaN), a negative scale negates the logits
 *           (tanh is odd), a NaN key behaves as in the base entries.  tanh is computed as 1 - 2 / (1 + e^(2y)) on the hardware
 *           exponential and reciprocal: an absolute error of the order of softcap * 1e-7 on a logit.
 * sinks     a device pointer to Hkv*G fp32 values, or NULL for none.  Head hq has the sink logit a = sinks[hq], in natural-log units
 *           and final: not multiplied by scale or k_scale, not soft-capped.  It is one extra key that every row of the head sees,
 *           with logit a and a zero V row, which no mask or window removes:
 *             O_i = sum_j exp(t_j) v_j / (exp(a) + sum_j exp(t_j)),   lse_i = ln(exp(a) + sum_j exp(t_j)).
 *           A row that sees no key gets O = 0 exactly and lse = a.  a = -inf is "no sink for this head": the head returns what it
 *           returns with sinks == NULL (a row without a key then has lse = -inf; never NaN).  lse is finite and correct for any
 *           finite a, however far above or below the keys' logits: the sink takes part in the reference maximum.  a = +inf or NaN
 *           gives a meaningless result, never an out-of-range access.  The sink counts ONCE per row, whatever the split count.
 *           The vector is read on the device only: a captured call follows a vector that is rewritten in place.  v_scale does not
 *           touch the sink (its V row is zero).
 * Merging over key ranges: the sink is part of lse, so a caller who merges results over disjoint key ranges by the rule of
 * fa_forward_kvcache (O = sum_r O_r exp(lse_r - lse), lse = ln sum_r exp(lse_r)) passes `sinks` to exactly ONE of the ranges.
 * Unchanged from the base entries: the length clamp; what is and is not read (rows past L_b, rows and pages below the window, bad
 * table entries reading as zeros); 64-bit page addresses; the fp8 scales; the folding of the G heads of a group (row r of a K/V head
 * belongs to query head hkv*G + r / Nq); "nothing on the host reads device data"; the split count and the workspace size, which
 * depend on (B, Hkv, G, Nq, capacity or span_cap, d) exactly as before -- fa_kvcache_decode_workspace_bytes returns what the flat
 * sizing function of the descriptor's form returns (0 for a descriptor that is NULL, of the wrong size or of an unknown kv_dtype).
 * Rejected with hipErrorInvalidValue before the device is touched: a NULL descriptor, a wrong `size`, an unknown kv_dtype, scales on
 * a 16-bit cache, a bad softcap, and everything the flat entry of the descriptor's form rejects.
 * seqlens_q   a device pointer to B int32, or NULL.  NULL: every sequence has Nq rows per head, and the call is exactly the one
 *           described above -- same checks, same kernels, same bits.  Else Nq is the PADDED row count and sequence b has
 *           n_b = min(max(seqlens_q[b], 0), Nq) LIVE rows per query head, rows i < n_b (a clamp, never a fault); Q, O [B,Hkv*G,Nq,d] and
 *           lse [B,Hkv*G,Nq] keep their padded layouts.  n_b takes the place of Nq in every limit:
 *             c_i = max(0, L_b - n_b + 1 + i) with causal (L_b without), lo_i = max(0, L_b - n_b + 1 + i - W), start_b = max(0, L_b - n_b + 1 - W),
 *           and what is and is not read below the window follows that start_b.  A live row that sees no key behaves as above (O = 0,
 *           lse = -inf, or the sink logit with sinks).  DEAD rows, i >= n_b, get O = 0 and lse = -inf exactly, with or without sinks;
 *           their Q rows are never used, may hold NaN bit patterns, and cannot move a live row's bits.  n_b = 0 is an idle slot: every
 *           row is dead, and none of the sequence's K/V rows, pages or table entries are read.  After fa_kvcache_append_ex with
 *           seqlens_new pointing at the same vector, row i of sequence b has the causal position L_b(before the append) + i -- its
 *           rotary position there.  Nothing on the host reads seqlens_q: grid, split count and workspace follow the host shape
 *           (the padded Nq; span_cap stays valid because n_b <= Nq), and fa_kvcache_decode_workspace_bytes ignores the field.  The
 *           split count therefore follows the padded G * Nq: a batch padded to a long prefill chunk gives its one-token sequences few
 *           splits.  With every n_b >= Nq the bits are those of the call without seqlens_q.
 *           A descriptor whose `size` is offsetof(fa_kvdecode_desc, seqlens_q) -- the structure before this field existed -- is
 *           accepted and means seqlens_q == NULL; every other wrong size is refused.
 * Not part of this entry: a sink per row or per token, sinks or a soft-cap on the dense prefill entries (fa_forward, fa_forward_ex;
 * the packed prefill has them: fa_forward_varlen_ex), a tanh other than
 * the one above; token-packed (cu_seqlens) layouts (a packed step is fa_kvcache_append_varlen, then fa_kvcache_decode_varlen, below),
 * a split count or a window per sequence, explicit position ids, per-sequence
 * query counts on the prefill entries or on the flat decode entries.  NOT a reference entry point. */
#define FA_KV_16BIT    0   /* K, V elements are of in_dtype */
#define FA_KV_FP8_E4M3 1   /* K, V elements are OCP e4m3fn bytes */
typedef struct fa_kvdecode_desc {
    size_t size;               /* sizeof(fa_kvdecode_desc) */
    const void *Q, *K, *V;     /* K, V: the cache [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d] */
    void* O;
    float* lse;                /* device, [B,Hkv*G,Nq] fp32, may be NULL */
    const int* seqlens_k;      /* device, B int32, may be NULL (= Ncap for all) */
    const int* block_table;    /* device, [B,max_pages] int32; NULL: a contiguous cache */
    const float* k_scale;      /* device, Hkv fp32, may be NULL (= 1.0); fp8 only */
    const float* v_scale;      /* device, Hkv fp32, may be NULL (= 1.0); fp8 only */
    const float* sinks;        /* device, Hkv*G fp32 natural-log logits, may be NULL (none) */
    int kv_dtype;              /* FA_KV_16BIT or FA_KV_FP8_E4M3 */
    int B, Hkv, G, Nq, d;
    int Ncap;                  /* contiguous only */
    int num_pages, page_size, max_pages;   /* paged only */
    float scale;
    int causal, window;
    float softcap;             /* 0: off */
    int in_dtype, out_dtype;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    const int* seqlens_q;      /* device, B int32 live rows per query head, may be NULL (= Nq for all) */
} fa_kvdecode_desc;
size_t fa_kvcache_decode_workspace_bytes(const fa_kvdecode_desc* desc);
int fa_kvcache_decode(const fa_kvdecode_desc* desc);

/* KV-cache append: the write half of a decode step.  Nnew new K and V rows per sequence are written behind the sequence's current
 * length, by one kernel for K and V, into any cache the decode entries above read.
 *   Knew, Vnew      [B, Hkv, Nnew, d] contiguous, fp16 or bf16 (`dtype` / `in_dtype`); d in {64,128}
 *   Kcache, Vcache  [B, Hkv, Ncap, d], resp. Kpool, Vpool [num_pages, Hkv, page_size, d] with block_table [B, max_pages] int32 on the
 *                   device and page_size a power of two >= 16 (Ncap = max_pages * page_size): the layouts of the decode entries.
 *                   Elements are 16 bit of the same `dtype` (the copy keeps every bit, NaN payloads included); on the _fp8 entries one
 *                   byte, OCP e4m3fn.
 *   seqlens_k       device, B int32, or NULL.  L_b = min(max(seqlens_k[b], 0), Ncap), the decode entries' clamp.  NULL means every
 *                   sequence is EMPTY (L_b = 0: a prefill into a fresh cache) -- NOT "full", which is what NULL means to the decode
 *                   entries.
 *   seqlens_out     device, B int32, or NULL: receives min(L_b + Nnew, Ncap).  NULL: no length is written and the caller updates the
 *                   lengths.  It may be exactly seqlens_k (an update in place) or a buffer that does not overlap seqlens_k; a partial
 *                   overlap is hipErrorInvalidValue.  It is written by a second, tiny kernel (ceil(B / 256) workgroups) behind the
 *                   copy on the same stream, launched only when seqlens_out is non-null: no copy thread can see a new length.
 * Placement: token t of sequence b goes to key position p = L_b + t.  A token with p >= Ncap is dropped: it is not written and no
 * address is formed from p.  On the paged entries position p is row p % page_size of page block_table[b][p / page_size]; a table
 * entry outside [0, num_pages) drops the tokens that would land in that page (the write-side counterpart of "reads as zeros"), and
 * table entries are read only for pages that receive a kept token.  Page addresses are 64 bit: a pool may exceed 4 GiB.  Every byte of
 * the cache or pool that is not the destination of a kept token is left as it was.
 * The pages a sequence appends into must be owned by that sequence alone: pages shared between sequences (a common prefix) may only
 * be written by the caller's own copy-on-write.  This is not checked.
 * fp8 entries: the stored code is e4m3fn_RNE(clamp(x / scale[hkv], -448, +448)) with x widened exactly to fp32 and a correctly rounded
 * fp32 division (never a reciprocal) -- ops.quantize_kv_fp8(x, scale) bit for bit, for every finite x.  k_scale, v_scale: device, Hkv
 * fp32 each, or NULL (1.0), read on the device only.  +-inf becomes +-448 (codes 0x7E / 0xFE), a NaN becomes a NaN code (0x7F or
 * 0xFF).  A scale must be finite and > 0; a bad one gives meaningless bytes, never an out-of-range access.
 * Nothing on the host reads seqlens_k, block_table or the scales; the grid depends on (B, Hkv, Nnew, d) only and there is no workspace,
 * so append -> decode with seqlens_out == seqlens_k, captured once into a HIP graph, serves every step of a growing cache.
 * hipErrorInvalidValue, before the device is touched: a null Knew, Vnew, cache or pool, or block_table; B, Hkv, Nnew or Ncap <= 0; d
 * not in {64,128}; a dtype not in {0,1}; an Ncap beyond the decode entries' bound; the paged entries' conditions on page_size,
 * num_pages, max_pages and their product; a source of 2^31 or more 16-byte chunks per tensor (B * Hkv * Nnew * d / 8: the kernel's
 * index type and the grid); the partial overlap of seqlens_out and seqlens_k.
 * Token-major pages, per-token or per-block scales, e5m2, fp8 sources and sliding windows are not part of these entries; nor, on the
 * _rope forms below, are explicit position ids or a per-sequence position offset, 16-bit tables, rotary on the prefill entries
 * (fa_forward*) and a rot_dim that is not a multiple of 16.  NOT reference entry points. */
int fa_kvcache_append(const void* Knew, const void* Vnew, void* Kcache, void* Vcache,
                      const int* seqlens_k,  /* device, B int32, may be NULL (= 0 for all: every sequence empty) */
                      int* seqlens_out,      /* device, B int32, may be NULL or == seqlens_k */
                      int B, int Hkv, int Nnew, int Ncap, int d, int dtype, void* stream);
int fa_kvcache_append_paged(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                            const int* seqlens_k, int* seqlens_out,
                            const int* block_table,  /* device, [B,max_pages] int32 */
                            int B, int Hkv, int Nnew, int num_pages, int page_size, int max_pages,
                            int d, int dtype, void* stream);
int fa_kvcache_append_fp8(const void* Knew, const void* Vnew, void* Kcache, void* Vcache,
                          const int* seqlens_k, int* seqlens_out,
                          const float* k_scale,  /* device, Hkv fp32, may be NULL (= 1.0) */
                          const float* v_scale,  /* device, Hkv fp32, may be NULL (= 1.0) */
                          int B, int Hkv, int Nnew, int Ncap, int d, int in_dtype, void* stream);
int fa_kvcache_append_paged_fp8(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                                const int* seqlens_k, int* seqlens_out, const int* block_table,
                                const float* k_scale, const float* v_scale,
                                int B, int Hkv, int Nnew, int num_pages, int page_size, int max_pages,
                                int d, int in_dtype, void* stream);

/* KV-cache append with rotary position embedding: fa_kvcache_append* with the new token's K rotated at its key position on its way
 * into the cache and the step's Q rows rotated by the same positions, in the same launch.  Each entry is its base entry's list with
 * (Q, Qout, rope_cos, rope_sin) inserted before B and (G, rot_dim, max_pos, interleaved) after d.  V, seqlens_out, placement, the
 * refusals and "nothing on the host reads device data" are the base entry's, unchanged; the grid depends on (B, Hkv, G, Nnew, d) and
 * on whether there is a Q only, and there is no workspace, so append_rope -> decode is captured once like append -> decode.
 *   rope_cos, rope_sin  device fp32 [max_pos, rot_dim/2], contiguous, the caller's: NTK, YaRN or Llama-3 scaling and any magnitude
 *                   factor are whatever the caller put into the table.  Read on the device only.
 *   rot_dim         a multiple of 16 with 16 <= rot_dim <= d.  Elements [rot_dim, d) of a row pass through untouched: on 16-bit caches
 *                   and on Q every bit is kept, as the copy keeps it; on fp8 caches they are quantised as the plain fp8 entry does.
 *   interleaved     0, the half-split (NeoX / HF) convention: pair i is (x[i], x[i + rot_dim/2]); 1, the GPT-J convention: pair i is
 *                   (x[2i], x[2i+1]).  In both, pair i uses c = rope_cos[r][i], s = rope_sin[r][i].
 *   position        token t of sequence b has p = L_b + t (L_b clamped as above, NULL lengths: 0): the position the append places it
 *                   at and the position the decode's causal mask gives query row t after the append.  The table row is
 *                   r = min(p, max_pos - 1): clamp, never fault.  A dropped token (p >= Ncap, or a bad table entry on the paged
 *                   forms) is still not written; its Q row is still rotated, with row r.
 *   Q, Qout         [B, Hkv*G, Nnew, d] contiguous, of the sources' 16-bit dtype (on the fp8 entries too).  Row (b, hq, t) is rotated
 *                   at p = L_b + t and written to the same place of Qout.  Qout == Q rotates in place; Q == NULL && Qout == NULL
 *                   rotates K only; the two buffers must be identical or disjoint, the rule of seqlens_out.
 * Arithmetic, pinned so that the bytes are a contract: the sources are widened exactly to fp32; y1 = fp32(x1*c) - fp32(x2*s) and
 * y2 = fp32(x2*c) + fp32(x1*s), each product and each sum rounded to fp32 on its own -- NO fused multiply-add.  For Q and 16-bit
 * caches one rounding to nearest even into the 16-bit type follows.  For fp8 caches the fp32 y goes into the recipe above,
 * e4m3fn_RNE(clamp(y / scale[hkv], -448, +448)), with no 16-bit rounding in between (one rounding fewer than rotating first and
 * appending afterwards).  This is what element-wise fp32 operators of torch and numpy compute, so a CPU reference reproduces every
 * byte.  A NaN result is a NaN; its payload is not promised.
 * hipErrorInvalidValue, before the device is touched, besides the base entry's: a NULL rope_cos or rope_sin; a rot_dim outside the rule;
 * max_pos <= 0; G <= 0; interleaved not in {0,1}; B * Hkv * G beyond int; 2^31 or more 16-byte chunks in Q; exactly one of Q, Qout
 * NULL; a partial overlap of Q and Qout.  NOT reference entry points. */
int fa_kvcache_append_rope(const void* Knew, const void* Vnew, void* Kcache, void* Vcache,
                           const int* seqlens_k, int* seqlens_out,
                           const void* Q, void* Qout,   /* device, [B,Hkv*G,Nnew,d]; both NULL, identical or disjoint */
                           const float* rope_cos, const float* rope_sin,   /* device, [max_pos,rot_dim/2] fp32 */
                           int B, int Hkv, int Nnew, int Ncap, int d,
                           int G, int rot_dim, int max_pos, int interleaved,
                           int dtype, void* stream);
int fa_kvcache_append_paged_rope(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                                 const int* seqlens_k, int* seqlens_out, const int* block_table,
                                 const void* Q, void* Qout, const float* rope_cos, const float* rope_sin,
                                 int B, int Hkv, int Nnew, int num_pages, int page_size, int max_pages, int d,
                                 int G, int rot_dim, int max_pos, int interleaved,
                                 int dtype, void* stream);
int fa_kvcache_append_fp8_rope(const void* Knew, const void* Vnew, void* Kcache, void* Vcache,
                               const int* seqlens_k, int* seqlens_out,
                               const float* k_scale, const float* v_scale,
                               const void* Q, void* Qout, const float* rope_cos, const float* rope_sin,
                               int B, int Hkv, int Nnew, int Ncap, int d,
                               int G, int rot_dim, int max_pos, int interleaved,
                               int in_dtype, void* stream);
int fa_kvcache_append_paged_fp8_rope(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                                     const int* seqlens_k, int* seqlens_out, const int* block_table,
                                     const float* k_scale, const float* v_scale,
                                     const void* Q, void* Qout, const float* rope_cos, const float* rope_sin,
                                     int B, int Hkv, int Nnew, int num_pages, int page_size, int max_pages, int d,
                                     int G, int rot_dim, int max_pos, int interleaved,
                                     int in_dtype, void* stream);

/* KV-cache append by descriptor: the one-call form of the eight append entries above, with a token count per sequence.  Which of
 * the eight forms a call is follows from the descriptor: block_table (NULL: a contiguous cache of Ncap rows; else pools with
 * num_pages, page_size, max_pages, and Ncap is ignored), kv_dtype (FA_KV_16BIT: cache elements of `dtype`, k_scale and v_scale must be
 * NULL; FA_KV_FP8_E4M3: one e4m3fn byte per element) and rope_cos (NULL: no rotation, and Q, Qout and rope_sin must be NULL too; else
 * the _rope form with Q, Qout, rope_sin, G, rot_dim, max_pos, interleaved).  Every field means what the argument of that name means in
 * the flat entries; `dtype` is their dtype / in_dtype.  `size` must equal sizeof(fa_kvappend_desc).
 * With seqlens_new == NULL the call IS the flat entry the descriptor names: same checks, same kernels, same bytes.
 * seqlens_new  a device pointer to B int32, or NULL.  Nnew is then the PADDED token count (Knew, Vnew [B,Hkv,Nnew,d], Q [B,Hkv*G,Nnew,d]),
 *           and sequence b appends m_b = min(max(seqlens_new[b], 0), Nnew) tokens (a clamp, never a fault).  Token t < m_b goes to
 *           p = L_b + t exactly as in the flat entry: the drops at p >= Ncap and at a bad table entry, the fp8 recipe and the pinned rotary
 *           arithmetic are unchanged.  Token t >= m_b is not written: no address is formed for it and no table entry is read for it, so
 *           a table slot only padding would reach may name a page the sequence does not own; its Q row reaches Qout with every bit
 *           kept.  seqlens_out[b] = min(L_b + m_b, Ncap), in place or disjoint as in the flat entries.  seqlens_new must not overlap
 *           seqlens_out (hipErrorInvalidValue).  Nothing on the host reads seqlens_new; the grid is the flat entry's for the padded Nnew.
 *           fa_kvcache_decode with seqlens_q pointing at the same vector then gives row i the causal position L_b + i.
 * Rejected with hipErrorInvalidValue before the device is touched: a NULL descriptor, a wrong `size`, an unknown kv_dtype, scales on a
 * 16-bit cache, Q, Qout or rope_sin without rope_cos, the overlap above, and everything the flat entry of the descriptor's form rejects.
 * Not part of this entry: explicit position ids, and what the flat entries exclude.  Token-packed (cu_seqlens) sources are
 * fa_kvcache_append_varlen's, below.  NOT a reference entry point. */
typedef struct fa_kvappend_desc {
    size_t size;               /* sizeof(fa_kvappend_desc) */
    const void *Knew, *Vnew;   /* device, [B,Hkv,Nnew,d] of `dtype` */
    void *K, *V;               /* the cache [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d] */
    const int* seqlens_k;      /* device, B int32, may be NULL (= 0 for all: every sequence empty) */
    int* seqlens_out;          /* device, B int32, may be NULL or == seqlens_k */
    const int* seqlens_new;    /* device, B int32 tokens per sequence, may be NULL (= Nnew for all) */
    const int* block_table;    /* device, [B,max_pages] int32; NULL: a contiguous cache */
    const float* k_scale;      /* device, Hkv fp32, may be NULL (= 1.0); fp8 only */
    const float* v_scale;      /* device, Hkv fp32, may be NULL (= 1.0); fp8 only */
    const void* Q;             /* rotary only: device, [B,Hkv*G,Nnew,d]; Q and Qout both NULL, identical or disjoint */
    void* Qout;
    const float* rope_cos;     /* device, [max_pos,rot_dim/2] fp32; NULL: no rotation */
    const float* rope_sin;
    int kv_dtype;              /* FA_KV_16BIT or FA_KV_FP8_E4M3 */
    int B, Hkv, Nnew, d;
    int Ncap;                  /* contiguous only */
    int num_pages, page_size, max_pages;   /* paged only */
    int G, rot_dim, max_pos, interleaved;  /* rotary only */
    int dtype;
    void* stream;
} fa_kvappend_desc;
int fa_kvcache_append_ex(const fa_kvappend_desc* desc);

/* KV-cache append of a token-packed batch: fa_kvcache_append_ex with the sources as the QKV projection leaves them.  Knew, Vnew are
 * packed (total_new, Hkv, d) and, with rotary, Q and Qout (total_new, Hkv*G, d): row (t, h) is d contiguous elements of `dtype` at
 * base + t*stride_t + h*stride_h (strides in ELEMENTS), so views of one fused (total, Hq + 2*Hkv, d) buffer, head-major tensors
 * (stride_t = d) and padded rows are all taken as they lie.  Which of the eight forms a call is follows from block_table, kv_dtype and
 * rope_cos exactly as in fa_kvcache_append_ex, and every field of that name means what it means there.
 * cu_seqlens_new  a device pointer to B+1 int32, read on the device only, clamped as fa_forward_varlen clamps its vectors:
 *           s_b = clamp(cu[b], 0, total_new), e_b = clamp(cu[b+1], s_b, total_new), m_b = e_b - s_b.  Token row t belongs to sequence b
 *           iff s_b <= t < e_b, and is its token i = t - s_b.  A vector that does not ascend places tokens without meaning, but never
 *           forms a source row outside [0, total_new) or a destination outside the cache: i is used only after it was found in [0, m_b).
 * Token i of sequence b goes to p = L_b + i, L_b = clamp(seqlens_k[b], 0, Ncap), exactly as fa_kvcache_append_ex places token i of
 * m_b: dropped at p >= Ncap or behind a table entry outside [0, num_pages); table entries are read only for pages that receive a kept
 * token; page addresses are 64 bit; the fp8 recipe and the pinned rotary arithmetic are those entries'.  Q row (t, hq) is rotated at p
 * (table row min(p, max_pos - 1)), also when the K token is dropped.  seqlens_out[b] = min(L_b + m_b, Ncap).
 * THE BYTES ARE A CONTRACT: for every sequence, the cache or pool bytes, the rotated Q rows and seqlens_out are exactly what
 * fa_kvcache_append_ex writes with seqlens_new[b] = m_b and Nnew = max m_b from the padded head-major copy of the same rows.
 * Rows of no sequence -- before s_0, at or past e_{B-1}, in gaps -- are never used: their K, V and Q rows may hold NaN patterns, and
 * their Qout rows are NOT written (fa_forward_varlen's rule for O, not the ragged append's copy-through).  An empty sequence reads no
 * table entry and writes nothing; its seqlens_out entry is L_b.
 * total_new is a HOST integer, the token rows of Knew, Vnew, Q and Qout and the bound of every source address.  Nothing on the host
 * reads device data; the grid follows (total_new, Hkv, G, d, whether there is a Q) only; there is no workspace; the call is one copy
 * kernel and, with seqlens_out, one tiny lengths kernel.  A captured call follows cu_seqlens_new, the lengths, the table, the scales
 * and the rotary tables when they are rewritten in place within the same total_new.  fa_forward_varlen_kvcache with Q = Qout,
 * cu_seqlens_q = cu_seqlens_new and seqlens_k = seqlens_out is the step's read half: two launches on the projection's own buffer.
 * Rejected with hipErrorInvalidValue before the device is touched: a NULL descriptor or a wrong `size`; everything
 * fa_kvcache_append_ex rejects for the cache and pool geometry, kv_dtype, scales on a 16-bit cache, the rotary fields, and Q, Qout or
 * rope_sin without rope_cos; a NULL cu_seqlens_new; total_new <= 0; a stride_t below d, a negative stride_h, a stride that is not a
 * multiple of 8 elements or a base that is not 16-byte aligned (fa_varlen_desc's rules); total_new*Hkv*d/8 or total_new*Hkv*G*d/8 of
 * 2^31 or more; a Qout that is neither Q with equal strides nor disjoint from Q's address extent; cu_seqlens_new overlapping
 * seqlens_out; a partial overlap of seqlens_out and seqlens_k.
 * Not part of this entry: explicit position ids or per-sequence position offsets, a token-major page layout,
 * per-token or per-page scales, fp8 sources.  (The decode of a packed step is fa_kvcache_decode_varlen's.)  NOT a reference entry point. */
typedef struct fa_kvappend_varlen_desc {
    size_t size;                    /* sizeof(fa_kvappend_varlen_desc) */
    const void *Knew, *Vnew;        /* device, packed: row (t, h) = d elements at base + t*stride_t + h*stride_h */
    void *K, *V;                    /* the cache [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d] */
    const int* cu_seqlens_new;      /* device, B+1 int32 */
    const int* seqlens_k;           /* device, B int32, may be NULL (= 0 for all: every sequence empty) */
    int* seqlens_out;               /* device, B int32, may be NULL; == seqlens_k or disjoint from it */
    const int* block_table;         /* device, [B,max_pages] int32; NULL: a contiguous cache */
    const float *k_scale, *v_scale; /* device, Hkv fp32 each, may be NULL (= 1.0); fp8 only */
    const void* Q; void* Qout;      /* rotary only: packed (total_new, Hkv*G, d) through their own strides; both NULL: K only */
    const float *rope_cos, *rope_sin;   /* device, [max_pos,rot_dim/2] fp32; rope_cos NULL: no rotation */
    int kv_dtype;                   /* FA_KV_16BIT or FA_KV_FP8_E4M3 */
    int B, Hkv, d, total_new;       /* total_new: HOST, the token rows of Knew, Vnew, Q and Qout */
    int Ncap, num_pages, page_size, max_pages;   /* Ncap: contiguous only; the other three: paged only */
    int G, rot_dim, max_pos, interleaved;        /* rotary only */
    int dtype;
    long long k_stride_t, k_stride_h, v_stride_t, v_stride_h,
              q_stride_t, q_stride_h, qo_stride_t, qo_stride_h;   /* ELEMENTS; d contiguous; the q pairs: with Q only */
    void* stream;
} fa_kvappend_varlen_desc;
int fa_kvcache_append_varlen(const fa_kvappend_varlen_desc* desc);

/* fa_kvcache_append_varlen with explicit rotary positions, for a step whose tokens do not sit one behind the other: the drafts of a
 * speculation TREE occupy consecutive cache slots while siblings share a position, their depth.
 * opts == NULL or opts->positions == NULL: the call IS fa_kvcache_append_varlen(desc), bit for bit.
 * With positions: token i of sequence b (token row t = s_b + i) still goes to SLOT L_b + i -- the drop rules, the table reads, the fp8
 * recipe and seqlens_out are the plain entry's -- and its K row and its Q rows (t, hq) are rotated at table row
 * clamp(positions[t], 0, max_pos - 1) in the place of min(L_b + i, max_pos - 1).  The pinned arithmetic is unchanged, so the bytes are
 * those of the plain entry's recipe at that table row, and positions[s_b + i] = L_b + i returns the plain call's bytes.  Positions of
 * rows of no sequence are never read; out-of-range positions clamp and never fault.  positions is read on the device only: a captured
 * call follows it when it is rewritten in place.
 * Rejected with hipErrorInvalidValue before the device is touched: an opts->size other than sizeof(fa_kvappend_varlen_opts);
 * positions without rope_cos; positions that are not 4-byte aligned; everything fa_kvcache_append_varlen rejects.
 * Not part of this entry: positions on the padded fa_kvcache_append_ex; a per-sequence position offset; re-rotating a kept row at
 * another position (fa_kvcache_commit, below, moves the accepted path's rows as they are: depth positions already are the path's
 * final positions).  NOT a reference entry point. */
typedef struct fa_kvappend_varlen_opts {
    size_t size;            /* sizeof(fa_kvappend_varlen_opts) */
    const int* positions;   /* device, [total_new] int32; NULL: position = slot (the plain entry's rule) */
} fa_kvappend_varlen_opts;
int fa_kvcache_append_varlen_ex(const fa_kvappend_varlen_desc* desc, const fa_kvappend_varlen_opts* opts);

/* Merge of attention states over disjoint key ranges: the rule the decode entries above promise (fa_forward_kvcache),
 *   lse = ln sum_r exp(lse_r),   O = sum_r O_r exp(lse_r - lse),
 * applied by ONE kernel to R parts, each an (O_r, lse_r) pair as a decode entry returns it with lse.  A part is addressed by rows:
 * row (b, h, r) of part p is x = b * stride_b + h * stride_h + r with r in [0, rows), its O row is the d elements at O + x * d and
 * its lse is lse[x].  The two strides let one launch read a part laid out [B, H, rows] (what a decode entry returns: stride_b =
 * H * rows, stride_h = rows) next to a part laid out [H, B, rows] (what a decode returns whose BATCH was folded into the rows of one
 * stream over a shared prefix: stride_h = B * rows, stride_b = rows), or a padded one, without a permute copy.  Bytes between the
 * rows a part names are never read.  H counts K/V heads and rows = G * Nq, so a part is exactly a decode entry's O and lse.
 * The parts travel in the kernel's argument block (FA_MERGE_MAX_PARTS * sizeof(fa_state_part) = 512 bytes): `parts` is HOST data that
 * is copied at the call, there is no device allocation, no host-to-device copy and no workspace, the launch is a single kernel that a
 * HIP graph captures, and nothing on the host reads device data.  The grid follows (B, H, rows) only.
 * Arithmetic, in fp32, each part's O widened exactly: M = max_r lse_r (natural-log units), w_r = exp(lse_r - M) on the hardware
 * exponential, L = sum_r w_r, O = (sum_r w_r O_r) / L with a correctly rounded division, lse = M + ln L; O is rounded ONCE, to
 * out_dtype.  The part with the largest lse has weight exactly 1.  Hence:
 *   R = 1            O and lse are the part's bits when part_dtype == out_dtype, else O is the one rounding of the part's bits to
 *                    out_dtype (the sign of a zero included)
 *   one finite part  among parts with lse_r = -inf: it comes through in the same way, exactly
 *   lse_r = -inf     the part is neutral: its O row is selected away, never multiplied -- it may hold NaN bit patterns (the O row of
 *                    a row without a key is 0 in the decode entries, but nothing here relies on that) and cannot move the result
 *   all -inf         O = +0 and lse = -inf exactly, never NaN
 *   lse_r = +inf or NaN   a meaningless row, never an out-of-range access: no address depends on an lse
 * Sinks are not an argument: a sink is part of the lse of the range it was passed to, and the caller passes `sinks` to exactly ONE
 * of the ranges (fa_kvcache_decode).  The output must not alias a part; this is not checked.
 * hipErrorInvalidValue, before the device is touched: a NULL descriptor or a wrong `size`; R outside [1, FA_MERGE_MAX_PARTS]; a null
 * O, or a null O or lse in any of the first R parts; B, H or rows <= 0; d not in {64,128}; a part_dtype or out_dtype that is no
 * FA_STATE_*; a negative stride in any of the first R parts; B * H * rows of 2^26 or more (one wave per row: the grid); an O, or a
 * part's O, that is not aligned to four of its elements (16 bytes for fp32, 8 for the 16-bit types).
 * Shared-prefix decode is a composition of entries above and this one (ops.fa_forward_kvcache_shared_prefix does it): B sequences
 * that share the keys [0, P) of one prefix cache [1, Hkv, Pcap, d] and own a suffix each.  (1) Q [B, Hkv*G, Nq, d] is permuted to
 * [1, Hkv*(B*G), Nq, d] and fa_forward_kvcache runs on the prefix with B = 1, G' = B*G, seqlens_k = the prefix length, causal = 0,
 * no sinks, fp32 O and lse: the batch is folded into the rows of one stream, so the prefix is read once, not B times.  (2) The
 * decode entry of the suffix's form runs as usual (its causal flag, its sinks), fp32 O and lse.  (3) fa_merge_states with H = Hkv,
 * rows = G*Nq: the prefix part has stride_h = B*G*Nq, stride_b = G*Nq, the suffix part stride_b = Hkv*G*Nq, stride_h = G*Nq.  A
 * causal mask is aligned to the end of the suffix, so every row sees the whole prefix.  A window or seqlens_q cannot be composed
 * this way (a window would cross the boundary; a dead row's q would reach the prefix decode).
 * Not part of this entry: parts of different element types in one call, more than FA_MERGE_MAX_PARTS parts (merge twice: the
 * rule is associative), a weight per part other than its lse, any collective.  NOT a reference entry point. */
#define FA_MERGE_MAX_PARTS 16
#define FA_STATE_F16  0   /* as in_dtype elsewhere */
#define FA_STATE_BF16 1
#define FA_STATE_F32  2
typedef struct fa_state_part {
    const void*  O;          /* device; row x of the part is d elements at O + x*d */
    const float* lse;        /* device; natural log, one per row, same row index x */
    long long stride_b, stride_h;   /* in ROWS: row (b, h, r) is x = b*stride_b + h*stride_h + r, r in [0, rows) */
} fa_state_part;
typedef struct fa_merge_desc {
    size_t size;             /* sizeof(fa_merge_desc) */
    fa_state_part parts[FA_MERGE_MAX_PARTS];   /* HOST data, copied into the kernel's arguments at the call */
    int R;                   /* 1 .. FA_MERGE_MAX_PARTS */
    int B, H, rows, d;       /* H = K/V heads, rows = G*Nq rows per K/V head; d in {64,128} */
    int part_dtype;          /* one FA_STATE_* for every part's O */
    void* O;                 /* [B, H, rows, d] contiguous, of out_dtype */
    float* lse;              /* [B, H, rows] fp32, may be NULL */
    int out_dtype;           /* FA_STATE_* */
    void* stream;
} fa_merge_desc;
int fa_merge_states(const fa_merge_desc* desc);

/* Variable-length packed prefill ("varlen"): B sequences of different lengths in ONE call, Q, K and V packed along the token axis
 * and cut by one cu_seqlens vector each for queries and keys, grouped-query heads without an expanded K/V, a causal mask aligned to
 * the end of each sequence's keys, and lse out.  d in {64,128}, fp16 / bf16, O fp32 or 16 bit.
 * Addressing: row (t, h) of a tensor is the d elements at base + t*stride_t + h*stride_h (strides in ELEMENTS, d contiguous), so
 * [total, H, d] (the usual varlen layout), [H, total, d] and padded forms are all expressible without a copy.  Q and O have Hkv*G
 * heads, K and V have Hkv; query head hq = hkv*G + g uses K/V head hkv, as everywhere else in the library.
 * Sequence bounds are clamped, never a fault: for sequence b, s = clamp(cu[b], 0, total) and e = clamp(cu[b+1], s, total), for q
 * (cu_seqlens_q, total_q) and k (cu_seqlens_k, total_k) separately; Lq_b = e_q - s_q and Lk_b = e_k - s_k.  A non-monotone vector
 * gives meaningless results but never an address outside [0, total) rows.
 * Untouched: rows of Q, K and V that belong to no sequence (at or past cu[B]) are never used and may hold NaN patterns; rows of O
 * and lse that belong to no sequence are not written.
 * causal = 0: row i of sequence b sees the keys [0, Lk_b) of that sequence.  causal = 1: row i sees [0, c_i) with
 * c_i = max(0, Lk_b - Lq_b + 1 + i) -- the decode entries' alignment to the END of the keys, so the last query row sees every key
 * and Lq == Lk is the ordinary triangle.  A row with c_i = 0, or with Lk_b = 0, gets O = 0 exactly and lse = -inf, never NaN.
 * lse = ln sum_j exp(scale * q.k_j) over the visible keys, in natural-log units, [Hkv*G, total_q] fp32: row i of sequence b and head
 * hq is lse[hq*total_q + s_q + i], so it feeds fa_merge_states directly (a prompt chunk merged with a decode over a cached prefix).
 * scale keeps the library-wide rule: a negative scale negates the logits; 0 gives uniform weights, never NaN (the host hands the
 * kernel +-FLT_MIN).
 * Nothing on the host reads cu_seqlens_*: the grid depends on (B, Hkv, G, total_q) only -- floor(total_q/128) + B block slots per
 * query head, which a workgroup maps to (sequence, query block) on the device -- and there is no workspace.  A call captured into a
 * HIP graph follows vectors that are rewritten in place later, within the same total_*.  total_q and total_k are HOST integers: the
 * token rows of Q/O resp. K/V, the bound of every address.
 * hipErrorInvalidValue, before the device is touched: a NULL descriptor or a wrong `size`; a null Q, K, V, O or cu_seqlens_*; B,
 * Hkv, G, total_q or total_k <= 0; d not in {64,128}; an in_dtype that is no FA_DTYPE_* or an out_dtype that is no FA_OUT_*; a
 * stride_t below d, a negative stride_h, or any stride that is not a multiple of 8 elements; a base pointer that is not 16-byte
 * aligned; a tensor whose last addressable byte, ((total-1)*stride_t + (H-1)*stride_h + d) * element bytes, does not fit 32 bits
 * (the kernel uses 32-bit buffer offsets); B*Hkv*G, or the block-slot count times Hkv*G, beyond 2^31 - 1 (the grid).
 * Not part of this entry: a window, sinks, a soft-cap, fp8, a paged K/V, rotary, max_seqlen hints, dropout.  The first three are
 * fa_forward_varlen_ex's, below, which takes this descriptor and a small structure of options; K/V in the KV cache, contiguous or
 * paged, is fa_forward_varlen_kvcache's, further below.  NOT a reference entry point. */
typedef struct fa_varlen_desc {
    size_t size;                    /* sizeof(fa_varlen_desc); any other value is refused */
    const void *Q, *K, *V;          /* device, 16-bit of in_dtype */
    void* O;                        /* device, of out_dtype (FA_OUT_F32 / FA_OUT_SAME) */
    float* lse;                     /* device, [Hkv*G, total_q] fp32 contiguous, may be NULL */
    const int* cu_seqlens_q;        /* device, B+1 int32 */
    const int* cu_seqlens_k;        /* device, B+1 int32; may be the same pointer as cu_seqlens_q */
    int B, Hkv, G, d;               /* d in {64,128} */
    int total_q, total_k;           /* HOST: token rows in Q/O resp. K/V; the bound of every address */
    long long q_stride_t, q_stride_h, k_stride_t, k_stride_h,
              v_stride_t, v_stride_h, o_stride_t, o_stride_h;   /* in ELEMENTS; d is contiguous */
    float scale; int causal;
    int in_dtype, out_dtype;
    void* stream;
} fa_varlen_desc;
int fa_forward_varlen(const fa_varlen_desc* desc);

/* fa_forward_varlen with the three options on the logits that the local-attention model families use and fa_kvcache_decode already
 * has: a sliding window, soft-capped logits (Gemma-2 style) and one attention sink per query head (gpt-oss style), so that a
 * prompt is prefilled by the arithmetic its tokens are decoded with.  `desc` means what it means above.  The semantics are the
 * decode side's, with Lq_b in the place of Nq and Lk_b in the place of L_b.
 * opts == NULL, or window == 0, softcap == 0 and sinks == NULL: the call IS fa_forward_varlen(desc): same checks, same kernels,
 * same bits.  `size` must equal sizeof(fa_varlen_opts).
 * window    a host int, baked into a captured call.  0: none.  W >= 1: row i of sequence b sees the keys [lo_i, c_i) with
 *           lo_i = max(0, Lk_b - Lq_b + 1 + i - W) and c_i as above (Lk_b without causal, max(0, Lk_b - Lq_b + 1 + i) with it).  The
 *           lower limit is the same with and without causal: flash-attn's window_size (W-1, 0) with causal = 1 and (W-1, -1) with
 *           causal = 0, as fa_forward_kvcache_window has it.  lo_i < c_i whenever c_i >= 1.  W >= Lk_b + Lq_b for every b returns the
 *           bits of the same call with window == 0.  W < 0: hipErrorInvalidValue.  One W for all sequences and heads.
 *           What is read: the K/V rows of a sequence below the 64-key tile that holds the first visible key of a 128-row query block
 *           are not read for that block.  A key below a row's lo_i inside a tile that is read is a masked score (weight exactly 0),
 *           but its K and V rows are used as they are: a NaN there behaves like a NaN in any other key of fa_forward_varlen.
 * softcap   a host float, baked into a captured call.  0: off.  > 0 and finite: the logit becomes
 *           t_j = softcap * tanh(s_j / softcap) with s_j = scale * q.k_j, by fa_kvcache_decode's formula (1 - 2 / (1 + e^(2y)) on the
 *           hardware exponential and reciprocal).  The masks apply AFTER the cap: a key outside [lo_i, c_i) has weight exactly 0.
 *           scale = 0 keeps its meaning (uniform weights), a negative scale negates the logits (tanh is odd).  Negative, NaN or inf:
 *           hipErrorInvalidValue.
 * sinks     a device pointer to Hkv*G fp32 values, or NULL for none.  Head hq has the sink logit a = sinks[hq], in natural-log units
 *           and final: not multiplied by scale, not soft-capped.  It is one extra key that every row of the head sees, with logit a
 *           and a zero V row, which no mask or window removes:
 *             O_i = sum_j exp(t_j) v_j / (exp(a) + sum_j exp(t_j)),   lse_i = ln(exp(a) + sum_j exp(t_j)).
 *           A row of a sequence that sees no key gets O = 0 exactly and lse = a.  a = -inf is "no sink for this head": the head
 *           returns the bits it returns with sinks == NULL.  The sink counts ONCE per row.  The vector is read on the device only: a
 *           captured call follows a vector that is rewritten in place.  Rows of O and lse that belong to no sequence stay unwritten.
 *           The sink is part of lse: a caller who merges this result with others through fa_merge_states passes `sinks` to one
 *           of the parts only.
 * Unchanged: nothing on the host reads device data; the grid depends on (B, Hkv, G, total_q) only; no workspace; one kernel; the
 * clamps of the sequence bounds; a captured call follows cu_seqlens_* and sinks that are rewritten in place.
 * hipErrorInvalidValue, before the device is touched: a wrong opts->size, window < 0, a bad softcap, and everything
 * fa_forward_varlen rejects.
 * Not part of this entry: a window that crosses into a separately cached prefix (a prompt chunk merged with a decode over a cached
 * prefix through fa_merge_states cannot carry a window over the boundary), a window per sequence or per head, fp8 or paged K/V,
 * rotary.  The window across a cached prefix and the 16-bit paged K/V are fa_forward_varlen_kvcache's, below.  NOT a reference
 * entry point. */
typedef struct fa_varlen_opts {
    size_t size;          /* sizeof(fa_varlen_opts); any other value is refused */
    const float* sinks;   /* device, Hkv*G fp32 natural-log logits, or NULL */
    int window;           /* 0: none; W >= 1 */
    float softcap;        /* 0: off; > 0 and finite */
} fa_varlen_opts;
int fa_forward_varlen_ex(const fa_varlen_desc* desc, const fa_varlen_opts* opts);

/* The varlen prefill against the KV cache: fa_forward_varlen_ex with the K/V rows of sequence b taken from the cache the decode and
 * append entries use -- a contiguous cache [B,Hkv,Ncap,d], or with `block_table` the page pools [num_pages,Hkv,page_size,d] -- in
 * the place of packed K/V tensors.  One launch covers chunked prefill (a long prompt fed in pieces, each attending to what is
 * cached plus itself: fa_kvcache_append* the chunk, then this call with causal = 1), prefix caching (only the uncached suffix of a
 * prompt is computed, over cached pages) and a window that runs across the boundary between cached and new tokens.
 * Semantics: exactly fa_forward_varlen_ex's, with one substitution.  Lq_b comes from cu_seqlens_q under the clamps above;
 * Lk_b = clamp(seqlens_k[b], 0, Ncap), with Ncap = max_pages*page_size when paged, counts the keys of sequence b in the cache, the
 * chunk's own tokens INCLUDED (the lengths after the append).  Key j of sequence b is cache row j: K[b][hkv][j], or when paged row
 * j % page_size of page block_table[b*max_pages + j / page_size].  Row i sees [lo_i, c_i): c_i = Lk_b, or max(0, Lk_b - Lq_b + 1 + i)
 * under causal; lo_i = max(0, Lk_b - Lq_b + 1 + i - W) under a window W, else 0.  So row i of an appended chunk sees the cached prefix
 * and the chunk up to itself, and a window simply runs across the prefix boundary.  A row without a key returns O = 0 exactly and
 * lse = -inf; with a sink, lse is the sink logit.  The lse layout, the scale rule, soft-cap before the masks and the sink counting
 * once per row are fa_forward_varlen_ex's.  sinks, window, softcap: fa_varlen_opts' three, same meaning; NULL / 0 / 0: off, and the
 * call runs the plain kernels.
 * Bits: on the same finite keys and the same options the entry returns the bits of fa_forward_varlen / fa_forward_varlen_ex on the
 * gathered packed K/V, for O and lse (tiles stay at absolute multiples of 64 keys from key 0), and the paged form returns the bits of
 * the contiguous form.
 * What is read -- the decode entries' contract: nothing on the host reads device data; the grid comes from (B, Hkv, G, total_q)
 * only; there is no workspace; it is one kernel.  A captured call follows cu_seqlens_q, seqlens_k, block_table and sinks when they
 * are rewritten in place.  Table entries at or past ceil(Lk_b / page_size) are never read; rows at or past Lk_b are never used.
 * Under a window, for a 128-row query block: K/V rows below the lo of its first row are never used -- the rows of the first
 * streamed 64-key tile that lie below that lo reach the arithmetic as zeros (a freed page may hold NaN, and 0 * NaN is NaN) -- and
 * the table entry of a page wholly below that lo is not read.  Therefore pages wholly below lo_0 = max(0, Lk_b - Lq_b + 1 - W) may
 * be freed.  A live table entry outside [0, num_pages) reads as a page of zeros.  Page addresses are 64 bit; only the offset inside
 * one page-head block is 32 bit.
 * hipErrorInvalidValue, before the device is touched: everything fa_forward_varlen_ex refuses for Q, O, lse, B, Hkv, G, d, the
 * dtypes, window and softcap; a wrong `size`; a null K, V or seqlens_k, or a K or V that is not 16-byte aligned; contiguous:
 * Ncap <= 0; paged: a page_size that is no power of two >= 16, num_pages <= 0, max_pages <= 0, or max_pages*page_size beyond
 * 2^31 - 1; a capacity whose rows of one (sequence, head), Ncap*d*2 bytes, do not fit 32 bits.  Ncap, num_pages, page_size and
 * max_pages of the other form are ignored.
 * Not part of this entry: fp8 caches; split-KV for a short chunk on a very long cache (that is fa_kvcache_decode_varlen on
 * the same packed Q -- see README for the crossover); rotary (fa_kvcache_append_ex rotates on the way into the cache); a window per sequence
 * or per head.  (An fp8 cache has an entry of its own on this descriptor: fa_forward_varlen_kvcache_fp8, below.)  NOT a reference
 * entry point. */
typedef struct fa_varlen_kvcache_desc {
    size_t size;                  /* sizeof(fa_varlen_kvcache_desc); any other value is refused */
    const void* Q; void* O; float* lse;      /* as in fa_varlen_desc: Q,O packed (total_q, Hkv*G, d); lse [Hkv*G,total_q] or NULL */
    const void *K, *V;            /* cache [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d]; 16 bit of in_dtype */
    const int* cu_seqlens_q;      /* device, B+1 */
    const int* seqlens_k;         /* device, B: keys of sequence b in the cache, the chunk's own tokens INCLUDED (i.e. after the append) */
    const int* block_table;       /* device [B,max_pages] int32, or NULL: contiguous cache */
    int B, Hkv, G, d, total_q, Ncap, num_pages, page_size, max_pages;
    long long q_stride_t, q_stride_h, o_stride_t, o_stride_h;
    float scale; int causal; int in_dtype, out_dtype;
    const float* sinks; int window; float softcap;   /* fa_varlen_opts' three, same meaning; 0/NULL: off */
    void* stream;
} fa_varlen_kvcache_desc;
int fa_forward_varlen_kvcache(const fa_varlen_kvcache_desc* desc);

/* fa_forward_varlen_kvcache on an fp8 cache -- the cache fa_kvcache_append_fp8 / _paged_fp8 write and fa_forward_kvcache_fp8 /
 * _paged_fp8 read -- so that a stack that keeps its cache in fp8 runs chunked prefill and prefix caching without widening it first.
 * The descriptor is fa_varlen_kvcache_desc as it is, and every field means what it means above, with these differences:
 *   K, V      one OCP e4m3fn byte per element: [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d].
 *   in_dtype  remains the type of Q: the codes are widened to it (exactly: every e4m3fn value is a normal fp16 and bf16 number)
 *             on the way into LDS, and P is packed to it.
 *   k_scale, v_scale   device pointers to Hkv fp32 each, or NULL for 1.0.  Read on the device only: a captured call follows scales
 *             that are rewritten in place.  They must be finite and > 0 (the caller's contract, as in the fp8 decode entries).
 * Semantics: fa_forward_varlen_kvcache's with the decode side's fp8 rule.  The logits are scale * k_scale[hkv] * q.k8; the factor
 * that goes to the device is clamped to +-FLT_MIN AFTER the product with k_scale, so scale = 0 still gives uniform weights under
 * every mask.  Soft-cap, masks and sinks follow after that; the sinks take neither scale.  O = v_scale[hkv] * softmax.v8, and lse is
 * that of the scaled logits (v_scale is no part of it).  With NULL scales the entry returns the bits of fa_forward_varlen_kvcache on
 * the widened cache, for O and lse, and the paged form returns the bits of the contiguous form.
 * Unchanged: the lengths include the chunk; the causal and window limits; rows without a key; table entries that are never read;
 * pages wholly below lo_0 may be freed; a live table entry outside [0, num_pages) reads as a page of zeros; nothing on the host
 * reads device data; one kernel; no workspace; the grid from (B, Hkv, G, total_q).  A freed page may hold the NaN codes 0x7F / 0xFF:
 * the rows at or past Lk_b, the rows of the first streamed tile below the lo of a query block's first row, and the pages wholly
 * below it reach the arithmetic as zeros because their RAW bytes are zeroed (or never loaded) before the widening.
 * hipErrorInvalidValue, before the device is touched: exactly what fa_forward_varlen_kvcache refuses, K and V that are not 16-byte
 * aligned included.  The capacity bound stays Ncap*d*2 bytes in 32 bits although a row is d bytes here: every 32-bit limit derived
 * from it (the byte offsets, |Lk - Lq + 1 + i| <= 2^26, the window clamp total_q + Ncap <= 2^27) then holds unchanged.
 * Not part of this entry: split-KV for a short chunk on a very long cache (that stays with fa_kvcache_decode and its seqlens_q);
 * per-token or per-page scales; an fp8 Q or fp8 MFMAs; rotary (the append rotates).  NOT a reference entry point. */
int fa_forward_varlen_kvcache_fp8(const fa_varlen_kvcache_desc* desc, const float* k_scale, const float* v_scale);

/* Token-packed split-KV decode against the KV cache: the read half of fa_kvcache_append_varlen for a step whose sequences bring few
 * rows each -- a pure decode step (one token per sequence), speculative or multi-token decode, a short chunk beside decode tokens.
 * It is fa_kvcache_decode with seqlens_q -- the split-KV stream, the G heads of a group folded into the rows, every cache form --
 * with Q, O and lse in the packed layout of fa_forward_varlen_kvcache, cut by cu_seqlens_q on the device, so that the rotated Q left
 * in a fused QKV buffer by the append goes in as it lies and O comes out token-major.
 * The descriptor carries everything fa_kvdecode_desc carries about the cache and the options, with the same meaning (K, V,
 * seqlens_k, block_table, k_scale, v_scale, sinks, kv_dtype, B, Hkv, G, d, Ncap or num_pages / page_size / max_pages, scale, causal,
 * window, softcap, in_dtype, out_dtype, workspace, workspace_bytes, stream), and in the place of the padded Q, O, lse, Nq and
 * seqlens_q the packed fields of fa_varlen_kvcache_desc: Q, O (total_q, Hkv*G, d) through q_stride_t, q_stride_h, o_stride_t,
 * o_stride_h (elements, d contiguous), lse [Hkv*G, total_q] fp32 or NULL, cu_seqlens_q (device, B+1 int32), total_q -- and one new
 * host integer, max_q: the most rows any sequence may have, which plays the part Nq plays as the padded count.
 * Semantics: [s_b, e_b) are fa_forward_varlen's clamps of cu_seqlens_q into [0, total_q] (s_b = clamp(cu[b]), e_b = clamp(cu[b+1])
 * and never below s_b), n_b = min(e_b - s_b, max_q), and row i < n_b of sequence b is token s_b + i.  On those rows the call IS
 * fa_kvcache_decode with Nq = max_q and seqlens_q[b] = n_b, run on the padded head-major copy [B,Hkv*G,max_q,d] of the same Q rows:
 * the same c_i = max(0, L_b - n_b + 1 + i) with causal (L_b without), lo_i = max(0, L_b - n_b + 1 + i - W) and
 * start_b = max(0, L_b - n_b + 1 - W); the same rules for what is and is not read below the window and past L_b; the sink counted
 * once per row; the soft-cap before the masks; the fp8 scale rules; a row without a key is O = 0, lse = -inf (the sink logit with
 * sinks).  It returns that call's BITS for O and lse, for every split count, contiguous and paged, 16-bit and e4m3fn caches, and
 * with every n_b = max_q.
 * Tokens that are no live row of any sequence -- before s_0, between or behind sequences, at or past s_b + max_q of a sequence that
 * is longer than max_q -- are left alone: their Q rows are never loaded and may hold NaN bit patterns, and their O rows and lse
 * entries are NEVER WRITTEN.  (The padded entry writes zeros and -inf into its dead rows; this one has no dead rows to own, as
 * fa_forward_varlen has "rows of no sequence".)  n_b = 0 is an idle slot: none of the sequence's K/V rows, pages or table entries are
 * read.  Sequences should own disjoint token ranges; where two overlap, each writes its result and the last store wins.
 * Nothing on the host reads device data.  Grid, split count and workspace follow (B, Hkv, G, max_q, capacity or span_cap, d) exactly
 * as fa_kvcache_decode's do with Nq = max_q, so the split count follows G * max_q: size max_q to the step, not to the longest
 * prompt.  fa_kvcache_decode_varlen_workspace_bytes returns what fa_kvcache_decode_workspace_bytes returns for that padded
 * descriptor (0 for a descriptor that is NULL, of the wrong size or of an unknown kv_dtype).  A captured call follows cu_seqlens_q,
 * seqlens_k, the block table, the scales and the sinks when they are rewritten in place; total_q, max_q, window and softcap are host
 * values.
 * hipErrorInvalidValue, before the device is touched: a NULL descriptor; any `size` but sizeof(fa_kvdecode_varlen_desc); an unknown
 * kv_dtype; scales on a 16-bit cache; everything fa_kvcache_decode of the same form refuses with Nq = max_q (null Q, K, V or O, bad
 * B, Hkv, G, d, causal, dtypes, window < 0, a bad softcap, a bad capacity or page geometry, G * max_q rows beyond the 32-bit
 * workspace offsets); fa_forward_varlen's checks on the packed Q and O (16-byte aligned, stride_t >= d, stride_h >= 0, strides
 * multiples of 8 elements, the last byte of the tensor inside 32 bits); a NULL cu_seqlens_q; total_q <= 0 or max_q <= 0; a
 * (sequence, K/V head) view -- (min(max_q, total_q) - 1) * stride_t + Hkv*G * stride_h + d elements of Q or of O -- whose bytes
 * do not fit 32 bits with 512 to spare.
 * Not part of this entry: a shared prefix (fa_merge_states composes one); a split count per sequence; splitting the keys inside the
 * prefill kernel; explicit position ids.  (The choice between this entry and fa_forward_varlen_kvcache per sequence, on the device,
 * is fa_kvcache_attend_varlen, below.)  NOT a reference entry point. */
typedef struct fa_kvdecode_varlen_desc {
    size_t size;               /* sizeof(fa_kvdecode_varlen_desc); any other value is refused */
    const void* Q; void* O;    /* packed (total_q, Hkv*G, d) through the strides below */
    float* lse;                /* device, [Hkv*G, total_q] fp32, may be NULL */
    const void *K, *V;         /* the cache [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d] */
    const int* cu_seqlens_q;   /* device, B+1 int32 */
    const int* seqlens_k;      /* device, B int32, may be NULL (= the capacity for all) */
    const int* block_table;    /* device, [B,max_pages] int32; NULL: a contiguous cache */
    const float* k_scale;      /* device, Hkv fp32, may be NULL (= 1.0); fp8 only */
    const float* v_scale;      /* device, Hkv fp32, may be NULL (= 1.0); fp8 only */
    const float* sinks;        /* device, Hkv*G fp32 natural-log logits, may be NULL (none) */
    int kv_dtype;              /* FA_KV_16BIT or FA_KV_FP8_E4M3 */
    int B, Hkv, G, d;
    int total_q;               /* token rows of Q and O */
    int max_q;                 /* the most rows a sequence may have: n_b = min(e_b - s_b, max_q) */
    int Ncap;                  /* contiguous only */
    int num_pages, page_size, max_pages;   /* paged only */
    long long q_stride_t, q_stride_h, o_stride_t, o_stride_h;   /* elements */
    float scale;
    int causal, window;
    float softcap;             /* 0: off */
    int in_dtype, out_dtype;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} fa_kvdecode_varlen_desc;
size_t fa_kvcache_decode_varlen_workspace_bytes(const fa_kvdecode_varlen_desc* desc);
int fa_kvcache_decode_varlen(const fa_kvdecode_varlen_desc* desc);

/* fa_kvcache_decode_varlen with a tree mask: the verify step of tree speculation (Medusa, EAGLE, SpecInfer), where a token sees the
 * committed context plus its own ancestors among the step's tokens and not every earlier token of the step.
 * opts == NULL or opts->tree_mask == NULL: the call IS fa_kvcache_decode_varlen(desc) -- same checks, same kernels, same bits.
 * With a mask: s_b, n_b, L_b are fa_kvcache_decode_varlen's (L_b includes the step's own tokens) and base_b = L_b - n_b, which may be
 * negative; token s_b + j is the key at cache position base_b + j.  For row i < n_b
 *   m_i = (tree_mask[s_b + i] & low n_b bits) | (1 << i):  bits at or above n_b are ignored, a token always sees itself, bits above i
 *         are legal, and nothing checks that the mask is ancestor-closed;
 *   row i sees key k iff 0 <= k < L_b, k >= lo_i and (k < base_b -- committed context, always visible -- or bit k - base_b of m_i);
 *   lo_i = max(0, base_b + popcount(m_i) - W) under a window W (0 without): for an ancestor-closed mask popcount(m_i) - 1 is the
 *         token's depth, so the window is measured from the token's position in its own branch; start_b = max(0, base_b + 1 - W) as
 *         in the plain entry, and no row reaches below it.
 * Everything else is fa_kvcache_decode_varlen's: the soft-cap before the masks, the sink once per row, the fp8 scale rules; a row
 * without a key (possible with base_b + i < 0) is O = 0, lse = -inf or the sink logit; tokens of no sequence are neither read nor
 * written, their mask words included; n_b = 0 reads nothing; split count, grid and workspace follow (B, Hkv, G, max_q, span) only, so
 * fa_kvcache_decode_varlen_workspace_bytes(desc) sizes the workspace of this entry too; nothing on the host reads device data, and a
 * captured call follows tree_mask when it is rewritten in place.
 * BITS: with tree_mask[s_b + i] = (1 << (i + 1)) - 1 on every live row the call returns the bits of fa_kvcache_decode_varlen with
 * causal = 1, for O and lse, for every split count, contiguous and paged, 16-bit and e4m3fn, with and without window, sinks, soft-cap.
 * hipErrorInvalidValue, before the device is touched: an opts->size other than sizeof(fa_kvdecode_tree_opts); with a mask,
 * causal != 1 (the tree takes the triangle's place), max_q > 64, or a tree_mask that is not 8-byte aligned; everything
 * fa_kvcache_decode_varlen refuses.
 * Not part of this entry: trees of more than 64 tokens per sequence, or a dense or bit-packed [n, n] mask; a mask on the prefill
 * entries or on the padded fa_kvcache_decode; per-head masks; a shared prefix under a tree; a commit after verification by
 * page-table edits (the commit by copies is fa_kvcache_commit, below).  NOT a reference entry point. */
typedef struct fa_kvdecode_tree_opts {
    size_t size;                          /* sizeof(fa_kvdecode_tree_opts); any other value is refused */
    const unsigned long long* tree_mask;  /* device, [total_q] 64-bit words, one per token row; NULL: no tree */
} fa_kvdecode_tree_opts;
int fa_kvcache_decode_varlen_ex(const fa_kvdecode_varlen_desc* desc, const fa_kvdecode_tree_opts* opts);

/* The mixed step: ONE attention call for the batch a continuous-batching scheduler packs on every iteration -- a few prompt chunks of
 * some hundred rows beside many one-token decodes -- with each sequence routed ON THE DEVICE to the stream that suits its row count.
 * fa_kvcache_append_varlen then fa_kvcache_attend_varlen is the two-call step of a serving loop, whatever mix was packed.
 * The descriptor is fa_kvdecode_varlen_desc as it is, and every field means what it means above, with one difference: max_q is the
 * routing threshold T.  [s_b, e_b) are the clamps of cu_seqlens_q both existing entries apply, and span_b = e_b - s_b:
 *   span_b = 0          the sequence has no rows: an idle slot, nothing of it is read;
 *   1 <= span_b <= T    SHORT: the packed split-KV stream (fa_kvcache_decode_varlen's kernels);
 *   span_b > T          LONG: the tiled kernel (fa_forward_varlen_kvcache's), one workgroup per (128-row block, query head).
 * Every token of every sequence is a live row: NOTHING is cut at T.  Row i of sequence b sees the keys [lo_i, c_i) with
 * c_i = max(0, L_b - span_b + 1 + i) and lo_i = max(0, L_b - span_b + 1 + i - W) under a window W, else 0 -- the one formula both existing entries already share, as they share the soft-cap before the masks, the sink counted once per row, the
 * fp8 scale rules and "a row without a key is O = 0, lse = -inf (the sink logit with sinks)".
 * BITS: on the rows of a SHORT sequence the call returns the bits of fa_kvcache_decode_varlen(desc) with the same descriptor, for O
 * and lse; on the rows of a LONG sequence the bits of fa_forward_varlen_kvcache on the same fields -- for kv_dtype FA_KV_FP8_E4M3
 * those of fa_forward_varlen_kvcache_fp8 with the descriptor's scales.  window = 0 maps as each entry maps it.
 * Tokens of no sequence are neither read nor written, as in both entries.
 * Parts: fa_kvcache_attend_varlen(desc) is fa_kvcache_attend_varlen_part(desc, FA_ATTEND_SHORT | FA_ATTEND_LONG).  FA_ATTEND_SHORT alone
 * computes and writes the SHORT rows only, FA_ATTEND_LONG alone the LONG rows only: the rows of the other class keep their bytes, and
 * for the skipped class no Q row, no K/V row and no table entry is read.  This is the form for a caller who puts the bandwidth-bound
 * half and the compute-bound half on two streams.
 * Launches, all on desc->stream, the SHORT half first (the halves write disjoint rows, so the order does not show in the result):
 * the SHORT half is the packed split-KV stream plus its merge when the split count exceeds 1, with grid, split count and workspace
 * from (B, Hkv, G, T, span) exactly as fa_kvcache_decode_varlen derives them from max_q -- so
 * fa_kvcache_decode_varlen_workspace_bytes(desc) sizes the workspace of this entry; the workgroups of a LONG sequence return before
 * any table entry, K/V row or Q row is read, and its merge waves return without writing.  The LONG half is the one launch of the tiled
 * kernel with its grid from (B, Hkv, G, total_q); a workgroup whose sequence has span_b <= T returns right after the slot search.
 * With total_q <= T no sequence can be LONG and the LONG half is not launched: a rule on host integers alone.  Nothing on the host
 * reads device data; a captured call follows cu_seqlens_q, seqlens_k, the block table, the scales and the sinks when they are
 * rewritten in place, a sequence changing class included; total_q, T, window and softcap are host values.
 * hipErrorInvalidValue, before the device is touched: everything fa_kvcache_decode_varlen refuses for this descriptor, a missing or
 * short workspace included, whichever parts are asked for; everything fa_forward_varlen_kvcache[_fp8] refuses for the same fields --
 * its 32-bit bounds on Q, O and the capacity cover all total_q rows, not T of them; causal != 1 (a mixed step is causal); a NULL
 * seqlens_k; parts outside {1, 2, 3}.
 * Not part of this entry: a tree mask (the tree step keeps fa_kvcache_decode_varlen_ex); a threshold per sequence; key splits for
 * LONG sequences; a shared prefix; concurrency of the two halves managed by the library (the caller has _part for that).  NOT a
 * reference entry point. */
#define FA_ATTEND_SHORT 1   /* the split-KV half */
#define FA_ATTEND_LONG  2   /* the tiled half    */
int fa_kvcache_attend_varlen(const fa_kvdecode_varlen_desc* desc);            /* == _part(desc, 3) */
int fa_kvcache_attend_varlen_part(const fa_kvdecode_varlen_desc* desc, int parts);

/* The commit step of tree speculation: after fa_kvcache_append_varlen_ex placed a step's n_b tokens at slots L_b .. L_b + n_b - 1 in
 * tree order and fa_kvcache_decode_varlen_ex verified them, one root-to-node path per sequence is kept.  This entry moves that path's
 * K/V rows to the consecutive slots behind L_b and writes the new lengths, so that every other entry reads the sequence as the dense
 * range [0, L_b + a_b) again.  append -> tree decode -> commit, captured once, serves every step on all four cache forms.
 * L_b = clamp(seqlens_k[b], 0, cap), cap = Ncap or, with block_table, max_pages * page_size: the append's clamp, on the lengths
 *           BEFORE the step (what the append read; NULL: 0 for all).
 * accept_mask  a device pointer to B 64-bit words, one per SEQUENCE.  Bit i names the step token the append placed at slot L_b + i.
 *           w_b = the word restricted to the bits i < max_new with L_b + i < cap: bits at or above max_new are ignored, and tokens the
 *           append dropped at the capacity are ignored and not counted.  a_b = popcount(w_b).  The word of a tree node as
 *           fa_kvcache_decode_varlen_ex takes it (the node's own bit and its ancestors') is the word that keeps the path to that node.
 * With i_0 < i_1 < ... the set bits of w_b: for every K/V head, for K and for V, row L_b + i_j is copied to row L_b + j.  A row is d
 *           elements, 16 bit or one e4m3fn byte: kv_dtype and d matter through the row's size alone, and every bit is kept, NaN
 *           payloads and NaN codes included.  The copy behaves as if all sources were read before any destination was written: {1,3}
 *           makes slot L_b + 1 the source of j = 0 and the destination of j = 1.
 * A move with i_j == j touches nothing.  A word that is a low-bit prefix (0, a fully accepted chain, a step of linear speculation)
 *           reads and writes no cache byte and no table entry: the call is a pure length update, so one captured graph serves linear
 *           and tree steps.
 * Paged: slots map to pages exactly as in the append, addresses are 64 bit.  Table entries are read only for the pages that hold the
 *           source or the destination of a move with i_j != j.  An entry outside [0, num_pages) skips that move: no address is formed
 *           from it, the destination keeps its bytes, and the move still counts in a_b.  The pages a sequence moves rows within must
 *           be owned by that sequence alone (the append's rule).
 * seqlens_out[b] = L_b + a_b, by a tiny second kernel behind the copy, as in the appends: seqlens_out may be NULL, seqlens_k itself
 *           or disjoint from it.
 * Every byte that is not the destination of a move with i_j != j is left as it was: slots at and past L_b + a_b keep whatever the
 *           step left there.  Nothing is read on the host and there is no workspace; the grid follows (B, Hkv, d, kv_dtype, max_new)
 *           only; a captured call follows the words, the lengths and the table when they are rewritten in place.
 * Rejected with hipErrorInvalidValue before the device is touched: a NULL descriptor or a wrong `size`; a NULL K, V or accept_mask; an
 * accept_mask that is not 8-byte aligned; max_new outside 1..64; everything fa_kvcache_append_ex rejects for the cache and pool
 * geometry, d, dtype and kv_dtype; a partial overlap of seqlens_out and seqlens_k; an accept_mask that overlaps seqlens_out.
 * Not part of this entry: trees above 64 tokens; a commit by page-table edits; moving rows between sequences; compacting the Q or O
 * rows of the step; re-rotating a moved K row.  NOT a reference entry point. */
typedef struct fa_kvcommit_desc {
    size_t size;                            /* sizeof(fa_kvcommit_desc) */
    void *K, *V;                            /* the cache [B,Hkv,Ncap,d], or with block_table the pools [num_pages,Hkv,page_size,d] */
    const int* seqlens_k;                   /* device, B int32: the lengths BEFORE the step (what the append read); NULL = 0 for all */
    int* seqlens_out;                       /* device, B int32; NULL, == seqlens_k, or disjoint from it */
    const unsigned long long* accept_mask;  /* device, B 64-bit words, one per SEQUENCE */
    const int* block_table;                 /* device, [B,max_pages] int32; NULL: a contiguous cache */
    int kv_dtype;                           /* FA_KV_16BIT or FA_KV_FP8_E4M3: only the element size matters */
    int dtype;                              /* the 16-bit element type, as in fa_kvcache_append_ex */
    int B, Hkv, d, max_new;                 /* max_new: HOST, 1..64; bits at or above it are ignored */
    int Ncap, num_pages, page_size, max_pages;   /* Ncap: contiguous only; the other three: paged only */
    void* stream;
} fa_kvcommit_desc;
int fa_kvcache_commit(const fa_kvcommit_desc* desc);

/* Multi-head latent attention (MLA) decode, as DeepSeek-V2/V3/R1 and Kimi K2 serve it: the cache holds ONE row per token, shared by
 * all query heads -- FA_MLA_DC = 512 compressed-KV elements followed by FA_MLA_DR = 64 rotary elements (they arrive rotated) -- and a
 * step attends with "absorbed" queries of width FA_MLA_DQK = 576 (q_nope . W_UK next to q_rope).  The logits run over all 576
 * elements of a row, the output is the softmax-weighted sum of its FIRST 512: V is a prefix of K and is never stored or staged apart.
 * A kernel of its own on the split-KV stream's plan (Hkv = 1, G = Hq): the Hq heads of a token are rows of one workgroup, so a latent
 * row is read from memory once and written to LDS once for both products.  DESIGN.md 7.22, profiles/mla_decode.txt.
 * Rows.     [s_b, e_b) are fa_forward_varlen's clamps of cu_seqlens_q: s_b = clamp(cu[b], 0, total_q), e_b = clamp(cu[b+1], s_b,
 *           total_q).  n_b = min(e_b - s_b, max_q); row i < n_b of sequence b is token s_b + i; a sequence that owns more than max_q
 *           tokens has its first max_q served.  L_b = clamp(seqlens_k[b], 0, capacity) (NULL: capacity), capacity = Ncap or, with
 *           block_table, max_pages * page_size.
 * Arithmetic, for every head h of token s_b + i, with C_b the latent rows of sequence b (row j of a paged sequence is row
 *           j % page_size of page block_table[b, j / page_size]):
 *             s_j = scale * sum_{e < 576} Q[s_b + i, h, e] * C_b[j, e]
 *             the row sees the keys [0, c_i): c_i = max(0, L_b - n_b + 1 + i) with causal, else L_b
 *             O[s_b + i, h, :] = sum_{j < c_i} softmax(s)_j * C_b[j, 0:512]        lse[h, s_b + i] = ln sum_{j < c_i} exp(s_j)
 *           Elements 512..575 never reach O.  Products in the 16-bit type's matrix instructions with fp32 accumulation, softmax in
 *           fp32, the weights rounded to the input type for the second product, as in every decode entry here.
 * Edges.    A row without a key (c_i = 0) returns O = 0 and lse = -inf exactly.  n_b = 0 is an idle slot: nothing of the sequence is
 *           read, its table row and cache rows included.  scale = 0 gives uniform weights and never NaN.
 * Never read or written: tokens that are no live row of any sequence (their Q rows may hold NaN; their O rows and lse entries keep
 *           what they held).  Cache rows at or past L_b are never used and may hold NaN bit patterns: they reach LDS as zeros, they
 *           are not merely masked in the score.  Table entries past a sequence's last live page are not read.  A live table entry
 *           outside [0, num_pages) reads as a page of zeros; no address is formed from it.
 * Host.     Nothing on the host reads device data.  Grid, split count and workspace follow (B, Hq, max_q, capacity, num_splits)
 *           only, so a captured call follows cu_seqlens_q, seqlens_k and the block table when they are rewritten in place.
 * Splits.   num_splits = 1 is one kernel and needs no workspace.  With S > 1 the 64-key tiles of EACH sequence's L_b keys are dealt
 *           to S partial workgroups, which write unnormalised fp32 (O, m, l) per (row, split) to the workspace, and a private merge
 *           kernel finishes; it writes no token of no sequence.  num_splits = 0 lets the library choose from (B, Hq, max_q,
 *           capacity) alone.  fa_mla_decode_workspace_bytes(desc) is the size the call needs (0 with one split, and 0 for a
 *           descriptor the call would refuse); it reads the fields named above, B, Hq, max_q, the capacity fields and num_splits.
 * Bits.     A paged and a contiguous cache holding the same keys return the same bits under the same num_splits, and a sequence's
 *           rows have the same bits whatever the other sequences of the batch hold.
 * Rejected with hipErrorInvalidValue before the device is touched: a NULL descriptor or a wrong `size`; a NULL Q, O, C or
 * cu_seqlens_q; B, total_q or max_q <= 0; Hq outside [1, 128]; in_dtype outside FA_DTYPE_F16 / FA_DTYPE_BF16, out_dtype outside
 * FA_OUT_F32 / FA_OUT_SAME; causal outside {0, 1}; contiguous: Ncap outside [1, 2^30]; paged: num_pages <= 0, max_pages <= 0, a
 * page_size that is no power of two >= 16, max_pages * page_size > 2^30; num_splits outside [0, ceil(capacity / 64)]; Q, O or C not
 * 16-byte aligned; a stride that is no multiple of 8 elements, a negative head stride, q_stride_t < 576 or o_stride_t < 512; a
 * sequence's view of Q or O -- max_q tokens over the Hq heads -- beyond 2^32 - 1 bytes; with more than one split a NULL workspace or
 * one below fa_mla_decode_workspace_bytes(desc).
 * An fp8 latent cache: fa_mla_decode_fp8 below.  Not part of this entry: a sliding window, soft-cap, sinks or a tree mask; latent widths other than 512 + 64;
 * the absorption and up-projection GEMMs (W_UK into q, W_UV out of O), which stay the caller's; a d = 512 form of
 * fa_merge_states -- the entry merges its own splits.  NOT a reference entry point. */
#define FA_MLA_DC  512   /* compressed-KV elements of a latent row: what O is made of */
#define FA_MLA_DR  64    /* rotary elements behind them: in the logits only */
#define FA_MLA_DQK 576   /* the width of a latent row and of an absorbed query */
typedef struct fa_mla_decode_desc {
    size_t size;                /* sizeof(fa_mla_decode_desc) */
    const void* Q;              /* packed (total_q, Hq, 576), d contiguous, through q_stride_t / q_stride_h (elements) */
    void* O;                    /* packed (total_q, Hq, 512) through o_stride_t / o_stride_h */
    float* lse;                 /* [Hq, total_q] fp32 natural log, may be NULL */
    const void* C;              /* latent cache [B, Ncap, 576] of in_dtype; with block_table a pool [num_pages, page_size, 576] */
    const int* cu_seqlens_q;    /* device, B+1 */
    const int* seqlens_k;       /* device, B; may be NULL (= capacity) */
    const int* block_table;     /* device, [B, max_pages]; NULL: contiguous */
    int B, Hq, total_q, max_q;
    int Ncap;                               /* contiguous only */
    int num_pages, page_size, max_pages;    /* paged only; page_size a power of two >= 16 */
    long long q_stride_t, q_stride_h, o_stride_t, o_stride_h;
    float scale;
    int causal;
    int num_splits;             /* 0: chosen by the library; else forced, 1 .. ceil(capacity/64) */
    int in_dtype, out_dtype;    /* FA_DTYPE_*; FA_OUT_F32 | FA_OUT_SAME */
    void* workspace; size_t workspace_bytes; void* stream;
} fa_mla_decode_desc;
size_t fa_mla_decode_workspace_bytes(const fa_mla_decode_desc* desc);
int    fa_mla_decode(const fa_mla_decode_desc* desc);

/* The write half of fa_mla_decode: a token-packed batch of latent rows goes into the latent cache.  Token i of sequence b -- row
 * s_b + i of Cnew, 576 elements read through new_stride_t, [s_b, e_b) the clamps of cu_seqlens_new as above, m_b = e_b - s_b -- is
 * copied bit for bit (NaN payloads included) to slot L_b + i, L_b = clamp(seqlens_k[b], 0, capacity) (NULL: 0 for all, a fresh
 * cache).  No rotary here: the 64 rotary elements arrive rotated.  A token whose slot is at or past the capacity is dropped; paged, a
 * table entry outside [0, num_pages) skips the write and no address is formed from it.  Rows of no sequence are not read.
 * seqlens_out[b] = min(L_b + m_b, capacity), by a tiny second kernel behind the copy on the same stream: seqlens_out may be NULL,
 * seqlens_k itself, or disjoint from it.  Nothing is read on the host; the grid follows total_new alone; a captured call follows
 * cu_seqlens_new, seqlens_k and the table when they are rewritten in place.
 * Rejected with hipErrorInvalidValue before the device is touched: a NULL descriptor or a wrong `size`; a NULL Cnew, C or
 * cu_seqlens_new; B or total_new <= 0; total_new above 2^24; a dtype outside FA_DTYPE_F16 / FA_DTYPE_BF16 (the copy does not look at
 * the elements, the field names the cache's type); the capacity and page geometry fa_mla_decode refuses; Cnew or C not 16-byte
 * aligned; new_stride_t < 576 or no multiple of 8; a partial overlap of seqlens_out and seqlens_k; a cu_seqlens_new that overlaps
 * seqlens_out.  NOT a reference entry point. */
typedef struct fa_mla_append_desc {
    size_t size;                /* sizeof(fa_mla_append_desc) */
    const void* Cnew;           /* packed (total_new, 576) through new_stride_t (elements) */
    void* C;                    /* the latent cache [B, Ncap, 576], or with block_table the pool [num_pages, page_size, 576] */
    const int* cu_seqlens_new;  /* device, B+1 */
    const int* seqlens_k;       /* device, B: the lengths BEFORE the append; NULL = 0 for all */
    int* seqlens_out;           /* device, B; NULL, == seqlens_k, or disjoint from it */
    const int* block_table;     /* device, [B, max_pages]; NULL: contiguous */
    int B, total_new;
    long long new_stride_t;
    int Ncap, num_pages, page_size, max_pages;   /* as in fa_mla_decode_desc */
    int dtype;                  /* FA_DTYPE_F16 or FA_DTYPE_BF16 */
    void* stream;
} fa_mla_append_desc;
int fa_mla_append(const fa_mla_append_desc* desc);

/* The fp8 latent cache of the two MLA entries.  A cache row is 576 BYTES: one OCP e4m3fn code per element, 512 compressed-KV codes
 * followed by 64 rotary codes; C is [B, Ncap, 576] or a pool [num_pages, page_size, 576] of bytes behind the same block table, 16-byte
 * aligned (576 = 36 * 16 keeps every row so).  ONE fp32 scale serves the whole cache: c_scale points to one float on the device,
 * 4-byte aligned, read on the device so that a captured call follows it; NULL is 1.0.  An element's value is decode(code) * c_scale.
 * The caller's contract is a finite c_scale > 0 (quantize_kv_fp8's); another value gives a meaningless result and never a fault.
 * The descriptors are the 16-bit entries': in_dtype (decode) names Q's type, dtype (append) names Cnew's.
 * fa_mla_decode_fp8: every rule of fa_mla_decode holds word for word -- rows, clamps, the causal mask, rows without a key, tokens of
 *   no sequence, the splits and the merge, num_splits = 0 (the SAME S as fa_mla_decode for the same descriptor; the workspace sizes are
 *   equal), a bad live page reads as zeros, paged and contiguous results are bit-equal.  The codes are widened EXACTLY to Q's type on
 *   their way into LDS (every e4m3fn value is a normal fp16 and bf16 number) and everything behind that is fa_mla_decode's arithmetic:
 *     s_j = (scale * c_scale) * sum_e Q[.., e] * code_j[e]          O = c_scale * sum_j softmax(s)_j * code_j[0:512]
 *   with lse the log-sum-exp of the s_j.  The factor is clamped after the product, so scale = 0 still gives uniform weights.  Rows at or
 *   past L_b, and pages no key lies in, may hold the NaN codes 0x7F / 0xFF: they lie outside the buffer descriptor's range and reach
 *   LDS as the code 0 (+0).  With c_scale NULL or 1.0 the result has the bits of fa_mla_decode on the widened cache.
 * fa_mla_append_fp8: fa_mla_append with the store changed -- the 8 elements of a 16-byte source chunk become 8 codes of x / c_scale:
 *   exact widening to fp32, IEEE division, clamp to +-448, round to nearest even, a NaN becomes 0x7F (the write side's quantisation,
 *   fa_kvcache_append's).  Drops, bad table entries, rows of no sequence and seqlens_out are fa_mla_append's.
 * Rejected: everything the 16-bit entries reject, and a c_scale that is not 4-byte aligned.
 * Not part of these entries: per-token scales; per-128-element scales; a 16-bit rotary tail (the 656-byte row some stacks use); an
 * fp8 Q; fp8 matrix instructions.  NOT reference entry points. */
int    fa_mla_decode_fp8(const fa_mla_decode_desc* desc, const float* c_scale);
size_t fa_mla_decode_fp8_workspace_bytes(const fa_mla_decode_desc* desc);   /* equals fa_mla_decode_workspace_bytes(desc) */
int    fa_mla_append_fp8(const fa_mla_append_desc* desc, const float* c_scale);

/* Stage-level debug entry (cf. the reference's single-stage experiments
 * FlashAttention/t16/ *debug*.cu): one stage of the tiled forward with its result in memory, through
 * the same LDS images, fragment loads and accumulator maps as the product kernels.  d in {64,128}.
 *   stage 1: A = Q, B = K [BH,N,d] 16-bit          -> Out = S = scale*Q.K^T  [BH,N,N] fp32
 *   stage 2: A = S [BH,N,N] fp32, B = NULL         -> Out = P = softmax rows of S, 16-bit [BH,N,N]
 *   stage 3: A = P [BH,N,N] 16-bit, B = V [BH,N,d] -> Out = O = P.V  [BH,N,d] fp32
 * Not a product path and not tuned. */
int fa_debug_stage(int stage, const void* A, const void* B, void* Out, int BH, int N, int d, float scale,
                   int dtype, void* stream);

/* 16x16 streaming family.  Replaces
 *   flashattn_streaming_16x16_kernel_mw(const __half* Q, const __half* K, const __half* V, float* O,
 *                                       int num_batches, int seq_len, float scale)
 *   Streaming_FlashAttention_Forward_Kernel/flashattn_streaming_16x16_mw.cu:73-81 (same list in
 *   _mw_fixed.cu:78, _mw_v2.cu:75, _mw_cpasync.cu:73, flashattn_warp_spc/..._v3..v7), launched as
 *   <<<num_batches, 64>>> (mw.cu:368-377).
 * Q [B,16,16], K [B,16,L] (k-major), V [B,L,16] fp16; O [B,16,16] fp32; O = y/(l+1e-6). */
int flashattn_streaming_16x16_mw(const void* Q, const void* K, const void* V, float* O,
                                 int num_batches, int seq_len, float scale, void* stream);

/* v8+ ABI of the same family: second pointer is K_T [B,L,16], produced by the host pre-transpose
 *   flashattn_streaming_16x16_kernel_mw_v8(const __half* Q, const __half* K_T, const __half* V, float* O,
 *                                          int num_batches, int seq_len, float scale)
 *   flashattn_warp_spc/flashattn_streaming_16x16_mw_v8.cu:103-111 (v10.cu:104, v11.cu:101). */
int flashattn_streaming_16x16_mw_kt(const void* Q, const void* K_T, const void* V, float* O,
                                    int num_batches, int seq_len, float scale, void* stream);

/* Library identification: "fa_mi355 <version> gfx950". */
const char* fa_mi355_version(void);

/* What FA_ALGO_AUTO resolves to for a shape on the CURRENT device (an FA_ALGO_* id; -1 for bad arguments), and the
 * name of the kernel template an algo id launches there (prefix of its rocprofv3 kernel-trace name; "" if unknown).
 * bench.py names its dominant kernel with these instead of hard-coding it. */
int fa_selected_algo(int B, int H, int N, int d, int in_dtype);
const char* fa_selected_kernel(int B, int H, int N, int d, int in_dtype, int algo);

/* 1 when the library was built with the experimental A/B kernels (`make experimental`: explicit algo ids
 * 7, 8, 13, 14, 16-22, 25 and the measurement entry points), 0 for the product build, where those ids return
 * hipErrorInvalidValue. */
int fa_mi355_has_experiments(void);

#ifdef __cplusplus
}
#endif
#endif
