// fa_fwd_varlen_kernel.hpp -- device code and host checks of the variable-length packed prefill, shared by fa_fwd_varlen.hip
// (fa_forward_varlen: the 16 plain instantiations) and fa_fwd_varlen_logits.hip (fa_forward_varlen_ex: the 16 kLogits ones, with a
// sliding window, a soft-cap and attention sinks).  The contract is include/fa_mi355.h's; the reasons are DESIGN.md 7.12 and 7.13.
//
// The design is the LDS-staged tiled kernel's (fa_fwd_kernel, fa_fwd_kernels.hip): S^T = K.Q^T on v_mfma_f32_32x32x16 with Q^T
// resident in registers, the packed P directly the B operand of O^T += V^T.P^T, V^T through ds_read_b64_tr_b16, the K/V tile loaded
// a tile ahead into a double-buffered LDS image (fa_tile.hpp), a lazy running max -- on 128-row workgroups (four waves of 32 rows),
// so that a short sequence wastes little.  Nothing of that kernel is used here; what is new:
//   * block -> (K/V head, slot, head of the group) with the G heads of a group, then the slots of a sequence, adjacent in the launch
//     order; slot -> (sequence, query block) on the device: sequence b owns the slots [first_b, first_{b+1}), first_b =
//     floor(s_q(b) / 128) + b, found by a binary search over cu_seqlens_q with scalar loads.  The grid is floor(total_q / 128) + B
//     slots per query head: host integers only;
//   * one buffer descriptor per (sequence, head) and tensor: base ptr + s * stride_t + h * stride_h, range (L - 1) * stride_t + d
//     elements (0 when L = 0).  A row at or past L is never addressed: its offset could wrap 32 bits, so it is selected away (a
//     partial tile's loads) or guarded (the stores), not left to the range check;
//   * the causal limit c_i = max(0, Lk - Lq + 1 + i); a row that sees no key keeps m_ref = -inf and is selected to O = 0, lse = -inf;
//   * lse = (m_ref + log2 l) ln 2, written with guarded vector stores.
// kLogits (the argument is then a VarlenLogitArgs): everything it adds sits behind `if constexpr (kLogits)`, and the plain
// instantiations keep their argument list and their code (profiles/varlen_logits.txt).  The three options are runtime and
// wave-uniform, as in the decode pack (fa_fwd_split_kernel.hpp):
//   * window W: row i also has a LOWER key limit lo_i = max(0, Lk - Lq + 1 + i - W), the same with and without the causal flag.  The
//     workgroup's tile loop starts at t0 = lo(first row) / 64 -- no row of the workgroup sees a key below that lo, so nothing below
//     tile t0 is loaded -- a wave skips the tiles wholly below the lo of ITS first row (it still stages and synchronises, as under
//     the causal skip), and only the tiles that start below the lo of the wave's last row take the per-score compare key < lo_i.
//     The masked scores are -inf; the K/V rows of such keys reach LDS as they are (a packed prompt has no freed pages).  "No
//     window" is a W that masks nothing: the host passes total_q + total_k;
//   * soft-cap: before the masks every score x = s c (log2 units) becomes cap2 tanh(x / cap2) by the decode side's formula; the
//     factor the vote and the weights then multiply a score by is 1 (`cs`).  cap2 == 0 skips it by a wave-uniform branch;
//   * sinks: one extra key per row with the head's logit and a zero V row, joined to (m, l) by sink_join() in the epilogue only.
// kCache (fa_forward_varlen_kvcache; the argument is then a VarlenCacheArgs): K/V rows come from the KV cache, and
// only that is new -- everything it adds sits behind `if constexpr (kCache ...)`, and the 32 packed instantiations keep their
// argument lists and their code (profiles/varlen_cache.txt).  Lk = clamp(seqlens_k[b], 0, Ncap) in the place of the cu_k pair:
//   * kVarlenContig: one descriptor per (b, hkv) of Lk rows of d elements; the loads are the packed ones;
//   * kVarlenPaged: the decode side's scheme (fa_fwd_split_kernel.hpp) on this kernel's staging.  With idx = tid + p * 256 the loads
//     one wave issues for one p cover 8 consecutive rows at d = 64 and 4 at d = 128, aligned to as many, so they lie inside ONE page
//     of >= 16 keys: the page number is wave-uniform, held in a scalar register per (wave, p), and goes into a descriptor that ends
//     at the page's last row below Lk (rows past it read 0, as the packed kernel's last tile selects them).  The table entries of
//     tile t + 1 are fetched while tile t - 1 computes; the entry index is clamped to [page of lo(first row), page of Lk - 1];
//   * with a window the rows of tile t0 below the lo of the workgroup's first row reach LDS as zeros, and a page wholly below that
//     lo gets a descriptor of no records: a freed page may hold NaN, and 0 * NaN in the PV MFMA is NaN.
// Tiles stay at absolute multiples of 64 from key 0, so on finite keys the cache kernels return the packed kernels' bits.
// kFp8 (fa_forward_varlen_kvcache_fp8; kCache with a VarlenCacheFp8Args): a K/V row is D e4m3fn bytes, and only that
// is new -- everything it adds sits behind `if constexpr (kFp8)` or a constant that is the 16-bit one without it, and the 96 other
// instantiations keep their code (profiles/varlen_cache_fp8.txt).  The decode side's scheme (fa_fwd_split_kernel.hpp): one 16-byte
// load carries the two adjacent LDS chunks 2c and 2c + 1 of a row, so a thread issues half the loads per tile, keeps the raw bytes
// across the tile's arithmetic and widens them (exactly) in stage_write(): the LDS image, and everything that reads it, is the 16-bit
// kernels'.  One wave's loads for one p cover 16 rows at d = 64 and 8 at d = 128, aligned to as many -- still inside one page of
// >= 16 keys.  The rows past Lk and the rows below lo_wg are zeroed as RAW bytes (code 0 is +0.0): a freed page may hold the NaN
// codes 0x7F / 0xFF.  k_scale[hkv] joins the logit factor, with the FLT_MIN clamp on the product; v_scale[hkv] joins 1 / l.
// kRouted (fa_kvcache_attend_varlen's LONG half; kCache, causal, with a VarlenRoutedArgs around the arguments): right
// after Lq is known a workgroup whose sequence has Lq <= min_rows returns -- such a sequence is the split-KV stream's.  The test is
// scalar and dead before the Q load; every other workgroup runs the unrouted kernel's code and returns its bits.
#pragma once
#include "../../include/fa_mi355.h"
#include "fa_tile.hpp"
#include "fa_dispatch.hpp"
#include "fa_fwd_split_kernel.hpp"   // to_sgpr(), sink_join()

#include <math.h>
#include <type_traits>

namespace fa {

constexpr int kVarlenWaves = 4;                    // 32 query rows each
constexpr int kVarlenRows = 32 * kVarlenWaves;     // BM: query rows per workgroup = rows per slot
constexpr float kVarlenLn2 = 0.6931471805599453f;

struct VarlenArgs {
    const uint16_t *Q, *K, *V;
    void* O;
    float* lse;
    const int *cu_q, *cu_k;
    int B, Hkv, G, total_q, total_k;
    unsigned nslots;                                // floor(total_q / BM) + B
    long long q_st, q_sh, k_st, k_sh, v_st, v_sh, o_st, o_sh;   // elements
    float scale_log2e;
};

// What the kLogits instantiations take: the plain arguments plus the three options.  The cap comes in log2 units, as in LogitArgs.
struct VarlenLogitArgs : VarlenArgs {
    const float* sinks;   // [Hkv * G] natural-log logits on the device, or nullptr: none
    int window;           // 1 <= W <= total_q + total_k (the host's clamp; at the upper end it masks nothing)
    float cap2;           // softcap * log2(e); 0: no cap
    float cap_rk;         // 2 / softcap
};

// Where the K/V rows come from (the kernel's kCache)
constexpr int kVarlenPacked = 0;   // token-packed tensors cut by cu_k
constexpr int kVarlenContig = 1;   // a cache [B, Hkv, Ncap, D]
constexpr int kVarlenPaged = 2;    // page pools [num_pages, Hkv, page, D] behind a block table

// What the cache instantiations take, plain and kLogits alike (the plain ones leave the three options unread).  K, V: the cache or
// the pools; cu_k is null; total_k is the capacity Ncap; k_st = v_st = D and k_sh = v_sh = Ncap * D (the contiguous descriptor's).
struct VarlenCacheArgs : VarlenLogitArgs {
    const int* seqlens_k;   // [B] keys of sequence b in the cache, on the device
    const int* table;       // [B][max_pages] page numbers on the device; null: contiguous
    int max_pages;          // row pitch of the table; Ncap = max_pages << lg_page
    int num_pages;          // pages in the pool: a live entry outside [0, num_pages) reads as a page of zeros
    int lg_page;            // log2 of the page size in keys (>= 4)
};

// What the fp8 cache instantiations take: K, V point at one e4m3fn byte per element (the strides stay in elements)
struct VarlenCacheFp8Args : VarlenCacheArgs {
    const float *k_scale, *v_scale;   // [Hkv] on the device, or nullptr (1.0)
};

// What the routed cache instantiations take (kRouted: the LONG half of fa_kvcache_attend_varlen): the cache arguments as they are plus
// the threshold, in a derived structure so that VarlenCacheArgs, and with it the argument layout of every other kernel, stays as it is
template <typename Base> struct VarlenRoutedArgs : Base {
    int min_rows;   // a sequence with Lq <= min_rows is the split-KV stream's: its workgroups return
};
// the argument structure of an instantiation
template <bool kLogits, int kCache, bool kFp8, bool kRouted> struct VarlenKernelArgs {
    using plain = std::conditional_t<kFp8, VarlenCacheFp8Args, std::conditional_t<kCache != 0, VarlenCacheArgs,
                                     std::conditional_t<kLogits, VarlenLogitArgs, VarlenArgs>>>;
    using type = std::conditional_t<kRouted, VarlenRoutedArgs<plain>, plain>;
};

// `elems` K/V elements past p.  With kFp8 p points at one byte per element; it keeps the type the argument structs give K and V, and
// is only ever the base of a buffer descriptor.  (Without kFp8 this must stay `p + elems`: written as byte arithmetic for both, the
// 16-bit cache kernels compile to another order of their scalar multiplies.)
template <bool kFp8> __device__ __forceinline__ const uint16_t* varlen_kv_at(const uint16_t* p, size_t elems)
{
    if constexpr (kFp8) return reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(p) + elems);
    else return p + elems;
}

// [s, e) of sequence b in a tensor of `total` rows: never outside it, never negative in length
__device__ __forceinline__ void varlen_bounds(const int* __restrict__ cu, unsigned b, int total, int& s, int& e)
{
    s = min(max(cu[b], 0), total);
    e = min(max(cu[b + 1], s), total);
}

// the (sequence, head) view of a packed tensor: rows [0, L) of stride_t elements, d contiguous; es = bytes per element
__device__ __forceinline__ __amdgpu_buffer_rsrc_t varlen_rsrc(const void* ptr, int s, int L, unsigned h, long long st, long long sh,
                                                              int d, unsigned es)
{
    const long long first = (long long)s * st + (long long)h * sh;
    const unsigned bytes = L > 0 ? (unsigned)((unsigned long long)((long long)(L - 1) * st + d) * es) : 0u;
    return make_rsrc(static_cast<const char*>(ptr) + first * (long long)es, bytes);
}

template <typename T, int D, bool kOutF32, bool kCausal, bool kLogits = false, int kCache = kVarlenPacked, bool kFp8 = false,
          bool kRouted = false>
__global__ __launch_bounds__(64 * kVarlenWaves, 2)
void fa_fwd_varlen_kernel(typename VarlenKernelArgs<kLogits, kCache, kFp8, kRouted>::type a)
{
    static_assert(!kFp8 || kCache != kVarlenPacked, "an fp8 K/V is a cache's");
    static_assert(!kRouted || (kCache != kVarlenPacked && kCausal), "the routed forms are causal cache kernels");
    using G = TileGeom<D>;
    constexpr unsigned kKvEs = kFp8 ? 1u : 2u;                          // bytes per K/V element
    constexpr int kLdChunks = kFp8 ? G::kChunks / 2 : G::kChunks;      // 16-byte loads per K/V row
    constexpr int W = kVarlenWaves;
    constexpr unsigned BM = kVarlenRows;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // ---- block -> (K/V head, slot, head of the group): blocks that share K/V sit on one XCD, consecutively ----
    const unsigned nwg = gridDim.x, bid = blockIdx.x;
    const unsigned xq = nwg >> 3, xr = nwg & 7u, xcd = bid & 7u;
    const unsigned wgid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    const unsigned grp = wgid / (unsigned)a.G, g = wgid - grp * (unsigned)a.G;
    const unsigned hkv = grp / a.nslots, sidx = grp - hkv * a.nslots;
    const unsigned slot = kCausal ? a.nslots - 1u - sidx : sidx;   // under the mask the last blocks of a sequence are the long ones
    const unsigned hq = hkv * (unsigned)a.G + g;

    // ---- slot -> (sequence, query block): the largest b with first_b <= slot (wave-uniform: scalar loads) ----
    const int* __restrict__ cu_q = a.cu_q;
    const int* __restrict__ cu_k = a.cu_k;
    unsigned lo = 0, hi = (unsigned)a.B;
    while (hi - lo > 1u) {
        const unsigned mid = (lo + hi) >> 1;
        const unsigned first = (unsigned)min(max(cu_q[mid], 0), a.total_q) / BM + mid;
        if (first <= slot) lo = mid; else hi = mid;
    }
    const unsigned b = lo;
    int sq, eq, sk, ek;
    varlen_bounds(cu_q, b, a.total_q, sq, eq);
    if constexpr (kCache != kVarlenPacked) {   // the keys of sequence b are the cache rows [0, Lk)
        sk = 0;
        ek = min(max(a.seqlens_k[b], 0), a.total_k);
    } else {
        varlen_bounds(cu_k, b, a.total_k, sk, ek);
    }
    const int Lq = eq - sq, Lk = ek - sk;
    // kRouted: a sequence of at most min_rows rows belongs to the other launch; wave-uniform, before anything of it is read
    if constexpr (kRouted) {
        if (Lq <= a.min_rows) return;
    }
    const unsigned first_b = (unsigned)sq / BM + b;
    if (slot < first_b) return;                        // slots below the first sequence's
    const unsigned qb = slot - first_b;
    if ((unsigned long long)qb * BM >= (unsigned long long)Lq) return;   // a spare slot of the sequence

    const unsigned tid  = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u;
    const unsigned r = lane & 31u, h = lane >> 5;

    const __amdgpu_buffer_rsrc_t rq = varlen_rsrc(a.Q, sq, Lq, hq, a.q_st, a.q_sh, D, 2u);
    // kCache: sequence b's part of the cache starts b * Hkv * Ncap rows in (64 bit); a.k_sh = Ncap * D then selects the head.  Paged:
    // these two are not used, every (wave, p) makes its own
    const size_t kv_b = kCache == kVarlenContig ? (size_t)b * (size_t)a.Hkv * (size_t)a.k_sh : 0;
    const __amdgpu_buffer_rsrc_t rk = varlen_rsrc(varlen_kv_at<kFp8>(a.K, kv_b), sk, Lk, hkv, a.k_st, a.k_sh, D, kKvEs);
    const __amdgpu_buffer_rsrc_t rv = varlen_rsrc(varlen_kv_at<kFp8>(a.V, kv_b), sk, Lk, hkv, a.v_st, a.v_sh, D, kKvEs);
    // byte strides of a token row; every offset of an existing row fits 32 bits (checked on the host)
    const unsigned q_stb = (unsigned)a.q_st * 2u;
    const unsigned k_stb = kCache != kVarlenPacked ? D * kKvEs : (unsigned)a.k_st * 2u;
    const unsigned v_stb = kCache != kVarlenPacked ? D * kKvEs : (unsigned)a.v_st * 2u;

    constexpr int kLoadsW = (kBlockN * kLdChunks) / (64 * W);
    const unsigned wave_row0 = qb * BM + wave * 32u;   // first query row of this wave, in the sequence
    const unsigned q_row = wave_row0 + r;
    const bool row_live = q_row < (unsigned)Lq;
    const int shift = Lk - Lq;                         // causal: row i sees the keys j <= i + shift

    // ---- Q^T fragments (B operand of S^T = K.Q^T), resident for the whole kernel ---------------
    // c = |scale|*log2(e) is applied to the fp32 scores; a negative scale flips Q's sign bits so that the row max of c*S is
    // always c*max(S).  Rows at or past Lq are zeros.
    // kFp8: the head's k_scale is part of the factor, and the clamp applies to the product (the host's clamp of scale_log2e alone does
    // not survive a k_scale below 1: +-FLT_MIN * 0.5 must not meet a masked -inf as 0).  The product is vector arithmetic, so it goes
    // back into a scalar register; v_scale is used at the end
    float c = fabsf(a.scale_log2e);
    [[maybe_unused]] float v_scale = 1.0f;
    if constexpr (kFp8) {
        const float k_scale = a.k_scale ? a.k_scale[hkv] : 1.0f;
        if (a.v_scale) v_scale = a.v_scale[hkv];
        c = to_sgpr(fmaxf(fabsf(a.scale_log2e * k_scale), 1.17549435e-38f));
    }
    const unsigned q_flip = a.scale_log2e < 0.0f ? 0x80008000u : 0u;
    // kLogits: what a score is multiplied by on its way into the vote and the exponent (c, or 1 once the soft-cap has made the scores
    // final) and the cap's two constants, in scalar registers: computed from kernel arguments they would live in VGPRs through the
    // tile loop (gfx950 has no scalar float arithmetic).  c itself is dead after this point
    [[maybe_unused]] float cs = c, cap_k1 = 0.0f, cap_n2 = 0.0f;
    // kLogits: the lower key limits of the workgroup's first row (tile t0 holds it), of this wave's first row (the wave's smallest)
    // and of its last row (its largest); |shift + 1 + row| <= 2^26 and window <= 2^27 by the host's checks, so nothing wraps
    [[maybe_unused]] int t0 = 0, lo_first = 0, lo_last = 0;
    // kCache: the lo of the workgroup's first row itself (0 without a window): no K/V row and no page below it is used
    [[maybe_unused]] unsigned lo_wg = 0;
    if constexpr (kLogits) {
        cs = to_sgpr(a.cap2 > 0.0f ? 1.0f : c);
        cap_k1 = to_sgpr(c * a.cap_rk);
        cap_n2 = to_sgpr(-2.0f * a.cap2);
        t0 = max(0, shift + 1 + (int)(qb * BM) - a.window) / kBlockN;
        if constexpr (kCache != kVarlenPacked) lo_wg = (unsigned)max(0, shift + 1 + (int)(qb * BM) - a.window);
        lo_first = max(0, shift + 1 + (int)wave_row0 - a.window);
        lo_last = max(0, shift + 1 + (int)wave_row0 + 31 - a.window);
    }
    u32x4 qf[G::kKSteps];
#pragma unroll
    for (int s = 0; s < G::kKSteps; ++s) {
        u32x4 raw = buf_load16(rq, (row_live ? q_row * q_stb : 0u) + (16u * s + 8u * h) * 2u);
#pragma unroll
        for (int w = 0; w < 4; ++w) raw[w] = row_live ? raw[w] ^ q_flip : 0u;
        qf[s] = raw;
    }

    // ---- staging: each thread moves kLoadsW 16-B chunks of K and of V per tile -----------------
    unsigned s_row[kLoadsW], s_col[kLoadsW], k_lds[kLoadsW], v_lds[kLoadsW];
#pragma unroll
    for (int p = 0; p < kLoadsW; ++p) {
        const unsigned idx = tid + p * 64u * W;
        const unsigned row = idx / kLdChunks, ch = idx % kLdChunks;
        s_row[p] = row;
        s_col[p] = ch * 16u;
        // kFp8: the load holds the LDS chunks 2 ch and 2 ch + 1; the second one's offset is the first's with bit 4 flipped, in the K
        // image (the swizzle XORs the chunk index) and in the V image (chunk & 3 is even)
        k_lds[p] = G::k_off(row, kFp8 ? 2u * ch : ch);
        v_lds[p] = G::kTileBytes + G::v_off(row, kFp8 ? 2u * ch : ch);
    }
    u32x4 kst[kLoadsW], vst[kLoadsW];
    // kVarlenPaged: the page numbers of the tile that is staged next, one per (wave, p), in scalar registers.  fetch_pages() reads them
    // for a tile (only called with Lk >= 1); the entry index is clamped to the sequence's last live page, so no entry at or past
    // ceil(Lk / page) is read -- which also makes a tile index past the last tile harmless.  `first_tile` (tile t0, in the prologue)
    // under a window: the index is clamped to lo_wg's page too (lo_wg < Lk), so no entry of a page wholly below the window is read,
    // and such a page gets a descriptor of no records; every later tile starts above lo_wg, so the loop does not carry lo_wg.
    // A (wave, p) whose rows all lie at or past Lk gets a descriptor of no records whatever the number says.
    [[maybe_unused]] int pg[kLoadsW];
    // the pools at this K/V head's block of page 0, and the pool's elements per page
    [[maybe_unused]] const uint16_t *k_pool = a.K, *v_pool = a.V;
    if constexpr (kCache == kVarlenPaged) {
        k_pool = varlen_kv_at<kFp8>(k_pool, ((size_t)hkv << a.lg_page) * D);
        v_pool = varlen_kv_at<kFp8>(v_pool, ((size_t)hkv << a.lg_page) * D);
    }
    [[maybe_unused]] auto fetch_pages = [&](unsigned kv0, [[maybe_unused]] auto first_tile) {
        if constexpr (kCache == kVarlenPaged) {
            const int* __restrict__ tbl = a.table + (size_t)b * (unsigned)a.max_pages;
            const unsigned last = ((unsigned)Lk - 1u) >> a.lg_page;
#pragma unroll
            for (int p = 0; p < kLoadsW; ++p) {
                const unsigned wrow = (wave * 64u + p * 64u * W) / kLdChunks;   // first row of the tile this wave loads with p
                unsigned e = min((kv0 + wrow) >> a.lg_page, last);
                if constexpr (kLogits && decltype(first_tile)::value) e = max(e, lo_wg >> a.lg_page);
                pg[p] = __builtin_amdgcn_readfirstlane(tbl[e]);
            }
        }
    };
    [[maybe_unused]] auto stage_load_paged = [&](unsigned kv0, [[maybe_unused]] auto first_tile) {
        if constexpr (kCache == kVarlenPaged) {
            const unsigned page = 1u << a.lg_page;
#pragma unroll
            for (int p = 0; p < kLoadsW; ++p) {
                const unsigned wrow = (wave * 64u + p * 64u * W) / kLdChunks;
                const unsigned first = (kv0 + wrow) & ~(page - 1u);            // first key of the page
                bool ok = (unsigned)pg[p] < (unsigned)a.num_pages && first < (unsigned)Lk;
                // a page wholly below the window: pg[p] is another page's
                if constexpr (kLogits && decltype(first_tile)::value) ok = ok && first + page > lo_wg;
                // the page's rows below Lk; a bad page number or a page outside the live range: no record, every load reads 0
                const unsigned bytes = ok ? min(page, (unsigned)Lk - first) * (D * kKvEs) : 0u;
                // 64-bit: pools beyond 4 GiB are normal; only the offset inside one page-head block is 32 bit
                const size_t blk = (((size_t)(ok ? pg[p] : 0) * (unsigned)a.Hkv) << a.lg_page) * D;
                const __amdgpu_buffer_rsrc_t pk = make_rsrc(varlen_kv_at<kFp8>(k_pool, blk), bytes),
                                             pv = make_rsrc(varlen_kv_at<kFp8>(v_pool, blk), bytes);
                // reduced to the page: a product that wraps 32 bits keeps its low bits
                const unsigned off = ((kv0 + s_row[p]) * (D * kKvEs) + s_col[p]) & (page * (D * kKvEs) - 1u);
                kst[p] = buf_load16(pk, off);
                vst[p] = buf_load16(pv, off);
            }
        }
    };
    auto stage_load = [&](unsigned kv0) {
        if (kv0 + (unsigned)kBlockN <= (unsigned)Lk) {          // a whole tile (wave-uniform)
#pragma unroll
            for (int p = 0; p < kLoadsW; ++p) {
                kst[p] = buf_load16(rk, (kv0 + s_row[p]) * k_stb + s_col[p]);
                vst[p] = buf_load16(rv, (kv0 + s_row[p]) * v_stb + s_col[p]);
            }
        } else {                                                // the last one: rows at or past Lk are zeros
#pragma unroll
            for (int p = 0; p < kLoadsW; ++p) {
                const unsigned key = kv0 + s_row[p];
                const bool ok = key < (unsigned)Lk;
                const u32x4 kk = buf_load16(rk, (ok ? key * k_stb : 0u) + s_col[p]);
                const u32x4 vv = buf_load16(rv, (ok ? key * v_stb : 0u) + s_col[p]);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    kst[p][w] = ok ? kk[w] : 0u;
                    vst[p][w] = ok ? vv[w] : 0u;
                }
            }
        }
    };
    // kCache with a window: the rows of the first streamed tile below lo_wg go to LDS as zeros (workgroup-uniform test, tile t0 only)
    [[maybe_unused]] auto stage_zero_below = [&](unsigned kv0) {
        if (kv0 < lo_wg) {
#pragma unroll
            for (int p = 0; p < kLoadsW; ++p)
                if (kv0 + s_row[p] < lo_wg) kst[p] = vst[p] = u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto stage_write = [&](unsigned buf) {
#pragma unroll
        for (int p = 0; p < kLoadsW; ++p) {
            if constexpr (kFp8) {   // the raw bytes become the two chunks of T (fp8x16_widen, exact)
                u32x4 lo, hi;
                fp8x16_widen<T>(kst[p], lo, hi);
                lds_write16(smem, buf * G::kBufBytes + k_lds[p], lo);
                lds_write16(smem, buf * G::kBufBytes + (k_lds[p] ^ 16u), hi);
                fp8x16_widen<T>(vst[p], lo, hi);
                lds_write16(smem, buf * G::kBufBytes + v_lds[p], lo);
                lds_write16(smem, buf * G::kBufBytes + (v_lds[p] ^ 16u), hi);
                continue;
            }
            lds_write16(smem, buf * G::kBufBytes + k_lds[p], kst[p]);
            lds_write16(smem, buf * G::kBufBytes + v_lds[p], vst[p]);
        }
    };

    // ---- per-lane LDS read addresses (fa_tile.hpp's images) ------------------------------------
    const unsigned k_rd_row = r * G::kRowBytes;
    const unsigned k_rd_swz = G::k_swz(r);
    const unsigned i16 = lane & 15u, vq = i16 >> 2, vp = i16 & 3u, vg = (lane >> 4) & 1u;
    unsigned v_rd[2];   // per parity of the column block (row-slot rotation)
#pragma unroll
    for (int par = 0; par < 2; ++par)
        v_rd[par] = G::kTileBytes + h * G::kDBlocks * 256u + ((vq ^ par) << 6) + vg * 32u + vp * 8u;

    // ---- running state -------------------------------------------------------------------------
    f32x16 o[G::kDBlocks];
#pragma unroll
    for (int db = 0; db < G::kDBlocks; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[db][i] = 0.0f;
    f32x16 zero16;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero16[i] = 0.0f;
    float m_ref = -INFINITY;   // reference max of this lane's query row, in log2 units (c*S); -inf: no key seen yet
    float l_part = 0.0f;       // this half-wave's share of the row sum

    // tiles up to the key limit of the workgroup's last existing row
    int klim = Lk;
    if constexpr (kCausal) {
        const int last_row = (int)min((unsigned)Lq - 1u, qb * BM + BM - 1u);
        klim = max(0, shift + 1 + last_row);           // <= Lk
    }
    const int ntiles = (klim + kBlockN - 1) / kBlockN;

    // kLogits: the loop starts at tile t0 (t0 < ntiles whenever ntiles > 0: lo < c for a row with c >= 1), in buffer t0 & 1
    if (kLogits ? t0 < ntiles : ntiles > 0) {
        if constexpr (kCache == kVarlenPaged) fetch_pages(kLogits ? t0 * kBlockN : 0, std::true_type{});
        if constexpr (kCache == kVarlenPaged) stage_load_paged(kLogits ? t0 * kBlockN : 0, std::true_type{});
        else stage_load(kLogits ? t0 * kBlockN : 0);
        if constexpr (kCache == kVarlenPaged) fetch_pages(((kLogits ? t0 : 0) + 1) * kBlockN, std::false_type{});
        if constexpr (kCache != kVarlenPacked && kLogits) stage_zero_below(t0 * kBlockN);
        stage_write(kLogits ? t0 & 1u : 0);
    }
    __syncthreads();

    for (int t = kLogits ? t0 : 0; t < ntiles; ++t) {
        const unsigned cur = t & 1u;
        const char* kbuf = smem + cur * G::kBufBytes;
        if constexpr (kCache == kVarlenPaged) {
            if (t + 1 < ntiles) stage_load_paged((t + 1) * kBlockN, std::false_type{});
        } else {
            if (t + 1 < ntiles) stage_load((t + 1) * kBlockN);
        }
        // kVarlenPaged: the table read of the tile after next (clamped to the last live page) overlaps this tile's arithmetic
        if constexpr (kCache == kVarlenPaged) fetch_pages((t + 2) * kBlockN, std::false_type{});
        // causal: tiles wholly past the limits of this wave's rows contribute nothing (wave-uniform)
        // kLogits: nor do tiles wholly below the lower limit of the wave's first row
        if ((!kCausal || t * kBlockN <= shift + (int)wave_row0 + 31) && (!kLogits || t * kBlockN + kBlockN > lo_first)) {

        // ---- S^T = K.Q^T (raw fp32 scores) ------------------------------------------------
        f32x16 s[2];
#pragma unroll
        for (int ks = 0; ks < G::kKSteps; ++ks) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const u32x4 kf = lds_read16(kbuf, kb * 32u * G::kRowBytes + k_rd_row +
                                                      (((2u * ks + h) ^ k_rd_swz) << 4));
                s[kb] = T::mfma32(kf, qf[ks], ks == 0 ? zero16 : s[kb]);
            }
        }

        // ---- soft-cap (wave-uniform), before the masks so that a masked key stays at -inf: the scores are final after it ----
        if constexpr (kLogits) {
            if (a.cap2 > 0.0f) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        s[kb][i] = __builtin_fmaf(cap_n2, __builtin_amdgcn_rcpf(1.0f + fast_exp2(s[kb][i] * cap_k1)), a.cap2);
            }
        }

        // ---- keys >= Lk (last tile only): -inf so that p = 0 --------------------------------
        if ((t + 1) * kBlockN > Lk) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = t * kBlockN + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * (int)h;
                    if (key >= Lk) s[kb][i] = -INFINITY;
                }
        }
        if constexpr (kCausal) {   // tiles a limit of this wave crosses: keys past the row's limit -> -inf
            if (t * kBlockN + kBlockN - 1 > shift + (int)wave_row0) {
                const int lim = shift + (int)q_row;   // the last key the row sees; negative: none
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = t * kBlockN + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * (int)h;
                        if (key > lim) s[kb][i] = -INFINITY;
                    }
            }
        }
        if constexpr (kLogits) {   // tiles a lower limit of this wave crosses: keys below the row's limit -> -inf
            if (t * kBlockN < lo_last) {
                const int lo_row = shift + 1 + (int)q_row - a.window;   // negative: the row sees from key 0
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = t * kBlockN + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * (int)h;
                        if (key < lo_row) s[kb][i] = -INFINITY;
                    }
            }
        }

        // ---- tile max vs the reference max; raise the reference only when needed ----------------
        float tmax = max3(s[0][0], s[0][1], s[0][2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) tmax = max3(tmax, s[0][i], s[0][i + 1]);
        tmax = max3(tmax, s[0][15], s[1][0]);
#pragma unroll
        for (int i = 1; i < 15; i += 2) tmax = max3(tmax, s[1][i], s[1][i + 1]);
        tmax = fmaxf(tmax, s[1][15]) * (kLogits ? cs : c);   // log2 units; -inf: the row sees no key of this tile

        // a row that has seen no key has m_ref = -inf: a first key raises it (inf > kThr), none leaves it (NaN > kThr is false)
        if (__any(tmax - m_ref > kThr)) {
            const float mx = fmaxf(tmax, swap_halves(tmax));         // row max, same in both halves
            const float m_new = fmaxf(mx, m_ref);
            const float alpha = m_ref == -INFINITY ? 0.0f : fast_exp2(m_ref - m_new);   // never 2^(-inf - -inf)
            m_ref = m_new;
#pragma unroll
            for (int db = 0; db < G::kDBlocks; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
            l_part *= alpha;
        }

        // ---- p = 2^(c*S - m_ref), row-sum share, pack to 16 bit (B operand of PV) -----------
        u32x4 pk[4];
        float lsum0 = 0.0f, lsum1 = 0.0f;
        const float neg_m = m_ref == -INFINITY ? 0.0f : -m_ref;   // every score of such a row is -inf: p = 2^-inf = 0
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][i] = fast_exp2(__builtin_fmaf(s[kb][i], kLogits ? cs : c, neg_m));
            if constexpr (!T::kSumRounded) {
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                    lsum0 += s[kb][i];
                    lsum1 += s[kb][i + 1];
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    pk[kb * 2 + s2][w] = T::pack2(s[kb][8 * s2 + 2 * w], s[kb][8 * s2 + 2 * w + 1]);
                    if constexpr (T::kSumRounded) {
                        if (w & 1) lsum1 = T::sum2(pk[kb * 2 + s2][w], lsum1);
                        else lsum0 = T::sum2(pk[kb * 2 + s2][w], lsum0);
                    }
                }
        }
        l_part += lsum0 + lsum1;

        // ---- O^T += V^T.P^T -------------------------------------------------------------------
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int db = 0; db < G::kDBlocks; ++db) {
                u32x4 vf;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const u32x2 half = lds_read_tr8(
                        kbuf, v_rd[db & 1] + ((4u * ks + 2u * jj) * G::kDBlocks + db) * 256u);
                    vf[2 * jj] = half[0];
                    vf[2 * jj + 1] = half[1];
                }
                o[db] = T::mfma32(vf, pk[ks], o[db]);
            }
        }
        }   // wave has work in this tile

        if (t + 1 < ntiles) stage_write(cur ^ 1u);
        __syncthreads();
    }

    // ---- normalise and store: lane holds O[q_row][db*32 + 8g + 4h + 0..3] in o[db][4g..4g+3] ---
    if (!row_live) return;                             // rows at or past Lq are the next sequence's, or nobody's
    float l = l_part + swap_halves(l_part);
    const bool none = m_ref == -INFINITY;              // the row saw no key: O = 0 and lse = -inf, never 0/0
    // kLogits: the sink joins here, once per row (hq is wave-uniform: a scalar load).  `nolse` then keys on the joined maximum -- a row
    // without a key has lse = the sink logit -- while O of such a row stays selected to 0 by `none`, the keys' own test.  A head
    // without a sink (-inf) keeps (m, l) bit for bit and takes the factor 1
    [[maybe_unused]] float w_keys = 1.0f;
    [[maybe_unused]] bool nolse = none;
    if constexpr (kLogits) {
        if (a.sinks) {
            w_keys = sink_join(a.sinks[hq] * kLog2e, m_ref, l);
            nolse = m_ref == -INFINITY;
        }
    }
    float inv = none ? 0.0f : 1.0f / l;
    if constexpr (kLogits) inv *= w_keys;
    if constexpr (kFp8) inv *= v_scale;
    if (a.lse && h == 0)
        a.lse[(size_t)hq * (size_t)a.total_q + (size_t)sq + q_row] =
            (kLogits ? nolse : none) ? -INFINITY : (m_ref + __log2f(l)) * kVarlenLn2;
    constexpr unsigned es = kOutF32 ? 4u : 2u;
    const __amdgpu_buffer_rsrc_t ro = varlen_rsrc(a.O, sq, Lq, hq, a.o_st, a.o_sh, D, es);
    const unsigned o_row = q_row * ((unsigned)a.o_st * es);
#pragma unroll
    for (int db = 0; db < G::kDBlocks; ++db) {
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const unsigned col = db * 32u + 8u * gg + 4u * h;
            const float x0 = none ? 0.0f : o[db][4 * gg] * inv, x1 = none ? 0.0f : o[db][4 * gg + 1] * inv;
            const float x2 = none ? 0.0f : o[db][4 * gg + 2] * inv, x3 = none ? 0.0f : o[db][4 * gg + 3] * inv;
            if constexpr (kOutF32) {
                const f32x4 v = {x0, x1, x2, x3};
                buf_store16(ro, o_row + col * 4u, __builtin_bit_cast(u32x4, v));
            } else {
                const u32x2 v = {T::pack2(x0, x1), T::pack2(x2, x3)};
                buf_store8(ro, o_row + col * 2u, v);
            }
        }
    }
}

// ---- host side: the checks, shared by the two entries ---------------------------------------------------------------------------

// the last addressable byte of a packed tensor, ((total-1)*stride_t + (H-1)*stride_h + d) * es, must fit 32 bits
static inline bool varlen_tensor_ok(const void* p, int total, int H, int d, long long st, long long sh, unsigned es)
{
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15u)) return false;
    if (st < d || sh < 0 || st % 8 != 0 || sh % 8 != 0) return false;
    const unsigned __int128 end = ((unsigned __int128)(total - 1) * (unsigned long long)st +
                                   (unsigned __int128)(H - 1) * (unsigned long long)sh + (unsigned)d) * es;
    return end <= 0xFFFFFFFFull;
}

// fa_forward_varlen's checks; on success the kernel arguments and the grid (host integers only)
static inline hipError_t varlen_check(const fa_varlen_desc* d, VarlenArgs& a, dim3& grid)
{
    if (!d || d->size != sizeof(fa_varlen_desc)) return hipErrorInvalidValue;
    if (!d->cu_seqlens_q || !d->cu_seqlens_k) return hipErrorInvalidValue;
    if (d->B <= 0 || d->Hkv <= 0 || d->G <= 0 || d->total_q <= 0 || d->total_k <= 0) return hipErrorInvalidValue;
    if (d->d != 64 && d->d != 128) return hipErrorInvalidValue;
    if (d->in_dtype != FA_DTYPE_F16 && d->in_dtype != FA_DTYPE_BF16) return hipErrorInvalidValue;
    if (d->out_dtype != FA_OUT_F32 && d->out_dtype != FA_OUT_SAME) return hipErrorInvalidValue;
    const long long Hq = (long long)d->Hkv * d->G;                                          // < 2^62
    if (Hq > 0x7FFFFFFFll || (unsigned __int128)Hq * (unsigned)d->B > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned es = d->out_dtype == FA_OUT_F32 ? 4u : 2u;
    if (!varlen_tensor_ok(d->Q, d->total_q, (int)Hq, d->d, d->q_stride_t, d->q_stride_h, 2u) ||
        !varlen_tensor_ok(d->K, d->total_k, d->Hkv, d->d, d->k_stride_t, d->k_stride_h, 2u) ||
        !varlen_tensor_ok(d->V, d->total_k, d->Hkv, d->d, d->v_stride_t, d->v_stride_h, 2u) ||
        !varlen_tensor_ok(d->O, d->total_q, (int)Hq, d->d, d->o_stride_t, d->o_stride_h, es))
        return hipErrorInvalidValue;
    // block slots: floor(total_q / BM) + B per query head, whatever the vectors hold
    const long long nslots = (long long)d->total_q / kVarlenRows + d->B;
    if (nslots * Hq > 0x7FFFFFFFll) return hipErrorInvalidValue;
    a = {static_cast<const uint16_t*>(d->Q), static_cast<const uint16_t*>(d->K), static_cast<const uint16_t*>(d->V),
         d->O, d->lse, d->cu_seqlens_q, d->cu_seqlens_k, d->B, d->Hkv, d->G, d->total_q, d->total_k, (unsigned)nslots,
         d->q_stride_t, d->q_stride_h, d->k_stride_t, d->k_stride_h, d->v_stride_t, d->v_stride_h, d->o_stride_t,
         d->o_stride_h, host_scale_log2e(d->scale)};
    grid = dim3((unsigned)(nslots * Hq));
    return hipSuccess;
}

// fa_forward_varlen_kvcache's checks (fa_fwd_varlen_cache.hip), which the fp8 entry runs too; on success the kernel arguments (the
// three options included) and the grid (host integers only)
hipError_t varlen_cache_check(const fa_varlen_kvcache_desc* d, VarlenCacheArgs& a, dim3& grid);

// the one launch: the instantiation of (types, d, causal) with the entry's kLogits and argument structure
template <bool kLogits, typename Args>
static inline hipError_t varlen_launch(const fa_varlen_desc* d, const Args& a, dim3 grid)
{
    const bool causal = d->causal != 0;
    return with_types(d->in_dtype, d->out_dtype, [&](auto t, auto f32) {
        using T = decltype(t);
        auto launch = [&](auto kernel, int lds) {
            const hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), lds);
            if (attr != hipSuccess) return attr;
            FA_LAUNCH(kernel, grid, dim3(64 * kVarlenWaves), (size_t)lds, static_cast<hipStream_t>(d->stream), a);
            return launch_status();
        };
        constexpr bool kF32 = decltype(f32)::value;
        if (d->d == 64)
            return causal ? launch(fa_fwd_varlen_kernel<T, 64, kF32, true, kLogits>, TileGeom<64>::kLdsBytes)
                          : launch(fa_fwd_varlen_kernel<T, 64, kF32, false, kLogits>, TileGeom<64>::kLdsBytes);
        return causal ? launch(fa_fwd_varlen_kernel<T, 128, kF32, true, kLogits>, TileGeom<128>::kLdsBytes)
                      : launch(fa_fwd_varlen_kernel<T, 128, kF32, false, kLogits>, TileGeom<128>::kLdsBytes);
    });
}

// the LONG half of fa_kvcache_attend_varlen: varlen_cache_launch's choice among the kRouted instantiations (causal only), with the
// threshold behind the checked arguments.  Base: VarlenCacheArgs or VarlenCacheFp8Args
template <bool kLogits, typename Base>
static inline hipError_t varlen_cache_routed_launch(const fa_varlen_kvcache_desc* d, const Base& base, dim3 grid, int min_rows)
{
    VarlenRoutedArgs<Base> a;
    static_cast<Base&>(a) = base;
    a.min_rows = min_rows;
    const bool paged = d->block_table != nullptr;
    return with_types(d->in_dtype, d->out_dtype, [&](auto t, auto f32) {
        using T = decltype(t);
        constexpr bool kF32 = decltype(f32)::value;
        constexpr bool kFp8 = std::is_same_v<Base, VarlenCacheFp8Args>;
        auto launch = [&](auto kernel, int lds) {
            const hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), lds);
            if (attr != hipSuccess) return attr;
            FA_LAUNCH(kernel, grid, dim3(64 * kVarlenWaves), (size_t)lds, static_cast<hipStream_t>(d->stream), a);
            return launch_status();
        };
        if (d->d == 64)
            return paged ? launch(fa_fwd_varlen_kernel<T, 64, kF32, true, kLogits, kVarlenPaged, kFp8, true>, TileGeom<64>::kLdsBytes)
                         : launch(fa_fwd_varlen_kernel<T, 64, kF32, true, kLogits, kVarlenContig, kFp8, true>, TileGeom<64>::kLdsBytes);
        return paged ? launch(fa_fwd_varlen_kernel<T, 128, kF32, true, kLogits, kVarlenPaged, kFp8, true>, TileGeom<128>::kLdsBytes)
                     : launch(fa_fwd_varlen_kernel<T, 128, kF32, true, kLogits, kVarlenContig, kFp8, true>, TileGeom<128>::kLdsBytes);
    });
}

// the one launch of fa_forward_varlen_kvcache: the cache instantiation of (types, d, causal, paged) with the unit's kLogits
// (Args a VarlenCacheFp8Args: of fa_forward_varlen_kvcache_fp8, the fp8 one)
template <bool kLogits, typename Args>
static inline hipError_t varlen_cache_launch(const fa_varlen_kvcache_desc* d, const Args& a, dim3 grid)
{
    const bool causal = d->causal != 0, paged = d->block_table != nullptr;
    return with_types(d->in_dtype, d->out_dtype, [&](auto t, auto f32) {
        using T = decltype(t);
        auto launch = [&](auto kernel, int lds) {
            const hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), lds);
            if (attr != hipSuccess) return attr;
            FA_LAUNCH(kernel, grid, dim3(64 * kVarlenWaves), (size_t)lds, static_cast<hipStream_t>(d->stream), a);
            return launch_status();
        };
        constexpr bool kF32 = decltype(f32)::value;
        auto by_mask = [&](auto dd, auto pp) {
            constexpr int D = decltype(dd)::value;
            constexpr int kCache = decltype(pp)::value ? kVarlenPaged : kVarlenContig;
            constexpr bool kFp8 = std::is_same_v<Args, VarlenCacheFp8Args>;
            return causal ? launch(fa_fwd_varlen_kernel<T, D, kF32, true, kLogits, kCache, kFp8>, TileGeom<D>::kLdsBytes)
                          : launch(fa_fwd_varlen_kernel<T, D, kF32, false, kLogits, kCache, kFp8>, TileGeom<D>::kLdsBytes);
        };
        using D64 = std::integral_constant<int, 64>;
        using D128 = std::integral_constant<int, 128>;
        if (d->d == 64) return paged ? by_mask(D64{}, std::true_type{}) : by_mask(D64{}, std::false_type{});
        return paged ? by_mask(D128{}, std::true_type{}) : by_mask(D128{}, std::false_type{});
    });
}

}  // namespace fa
