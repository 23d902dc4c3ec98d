// fa_fwd_varlen256_kernel.hpp -- device code of fa_forward_varlen_d256 and fa_forward_varlen_kvcache_d256 (fa_fwd_varlen256.hip): the
// variable-length prefill at head dimension 256 (the Gemma-2 / Gemma-3 head), K/V token-packed, in a contiguous cache or in page
// pools, with the causal mask, the sliding window and the soft-cap.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md
// 7.26.  A kernel of its own: the d <= 128 varlen kernel (fa_fwd_varlen_kernel.hpp) runs two workgroups per CU at <= 256 registers a
// lane, and a 32-row wave at d = 256 holds 128 accumulators for O^T, 64 registers of Q^T and 32 of S^T before anything is staged.
//   * work split: the varlen kernel's, unchanged in meaning -- floor(total_q / 128) + B slots per query head, slot -> (sequence, query
//     block) by a scalar binary search over cu_seqlens_q, the G heads of a group adjacent on an XCD, the long blocks first under the
//     mask; 128-row workgroups of four waves, each wave owning 32 rows and ALL 256 columns of them;
//   * one workgroup per CU (__launch_bounds__(256, 1)): a wave has a SIMD's whole register file (O^T 128, Q^T 64, S^T 32, packed P 16,
//     the tile in flight 64);
//   * LDS: the K and the V image of a 64-key tile are kv256::img_off's (fa_fwd_kv256_kernel.hpp: 512-byte rows, the XOR swizzle that
//     is conflict-free for the ds_read_b128 row reads of S^T and the ds_read_b64_tr_b16 reads of V^T), 32 KiB each, double-buffered:
//     128 KiB.  The next tile's 16 loads per lane are issued before the current tile's arithmetic and written to the other buffer
//     behind it: one barrier per tile;
//   * MFMA: v_mfma_f32_32x32x16 in the project's orientation, S^T = K.Q^T (2 key blocks x 16 steps) and O^T += V^T.P^T with the packed
//     P straight from the accumulators as the B operand (8 column blocks x 4 steps); every wave reads both images whole;
//   * staging: kv256's shape -- the tile's eight 8-row groups are dealt to the waves, two each; a cache form makes one buffer
//     descriptor per (wave, group), 64-bit base, ending at the last row below Lk (rows past it read 0); eight aligned rows lie inside
//     one page of >= 16 keys, so the page number is wave-uniform and sits in a scalar register; the table entries are fetched a tile
//     ahead, the entry index clamped to [page of lo_wg, last live page]; a page number outside [0, num_pages) and a group wholly below
//     lo_wg get a descriptor of no records, and the rows of the first streamed tile below lo_wg are zeroed in their registers (a
//     masked weight of 0 times a NaN is a NaN in the PV MFMA).  The packed form runs the same code on the strided (sequence, head)
//     view: the descriptor's base is the group's first token row, a row is stride_t elements;
//   * softmax: the varlen kernel's lazy running maximum; the weights' row sum is that of the ROUNDED weights, as in the d = 256
//     decode.  A wave skips the tiles wholly outside [lo of its first row, limit of its last row) -- it still stages and synchronises
//     -- and only the tiles that straddle a limit of the wave take the per-score compare (one unsigned compare for both limits);
//   * causal, window and soft-cap are runtime and wave-uniform (kernel arguments, scalar registers): 12 instantiations, type x output
//     x {packed, contiguous, paged}.  "No window" is a W that masks nothing (the host's clamp); cap2 == 0 skips the cap by a branch.
// Tiles stay at absolute multiples of 64 keys from key 0 and the three forms differ in where a row comes from alone, so on the same
// finite keys they return the same bits.
// kFp8 (fa_forward_varlen_kvcache_d256_fp8, the 8 cache instantiations of fa_fwd_varlen256_fp8.hip): K and V address
// one e4m3fn byte per element.  Only the staging differs: an 8-row group is 2 KiB, two 16-byte loads per lane by kv256's e4m3fn lane
// map (fp8_row, fp8_ld_off: two rows to a quarter wave, so every ds_write_b128 round keeps 16 slots), the descriptors cover
// (rows - 1) * 256 + 256 bytes, so what lies outside them reads as the code 0 (+0) whatever NaN codes memory holds, the rows of the
// first tile below lo_wg are zeroed as raw bytes, and the raw bytes wait in 32 registers through the tile's arithmetic and are
// widened exactly to T (fp8x16_widen) in stage_write, into the same images.  k_scale[hkv] joins the logit factor before the clamp and
// the cap's constant, v_scale[hkv] joins 1 / l.  With both null every factor keeps its bits: the 16-bit kernel's result on the widened
// cache.  Private to csrc/.
#pragma once
#include "fa_fwd_kv256_kernel.hpp"    // kv256::img_off, swz and the image constants
#include "fa_fwd_varlen_kernel.hpp"   // varlen_bounds, varlen_rsrc, the slot constants

namespace fa {

namespace varlen256 {
constexpr int kD = kv256::kD;
constexpr int kTile = kv256::kTile;
constexpr int kRowBytes = kv256::kRowBytes;
constexpr int kImgBytes = kv256::kImgBytes;      // 32 KiB: one image
constexpr int kBufBytes = 2 * kImgBytes;         // K then V of one tile
constexpr int kLdsBytes = 2 * kBufBytes;         // 128 KiB of the CU's 160: one workgroup per CU
constexpr int kKSteps = kv256::kKSteps;          // 16
constexpr int kDBlocks = kD / 32;                // 8 32-column blocks of O^T, all with every wave
constexpr int kGroups = kv256::kGroups;          // 2 eight-row groups of a tile per wave
constexpr int kGroupLoads = kv256::kGroupLoads;  // 4 16-byte loads per lane and group

constexpr int kPacked = 0, kContig = 1, kPaged = 2;   // where the K/V rows come from

struct Dev {
    const uint16_t* Q;
    void* O;
    float* lse;
    const char *K, *V;                   // packed tensors, the cache, or the pools
    const int *cu_q, *cu_k, *seqlens, *table;
    int B, Hkv, G, total_q, total_k;     // total_k: the packed K/V rows, or the capacity of a cache
    unsigned nslots;                     // floor(total_q / 128) + B
    int max_pages, num_pages, lg_page;   // paged only
    long long q_st, q_sh, k_st, k_sh, v_st, v_sh, o_st, o_sh;   // elements; k_*, v_*: packed only
    float scale_log2e;
    float cap2, cap_rk;                  // softcap * log2(e) and 2 / softcap; 0: no cap
    int causal, window;                  // window >= 1: "none" comes in as total_q + total_k
    const float *k_scale, *v_scale;      // kFp8 only: [Hkv] on the device, or nullptr (1.0).  Last, so that no other field moves
};
}  // namespace varlen256

template <typename T, bool kOutF32, int kForm, bool kFp8 = false>
__global__ __launch_bounds__(64 * kVarlenWaves, 1)
void fa_fwd_varlen256_kernel(varlen256::Dev a)
{
    using namespace varlen256;
    using kv256::img_off;
    using kv256::swz;
    static_assert(!kFp8 || kForm != kPacked, "an e4m3fn source is a cache");
    constexpr unsigned W = kVarlenWaves, BM = kVarlenRows;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool causal = a.causal != 0;

    // ---- block -> (K/V head, slot, head of the group): blocks that share K/V sit on one XCD, consecutively ----
    const unsigned nwg = gridDim.x, bid = blockIdx.x;
    const unsigned xq = nwg >> 3, xr = nwg & 7u, xcd = bid & 7u;
    const unsigned wgid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    const unsigned grp = wgid / (unsigned)a.G, g_hd = wgid - grp * (unsigned)a.G;
    const unsigned hkv = grp / a.nslots, sidx = grp - hkv * a.nslots;
    const unsigned slot = causal ? a.nslots - 1u - sidx : sidx;   // under the mask the last blocks of a sequence are the long ones
    const unsigned hq = hkv * (unsigned)a.G + g_hd;

    // ---- slot -> (sequence, query block): the largest b with first_b <= slot (wave-uniform: scalar loads) ----
    const int* __restrict__ cu_q = a.cu_q;
    unsigned lo_b = 0, hi_b = (unsigned)a.B;
    while (hi_b - lo_b > 1u) {
        const unsigned mid = (lo_b + hi_b) >> 1;
        const unsigned first = (unsigned)min(max(cu_q[mid], 0), a.total_q) / BM + mid;
        if (first <= slot) lo_b = mid; else hi_b = mid;
    }
    const unsigned b = lo_b;
    int sq, eq, sk = 0, ek;
    varlen_bounds(cu_q, b, a.total_q, sq, eq);
    if constexpr (kForm != kPacked) ek = min(max(a.seqlens[b], 0), a.total_k);   // the keys of sequence b are the cache rows [0, Lk)
    else varlen_bounds(a.cu_k, b, a.total_k, sk, ek);
    const int Lq = eq - sq, Lk = ek - sk;
    const unsigned first_b = (unsigned)sq / BM + b;
    if (slot < first_b) return;                        // slots below the first sequence's
    const unsigned qb = slot - first_b;
    if ((unsigned long long)qb * BM >= (unsigned long long)Lq) return;   // a spare slot of the sequence

    const unsigned tid = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u, r = lane & 31u, h = lane >> 5;

    const unsigned wave_row0 = qb * BM + wave * 32u;   // first query row of this wave, in the sequence
    const unsigned q_row = wave_row0 + r;
    const bool row_live = q_row < (unsigned)Lq;
    const int shift = Lk - Lq;                         // causal: row i sees the keys j <= i + shift

    // ---- the limits.  Row i sees [lo_i, hi_i): hi_i = Lk, or under causal max(0, shift + 1 + i) (<= Lk for a row below Lq; cut to
    // Lk for the others), lo_i = max(0, shift + 1 + i - W).  |shift + 1 + row| <= 2^26 and W <= 2^27 by the host's checks.
    auto hi_of = [&](unsigned row) { return causal ? (unsigned)min(max(shift + 1 + (int)row, 0), Lk) : (unsigned)Lk; };
    auto lo_of = [&](unsigned row) { return (unsigned)max(shift + 1 + (int)row - a.window, 0); };
    const unsigned lo_wg = lo_of(qb * BM);             // no row of the workgroup sees a key below it: nothing below it is used
    const unsigned klim = hi_of(min((unsigned)Lq - 1u, qb * BM + BM - 1u));   // the limit of the workgroup's last existing row
    const int t0 = (int)(lo_wg / kTile), ntiles = (int)((klim + kTile - 1) / kTile);
    const unsigned lo_first = lo_of(wave_row0), lo_last = lo_of(wave_row0 + 31u);   // the wave's smallest and largest lower limit
    const unsigned hi_first = hi_of(wave_row0), hi_last = hi_of(wave_row0 + 31u);   // ... and upper limit
    const unsigned lo_row = lo_of(q_row), hi_row = hi_of(q_row);
    const unsigned seen = hi_row > lo_row ? hi_row - lo_row : 0u;

    // ---- Q^T fragments (B operand of S^T = K.Q^T), resident for the whole kernel; rows at or past Lq are zeros ----
    float sl2 = a.scale_log2e;
    if constexpr (kFp8) {
        if (a.k_scale) sl2 *= a.k_scale[hkv];   // before the clamp, and under a cap what the cap sees
    }
    const float c = fmaxf(fabsf(sl2), 1.17549435e-38f);   // a scale of 0 must not meet a masked -inf as 0 * -inf
    const unsigned q_flip = a.scale_log2e < 0.0f ? 0x80008000u : 0u;
    // what a score is multiplied by on its way into the vote and the exponent (1 once the cap has made the scores final), and the
    // cap's two constants, in scalar registers
    const float cs = to_sgpr(a.cap2 > 0.0f ? 1.0f : c);
    const float cap_k1 = to_sgpr(c * a.cap_rk), cap_n2 = to_sgpr(-2.0f * a.cap2);
    const __amdgpu_buffer_rsrc_t rq = varlen_rsrc(a.Q, sq, Lq, hq, a.q_st, a.q_sh, kD, 2u);
    u32x4 qf[kKSteps];
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) {
        u32x4 raw = buf_load16(rq, (row_live ? q_row * ((unsigned)a.q_st * 2u) : 0u) + (16u * s + 8u * h) * 2u);
#pragma unroll
        for (int w = 0; w < 4; ++w) raw[w] = row_live ? raw[w] ^ q_flip : 0u;
        qf[s] = raw;
    }

    // ---- staging: group g of the tile's 8-row groups that this wave loads is group g * W + wave; lane idx = lane + 64 p of a group is
    // chunk idx % 32 = r of row idx / 32 = 2 p + h, which in a cache is byte idx * 16 of the group ----
    // kFp8: kv256's e4m3fn lane map -- load p of a lane is the 16 codes j + 8 p of row fp8_row(lane) of the group, which widened are
    // the chunks 2 (j + 8 p) and the one after it of that row: l_off[0] is chunk 2 j in the image, the odd chunk lies at l_off[0] ^ 16
    constexpr int kLoads = kFp8 ? kv256::kGroupLoads8 : kGroupLoads;   // 2 or 4 16-byte loads per lane, group and tensor
    constexpr unsigned kSrcRow = kFp8 ? kv256::kRowBytes8 : kRowBytes;  // bytes of a cache row
    unsigned l_off[kFp8 ? 1 : kGroupLoads];
    if constexpr (kFp8) {
        l_off[0] = img_off(wave * 8u + kv256::fp8_row(lane), 2u * (lane & 7u));
    } else {
#pragma unroll
        for (int p = 0; p < kGroupLoads; ++p) l_off[p] = img_off(wave * 8u + 2u * p + h, r);   // swz has period 16: g adds 32 rows
    }
    const char *kbase = a.K, *vbase = a.V;
    if constexpr (kForm == kContig) {
        kbase += ((size_t)b * (unsigned)a.Hkv + hkv) * (unsigned)a.total_k * kSrcRow;
        vbase += ((size_t)b * (unsigned)a.Hkv + hkv) * (unsigned)a.total_k * kSrcRow;
    }
    // packed: the (sequence, head) view starts (sk * stride_t + hkv * stride_h) elements in, and a token row is stride_t elements
    // (every offset of an existing row fits 32 bits: checked on the host); a cache row is 512 bytes, or 256 codes
    unsigned k_stb = kSrcRow, v_stb = kSrcRow;
    if constexpr (kForm == kPacked) {
        k_stb = (unsigned)a.k_st * 2u;
        v_stb = (unsigned)a.v_st * 2u;
        kbase += ((long long)sk * a.k_st + (long long)hkv * a.k_sh) * 2;
        vbase += ((long long)sk * a.v_st + (long long)hkv * a.v_sh) * 2;
    }
    // the lane's byte offset inside a group, per tensor (the same register for both in a cache)
    unsigned k_off[kLoads], v_off[kLoads];
#pragma unroll
    for (int p = 0; p < kLoads; ++p) {
        if constexpr (kFp8) {
            k_off[p] = v_off[p] = kv256::fp8_ld_off(lane) + 128u * p;
        } else {
            k_off[p] = (2u * p + h) * k_stb + r * 16u;
            v_off[p] = (2u * p + h) * v_stb + r * 16u;
        }
    }
    u32x4 kst[kGroups][kLoads], vst[kGroups][kLoads];   // kFp8: the raw codes, 32 registers where the 16-bit tile takes 64
    // paged: the page numbers of the tile that is staged next, one per (wave, group), in scalar registers.  Only called with Lk >= 1;
    // the entry index is clamped to [page of lo_wg, last live page] (lo_wg < Lk whenever a tile is streamed), so no entry at or past
    // ceil(Lk / page) and no entry of a page wholly below the window is read, and a tile index past the last tile is harmless
    [[maybe_unused]] int pg[kGroups];
    [[maybe_unused]] auto fetch_pages = [&](unsigned kv0) {
        if constexpr (kForm == kPaged) {
            const int* __restrict__ tbl = a.table + (size_t)b * (unsigned)a.max_pages;
            const unsigned last = ((unsigned)Lk - 1u) >> a.lg_page;
#pragma unroll
            for (int g = 0; g < kGroups; ++g) {
                const unsigned e = max(min((kv0 + (g * W + wave) * 8u) >> a.lg_page, last), lo_wg >> a.lg_page);
                pg[g] = __builtin_amdgcn_readfirstlane(tbl[e]);
            }
        }
    };
    // One descriptor per (wave, group) and tensor: it starts at the group's first row and ends with its last row below Lk, so the
    // loads of the rows past it read 0 whatever memory holds: offset j * stride + 16 r of row j >= rows lies at or past the
    // (rows - 1) * stride + 512 bytes of the range (kFp8: offset j * 256 + ... at or past rows * 256; what is not read is the code 0).  (Packed, with a token stride beyond 2^29 bytes such an offset may wrap 32 bits
    // into the range: it then reads a live row of the same sequence, whose score is masked.)
    auto stage_load = [&](unsigned kv0) {
#pragma unroll
        for (int g = 0; g < kGroups; ++g) {
            const unsigned kg = kv0 + (g * W + wave) * 8u;                          // the group's first key
            unsigned rows = kg < (unsigned)Lk ? min(8u, (unsigned)Lk - kg) : 0u;    // its rows below Lk
            if constexpr (kForm != kPacked) {
                if (kg + 8u <= lo_wg) rows = 0u;                                    // wholly below the window: pg[g] is another page's
            }
            size_t row0 = kg;                                                       // the row of `kbase` the group starts at
            if constexpr (kForm == kPaged) {
                if ((unsigned)pg[g] >= (unsigned)a.num_pages) rows = 0u;            // a bad page number: no record, every load reads 0
                row0 = (((size_t)(unsigned)pg[g] * (unsigned)a.Hkv + hkv) << a.lg_page) + (kg & ((1u << a.lg_page) - 1u));
            }
            if (!rows) row0 = 0;
            const __amdgpu_buffer_rsrc_t rk = make_rsrc(kbase + row0 * k_stb, rows ? (rows - 1u) * k_stb + kSrcRow : 0u),
                                         rv = make_rsrc(vbase + row0 * v_stb, rows ? (rows - 1u) * v_stb + kSrcRow : 0u);
#pragma unroll
            for (int p = 0; p < kLoads; ++p) {
                kst[g][p] = buf_load16(rk, k_off[p]);
                vst[g][p] = buf_load16(rv, v_off[p]);
            }
        }
    };
    // a cache under a window: the rows of the first streamed tile below lo_wg go to LDS as zeros (workgroup-uniform, tile t0 only).
    // kFp8: the raw bytes are zeroed -- the code 0 is +0 -- by the e4m3fn lane-to-row map, which does not depend on p
    [[maybe_unused]] auto stage_zero_below = [&](unsigned kv0) {
        if (kv0 < lo_wg) {
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
#pragma unroll
                for (int p = 0; p < kLoads; ++p) {
                    if constexpr (kFp8) {
                        if (kv0 + (g * W + wave) * 8u + kv256::fp8_row(lane) < lo_wg) kst[g][p] = vst[g][p] = u32x4{0u, 0u, 0u, 0u};
                    } else {
                        if (kv0 + (g * W + wave) * 8u + 2u * p + h < lo_wg) kst[g][p] = vst[g][p] = u32x4{0u, 0u, 0u, 0u};
                    }
                }
        }
    };
    auto stage_write = [&](unsigned buf) {
#pragma unroll
        for (int g = 0; g < kGroups; ++g)
#pragma unroll
            for (int p = 0; p < kLoads; ++p) {
                if constexpr (kFp8) {   // one load is the row's chunks 2 c and 2 c + 1, c = j + 8 p: the even round, then the odd one
                    const unsigned at = buf * kBufBytes + g * (W * 8 * kRowBytes) + p * 256u;   // a multiple of 256
                    u32x4 klo, khi, vlo, vhi;
                    fp8x16_widen<T>(kst[g][p], klo, khi);
                    fp8x16_widen<T>(vst[g][p], vlo, vhi);
                    lds_write16(smem, at + l_off[0], klo);
                    lds_write16(smem, at + (l_off[0] ^ 16u), khi);
                    lds_write16(smem, kImgBytes + at + l_off[0], vlo);
                    lds_write16(smem, kImgBytes + at + (l_off[0] ^ 16u), vhi);
                } else {
                    lds_write16(smem, buf * kBufBytes + g * (W * 8 * kRowBytes) + l_off[p], kst[g][p]);
                    lds_write16(smem, buf * kBufBytes + kImgBytes + g * (W * 8 * kRowBytes) + l_off[p], vst[g][p]);
                }
            }
    };

    // ---- per-lane LDS read addresses (kv256's images) ----
    // row reads of S^T: lane (r, h) takes chunk 2 ks + h of key kb * 32 + r.  (2 ks + h) ^ x = 2 (ks % 8) ^ (h ^ x) in the low four
    // bits, so one register holds the address and a step XORs (ks % 8) << 5 into it; ks / 8 and kb are immediates
    const unsigned k_rd = r * kRowBytes + ((h ^ swz(r)) << 4);
    // transposed reads of V^T: lane 4 vq + vp of a 16-lane group supplies row vq, columns 4 vp .. 4 vp + 3 of the block of keys
    // 16 q4 + 8 jj + 4 h .. + 3 and columns 32 db + 16 vg .. + 15, i.e. chunk 4 db + 2 vg + vp / 2.  The swizzle XORs the chunk's low
    // four bits: one address per (jj, db % 4); db / 4 (chunk bit 4: 256 bytes) and q4 (16 rows) are immediates
    const unsigned i16 = lane & 15u, vq = i16 >> 2, vp = i16 & 3u, vg = (lane >> 4) & 1u;
    unsigned v_rd[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v_rd[jj][k] = kImgBytes + img_off(8u * jj + 4u * h + vq, 4u * k + 2u * vg + (vp >> 1)) + (vp & 1u) * 8u;

    // ---- running state ----
    f32x16 zero16;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero16[i] = 0.0f;
    f32x16 o[kDBlocks];
#pragma unroll
    for (int db = 0; db < kDBlocks; ++db) o[db] = zero16;
    float m_ref = -INFINITY;   // reference max of this lane's query row, in log2 units; -inf: no key seen yet
    float l_part = 0.0f;       // this half-wave's share of the row sum

    // the loop runs over the tiles [t0, ntiles), tile t in buffer t & 1 (t0 < ntiles whenever ntiles > 0: lo < hi for a row with hi >= 1)
    if (t0 < ntiles) {
        fetch_pages((unsigned)t0 * kTile);
        stage_load((unsigned)t0 * kTile);
        fetch_pages((unsigned)(t0 + 1) * kTile);
        if constexpr (kForm != kPacked) stage_zero_below((unsigned)t0 * kTile);
        stage_write((unsigned)t0 & 1u);
    }
    __syncthreads();

    for (int t = t0; t < ntiles; ++t) {
        const unsigned kv0 = (unsigned)t * kTile, cur = (unsigned)t & 1u;
        const char* kbuf = smem + cur * kBufBytes;
        if (t + 1 < ntiles) stage_load(kv0 + kTile);
        fetch_pages(kv0 + 2u * kTile);   // the table read of the tile after next overlaps this tile's arithmetic
        // tiles wholly at or past the limit of this wave's last row, or wholly below the lower limit of its first, contribute nothing
        if (kv0 < hi_last && kv0 + kTile > lo_first && wave_row0 < (unsigned)Lq) {   // ... nor does a wave without a row

        // ---- S^T = K.Q^T (raw fp32 scores); consecutive MFMAs alternate accumulators ----
        f32x16 s[2];
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const u32x4 kf = lds_read16(kbuf, (k_rd ^ ((unsigned)(ks & 7) << 5)) + (unsigned)(ks >> 3) * 256u + kb * 32u * kRowBytes);
                s[kb] = T::mfma32(kf, qf[ks], ks == 0 ? zero16 : s[kb]);
            }
        if (a.cap2 > 0.0f) {   // wave-uniform; before the masks, so a masked key stays at -inf: the scores are final after it
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    s[kb][i] = __builtin_fmaf(cap_n2, __builtin_amdgcn_rcpf(1.0f + fast_exp2(s[kb][i] * cap_k1)), a.cap2);
        }
        // keys outside [lo, hi) -> -inf: one unsigned compare per score, in the tiles that reach past the wave's smallest upper limit
        // (the last tile's keys at or past Lk among them) or start below its largest lower one
        if (kv0 + kTile > hi_first || kv0 < lo_last) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned key = kv0 + (unsigned)(kb * 32 + (i & 3) + 8 * (i >> 2)) + 4u * h;
                    if (key - lo_row >= seen) s[kb][i] = -INFINITY;
                }
        }

        // ---- tile max vs the reference max; raise the reference only when needed ----
        float tmax = -INFINITY;
#pragma unroll
        for (int e = 0; e < 32; e += 2) tmax = max3(tmax, s[e >> 4][e & 15], s[(e + 1) >> 4][(e + 1) & 15]);
        tmax *= cs;   // log2 units; -inf: the row sees no key of this tile
        // a row that has seen no key has m_ref = -inf: a first key raises it (inf > kThr), none leaves it (NaN > kThr is false)
        if (__any(tmax - m_ref > kThr)) {
            const float mx = fmaxf(tmax, swap_halves(tmax));         // row max, same in both halves
            const float m_new = fmaxf(mx, m_ref);
            const float alpha = m_ref == -INFINITY ? 0.0f : fast_exp2(m_ref - m_new);   // never 2^(-inf - -inf)
            m_ref = m_new;
#pragma unroll
            for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
            l_part *= alpha;
        }

        // ---- p = 2^(cs*S - m_ref), packed to 16 bit (B operand of PV); the row-sum share is that of the rounded weights ----
        u32x4 pk[4];
        float ls0 = 0.0f, ls1 = 0.0f;
        const float neg_m = m_ref == -INFINITY ? 0.0f : -m_ref;   // every score of such a row is -inf: p = 2^-inf = 0
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int kb = q4 >> 1, b8 = (q4 & 1) * 8;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float p0 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w], cs, neg_m));
                const float p1 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w + 1], cs, neg_m));
                pk[q4][w] = T::pack2(p0, p1);
                if (w & 1) ls1 = T::sum2(pk[q4][w], ls1);
                else ls0 = T::sum2(pk[q4][w], ls0);
            }
        }
        l_part += ls0 + ls1;

        // ---- O^T += V^T.P^T ----
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
            for (int db = 0; db < kDBlocks; ++db) {
                u32x4 vf;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const u32x2 half = lds_read_tr8(kbuf, q4 * 16u * kRowBytes + (unsigned)(db >> 2) * 256u + v_rd[jj][db & 3]);
                    vf[2 * jj] = half[0];
                    vf[2 * jj + 1] = half[1];
                }
                o[db] = T::mfma32(vf, pk[q4], o[db]);
            }
        }   // the wave has work in this tile

        if (t + 1 < ntiles) stage_write(cur ^ 1u);
        __syncthreads();
    }

    // ---- normalise and store: lane holds O[q_row][db*32 + 8g + 4h + 0..3] in o[db][4g..4g+3] ----
    if (!row_live) return;                             // rows at or past Lq are the next sequence's, or nobody's
    const float l = l_part + swap_halves(l_part);
    const bool none = m_ref == -INFINITY;              // the row saw no key: O = 0 and lse = -inf, never 0/0
    float inv = none ? 0.0f : 1.0f / l;
    if constexpr (kFp8) {
        if (a.v_scale) inv *= a.v_scale[hkv];
    }
    if (a.lse && h == 0)
        a.lse[(size_t)hq * (size_t)a.total_q + (size_t)sq + q_row] = none ? -INFINITY : (m_ref + __log2f(l)) * kLn2;
    constexpr unsigned es = kOutF32 ? 4u : 2u;
    const __amdgpu_buffer_rsrc_t ro = varlen_rsrc(a.O, sq, Lq, hq, a.o_st, a.o_sh, kD, es);
    const unsigned o_row = q_row * ((unsigned)a.o_st * es);
#pragma unroll
    for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const unsigned col = db * 32u + 8u * gg + 4u * h;
            const float x0 = none ? 0.0f : o[db][4 * gg] * inv, x1 = none ? 0.0f : o[db][4 * gg + 1] * inv;
            const float x2 = none ? 0.0f : o[db][4 * gg + 2] * inv, x3 = none ? 0.0f : o[db][4 * gg + 3] * inv;
            if constexpr (kOutF32) {
                const f32x4 v = {x0, x1, x2, x3};
                buf_store16(ro, o_row + col * 4u, __builtin_bit_cast(u32x4, v));
            } else {
                buf_store8(ro, o_row + col * 2u, u32x2{T::pack2(x0, x1), T::pack2(x2, x3)});
            }
        }
}

// The one launch of a checked call: the instantiation of (types, form, element size).
template <int kForm, bool kFp8>
hipError_t varlen256_launch(const varlen256::Dev& a, dim3 grid, int in_dtype, int out_dtype, void* stream)
{
    return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
        auto kernel = fa_fwd_varlen256_kernel<decltype(t), decltype(f32)::value, kForm, kFp8>;
        const hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), varlen256::kLdsBytes);
        if (attr != hipSuccess) return attr;
        FA_LAUNCH(kernel, grid, dim3(64 * kVarlenWaves), (size_t)varlen256::kLdsBytes, static_cast<hipStream_t>(stream), a);
        return launch_status();
    });
}
// fa_fwd_varlen256_fp8.hip: varlen256_launch<kContig | kPaged, true>, the fp8 unit's instantiations behind the checks of
// fa_fwd_varlen256.hip
hipError_t varlen256_launch_fp8(const varlen256::Dev& a, dim3 grid, int in_dtype, int out_dtype, bool paged, void* stream);

}  // namespace fa
