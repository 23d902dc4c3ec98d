// fa_fwd_kv256_kernel.hpp -- device code of fa_kvcache_decode_d256 (fa_fwd_kv256.hip) and, with kFp8, of fa_kvcache_decode_d256_fp8
// (fa_fwd_kv256_fp8.hip: rows of 256 e4m3fn codes, widened on their way into LDS): token-packed split-KV decode against a
// KV cache at head dimension 256, contiguous and paged, with the causal tail, the sliding window and the soft-cap.  A kernel of its
// own on the plan of the split-KV stream (fa_fwd_split_kernel.hpp, whose TileGeom<64|128> sits at its register limits): the G * n_b
// rows of a (sequence, K/V head) are folded into 32-row blocks, lengths, cu_seqlens and the block table are read on the device, the
// 64-key tiles of a sequence from start_t on are dealt to S splits, and a private merge kernel finishes behind a split.  What is new
// is the tile at 512-byte rows: ALL FOUR waves of a workgroup own the SAME 32 rows, every wave computes the whole S^T = K Q^T of the
// tile (so all four hold the same (m, l) and the same packed P, bit for bit, from the same LDS bytes), and the 256 columns of V are
// split over the waves: a wave keeps O^T for 64 columns in 32 accumulator registers and reads only its quarter of the V image.
// Private to csrc/.  DESIGN.md sections 7.25 and 7.27, profiles/kv256_decode.txt, profiles/kv256_fp8.txt.
#pragma once
#include "../../include/fa_mi355.h"
#include "fa_dispatch.hpp"
#include "fa_fwd_split_kernel.hpp"   // packed_rows, packed_rsrc, to_sgpr, kLn2

namespace fa {

namespace kv256 {
constexpr int kD = 256;
constexpr int kW = 4;                          // waves per workgroup
constexpr int kRows = 32;                      // query rows per workgroup: one block, shared by the four waves
constexpr int kTile = 64;                      // keys per tile, and the unit the splits deal out
constexpr int kRowBytes = kD * 2;              // 512
constexpr int kChunks = kD / 8;                // 32 16-byte chunks per row
constexpr int kKSteps = kD / 16;               // 16 steps of the 32x32x16 instruction over the reduction dimension of S^T
constexpr int kImgBytes = kTile * kRowBytes;   // 32 KiB: the K image; the V image follows it
constexpr int kLdsBytes = 2 * kImgBytes;       // 64 KiB, single-buffered: two workgroups per CU (128 of 160 KiB)
constexpr int kDBlocks = kD / 32 / kW;         // 2 32-column blocks of O^T per wave
constexpr int kGroups = kTile / 8 / kW;        // 2 eight-row groups of a tile each wave stages, for K and for V
constexpr int kGroupLoads = 8 * kChunks / 64;  // 4 16-byte loads per lane and group
constexpr int kWsRow = kD + 4;                 // floats per workspace row: O^T, m, l and two of padding (rows stay 16-byte aligned)
constexpr int kRowBytes8 = kD;                 // an e4m3fn cache row: 256 bytes, 16 loads of 16 bytes
constexpr int kGroupLoads8 = 8 * kRowBytes8 / 16 / 64;   // 2 16-byte loads per lane and group of an e4m3fn cache

// The LDS images, K and V alike: row-major rows of 512 bytes, the low four bits of the 16-byte chunk index XORed with x(row).
// A row is two bank rows (64 banks x 4 bytes = 16 slots of 16 bytes), so without the XOR chunk c of EVERY row lies in slot c % 16.
//   x(row) = (row & 3) << 2 | (row >> 2) & 3      -- the row's low four bits with its two bit pairs exchanged
// Row reads of S^T (ds_read_b128, 16 lanes at a time: 16 consecutive rows, the same chunk c): x is a bijection of row % 16 onto
// 0..15, so the slots (c ^ x) % 16 are 16 different ones.  Transposed reads of PV (ds_read_b64_tr_b16, 32 lanes at a time: rows
// 4n .. 4n + 3 times the chunks c0 .. c0 + 3, c0 % 4 == 0, both 8-byte halves of each): slot = (c0 ^ (row & 3) << 2) | (k ^ n % 4)
// for chunk c0 + k -- the four rows differ in the slot's high pair, the four chunks in its low pair: 16 different slots, and the two
// halves of a chunk are different banks of its slot.  (With x = row % 16, the d = 128 image's map, the four rows of a transposed
// read would share four slots.)  Staging writes (ds_write_b128: 16 lanes are 16 consecutive chunks of one row) keep 16 slots under
// any XOR.  x has period 16 in the row, so a block of 16 or 32 rows further down adds an immediate offset and nothing else.
__device__ __forceinline__ unsigned swz(unsigned row) { return ((row & 3u) << 2) | ((row >> 2) & 3u); }
__device__ __forceinline__ unsigned img_off(unsigned row, unsigned chunk)
{
    return row * kRowBytes + (((chunk & 16u) | ((chunk & 15u) ^ swz(row))) << 4);
}

struct Dev {
    const uint16_t* Q;
    void* O;
    float* lse;
    const char *K, *V;
    float* ws;
    const int *cu_q, *seqlens, *table;
    int B, Hkv, G, total_q, max_q, cap;
    int max_pages, num_pages, lg_page;   // paged only
    long long q_st, q_sh, o_st, o_sh;    // elements
    float scale_log2e;
    float cap2, cap_rk;                  // softcap * log2(e) and 2 / softcap; 0: no cap
    int causal, window;                  // window >= 1: "none" comes in as the capacity
    int S, nqb;
    const float *k_scale, *v_scale;      // kFp8 only: [Hkv] on the device, or nullptr (1.0).  Last, so that no other field moves
};

// The staging of an e4m3fn cache (kFp8).  An 8-row group is 2 KiB, two 16-byte loads per lane; load p of lane (a = lane >> 4,
// b = lane >> 3 & 1, j = lane & 7) is the 16 codes c = j + 8 p of row 4 b + a of the group: the 16 lanes of a quarter wave read half
// a row of row a and the same half of row a + 4, 128 contiguous bytes each.  Widened, the 16 codes are the LDS chunks 2 c and 2 c + 1
// of the row, written by two ds_write_b128 (first every lane's chunk 2 c, then every lane's 2 c + 1).  Slots: were the 16 lanes one
// row, chunks 2 c, c = 0 .. 15, would have only the 8 even values of (chunk & 15) -- 2 c and 2 c + 16 share their low four bits --
// and the XOR with x(row) permutes slots without separating them: each round 2-way conflicted.  With two rows R and R + 4 to a
// quarter wave, the lanes of one row cover the 8 values 2 j ^ x(R), all of one parity, and x(R + 4) = x(R) ^ 1 (bit 2 of the row is
// bit 0 of x), so the other row's 8 slots are those of the other parity: 16 lanes, 16 slots, in the round of the even chunks and, by
// the same argument with 2 j + 1, in the round of the odd ones.  p adds 16 chunks (256 bytes) and g 32 rows: immediates.
__device__ __forceinline__ unsigned fp8_row(unsigned lane) { return ((lane >> 3) & 1u) * 4u + (lane >> 4); }
__device__ __forceinline__ unsigned fp8_ld_off(unsigned lane) { return fp8_row(lane) * kRowBytes8 + (lane & 7u) * 16u; }   // + 128 p
}  // namespace kv256

// Rows: the live rows of (sequence b, K/V head hkv) are (head hd < G of the group, token i < n_b), folded as p = hd * n_b + i into
// blocks of 32; workgroup (b, hkv, qb, sp) owns block qb and split sp, and lane (r, h) of EVERY wave owns row p = 32 qb + r.  A lane
// past the live rows loads Q from past the view (zeros), takes the limits of the last live row, so that it votes for a new reference
// maximum only where a live row votes, and stores nothing.  A workgroup whose block holds no live row returns before anything is
// read -- with n_b = 0 that is every workgroup of the sequence.
// Keys: row i sees [lo_i, c_i), c_i = L (causal: max(0, L - n_b + 1 + i)), lo_i = max(0, L - n_b + 1 + i - W).  No row sees a key
// below start_b = lo_0, so the splits deal out the tiles from start_t = start_b rounded down to a tile and nothing below it is
// touched.  A tile's rows come through one buffer descriptor per (wave, 8-row group), 64-bit base, ending at the split's last key:
// rows at or past it read as zeros whatever memory holds.  Eight aligned rows lie inside one page (>= 16 keys), so the page number
// is wave-uniform; the numbers of the tile after next are fetched while the current one computes, the entry index clamped into
// [page of start_b, the split's last live page].  A group wholly below start_b and a page number outside [0, num_pages) get a
// descriptor of zero records; the rows of the first tile below start_b are loaded and zeroed in their registers.  So every row no
// key of the split lies in reaches LDS as zeros: masking the score is not enough for V, because a weight of 0 times a NaN is a NaN
// in the PV MFMA.  Contiguous and paged kernels differ in the descriptor's base alone: the bits are the same.
// Tile loop, single-buffered: the next tile's 16 loads per lane are issued into registers before the arithmetic of the current one,
// and go to LDS between two barriers behind it; the second workgroup of the CU computes meanwhile.
// Soft-cap: the stream's arithmetic.  Before the masks every score x = s c (log2 units) becomes cap2 tanh(x / cap2), with tanh(y) =
// 1 - 2 / (1 + e^(2y)) on v_exp_f32 and v_rcp_f32; the scores are then final and the factor of the vote and of the weights is 1.
// cap2 == 0 skips it by a wave-uniform branch.
// kFp8: K and V address one e4m3fn byte per element.  Only the staging differs (above): the descriptors cover rows x 256 bytes, so
// what lies outside them reads as the code 0 (+0) whatever NaN codes memory holds; the raw bytes wait in 32 registers through the
// tile's arithmetic and are widened exactly to T (fp8x16_widen) in stage_write.  k_scale[hkv] joins the logit factor -- the clamp
// comes after the product, and under the soft-cap the product is what the cap sees -- and v_scale[hkv] joins 1 / l here and in
// the merge.  With both null every factor keeps its bits: the result is the 16-bit kernel's on the widened cache.
template <typename T, bool kOutF32, bool kPartial, bool kPaged, bool kFp8>
__global__ __launch_bounds__(64 * kv256::kW, 2)
void fa_kv256_decode_kernel(kv256::Dev a)
{
    using namespace kv256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned sp = blockIdx.x % (unsigned)a.S, rest = blockIdx.x / (unsigned)a.S;
    const unsigned qb = rest % (unsigned)a.nqb, bh = rest / (unsigned)a.nqb;
    const unsigned b = bh / (unsigned)a.Hkv, hkv = bh % (unsigned)a.Hkv;
    const unsigned tid = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u, r = lane & 31u, h = lane >> 5;

    // the sequence's rows (wave-uniform): fa_forward_varlen's clamps, cut to max_q
    int s_tok;
    unsigned n_q;
    packed_rows(a.cu_q, b, a.total_q, a.max_q, s_tok, n_q);
    const unsigned live = n_q * (unsigned)a.G;
    if (qb * (unsigned)kRows >= live) return;   // workgroup-uniform; nothing was read.  n_q >= 1 from here on
    const unsigned nkeys = a.seqlens ? (unsigned)min(max(a.seqlens[b], 0), a.cap) : (unsigned)a.cap;
    const int first = (int)nkeys - (int)n_q + 1;   // the causal limit of row 0; may be <= 0
    const unsigned start_b = (unsigned)max(first - a.window, 0), start_t = start_b & ~(unsigned)(kTile - 1);
    const unsigned chunk = (((nkeys - start_t + kTile - 1) / kTile + (unsigned)a.S - 1) / (unsigned)a.S) * kTile;
    const unsigned key0 = start_t + sp * chunk, key1 = min(nkeys, key0 + chunk);

    // the lane's row: token i of head hd of the group, in the (sequence, K/V head) view of Q
    const unsigned p_row = qb * (unsigned)kRows + r;
    const unsigned pc = min(p_row, live - 1u), row_hd = pc / n_q, row_i = pc - row_hd * n_q;
    unsigned qend;
    const __amdgpu_buffer_rsrc_t rq = packed_rsrc(a.Q, s_tok, n_q, hkv * (unsigned)a.G, (unsigned)a.G, a.q_st, a.q_sh, kD, 2u, qend);
    const unsigned qoff = p_row < live ? (row_i * (unsigned)a.q_st + row_hd * (unsigned)a.q_sh) * 2u : qend;

    // the row's causal limit before any clamp (both of its limits follow from it in the few tiles that mask); the smallest upper
    // and the largest lower limit of any row: tiles between them need no mask
    const int row_end = first + (int)row_i;
    const unsigned lim_lo = a.causal ? min((unsigned)max(first, 0), key1) : key1;
    const unsigned lo_hi = (unsigned)max((int)nkeys - a.window, 0);

    float sl2 = a.scale_log2e;
    if constexpr (kFp8) {
        if (a.k_scale) sl2 *= a.k_scale[hkv];
    }
    const float c = fmaxf(fabsf(sl2), 1.17549435e-38f);   // a scale of 0 must not meet a masked -inf as 0 * -inf
    const unsigned q_flip = a.scale_log2e < 0.0f ? 0x80008000u : 0u;
    // what a score is multiplied by on its way into the vote and the exponent (1 once the cap has made the scores final), and the
    // cap's two constants, in scalar registers
    const float cs = to_sgpr(a.cap2 > 0.0f ? 1.0f : c);
    const float cap_k1 = to_sgpr(c * a.cap_rk), cap_n2 = to_sgpr(-2.0f * a.cap2);
    u32x4 qf[kKSteps];
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) {
        u32x4 raw = buf_load16(rq, qoff + (16u * s + 8u * h) * 2u);
#pragma unroll
        for (int w = 0; w < 4; ++w) raw[w] ^= q_flip;
        qf[s] = raw;
    }

    // staging: group g of the tile's 8-row groups that this wave loads is group g * kW + wave; lane idx = lane + 64 p of a group is
    // chunk idx % 32 of row idx / 32, which in memory is byte idx * 16 of the group
    constexpr int kLoads = kFp8 ? kGroupLoads8 : kGroupLoads;
    constexpr unsigned kSrcRow = kFp8 ? kRowBytes8 : kRowBytes;   // bytes of a cache row
    unsigned l_off[kLoads];   // kFp8: [0] is chunk 2 j of the lane's row in the image (chunk 2 j + 1 lies at [0] ^ 16), [1] its load offset
    if constexpr (kFp8) {
        l_off[0] = img_off(wave * 8u + fp8_row(lane), 2u * (lane & 7u));
        l_off[1] = fp8_ld_off(lane);
    } else {
#pragma unroll
        for (int p = 0; p < kGroupLoads; ++p) l_off[p] = img_off(wave * 8u + 2u * p + h, r);   // swz has period 16: g adds 32 rows
    }
    const char *kbase = a.K, *vbase = a.V;
    if constexpr (!kPaged) {
        kbase += (size_t)bh * (unsigned)a.cap * kSrcRow;
        vbase += (size_t)bh * (unsigned)a.cap * kSrcRow;
    }
    u32x4 kst[kGroups][kLoads], vst[kGroups][kLoads];
    [[maybe_unused]] int pg[kGroups];
    [[maybe_unused]] auto fetch_pages = [&](unsigned kv0) {
        if constexpr (kPaged) {
            const int* tbl = a.table + (size_t)b * (unsigned)a.max_pages;
            const unsigned last = (key1 - 1u) >> a.lg_page;   // only called with key1 > key0; key1 > start_b
#pragma unroll
            for (int g = 0; g < kGroups; ++g) {
                const unsigned e = max(min((kv0 + (g * kW + wave) * 8u) >> a.lg_page, last), start_b >> a.lg_page);
                pg[g] = __builtin_amdgcn_readfirstlane(tbl[e]);
            }
        }
    };
    auto stage_load = [&](unsigned kv0) {
#pragma unroll
        for (int g = 0; g < kGroups; ++g) {
            const unsigned kg = kv0 + (g * kW + wave) * 8u;               // the group's first key
            unsigned rows = kg < key1 ? min(8u, key1 - kg) : 0u;          // its rows below the split's end
            if (kg + 8u <= start_b) rows = 0u;                            // wholly below the window: pg[g] is another page's
            size_t row0 = kg;                                             // the row of `kbase` the group starts at
            if constexpr (kPaged) {
                if ((unsigned)pg[g] >= (unsigned)a.num_pages) rows = 0u;  // a bad page number: no record, every load reads 0
                row0 = rows ? ((((size_t)(unsigned)pg[g] * (unsigned)a.Hkv + hkv) << a.lg_page) + (kg & ((1u << a.lg_page) - 1u))) : 0;
            }
            const size_t byte0 = (rows ? row0 : 0) * kSrcRow;
            const __amdgpu_buffer_rsrc_t rk = make_rsrc(kbase + byte0, rows * kSrcRow), rv = make_rsrc(vbase + byte0, rows * kSrcRow);
#pragma unroll
            for (int p = 0; p < kLoads; ++p) {
                const unsigned off = kFp8 ? l_off[1] + 128u * p : (lane + 64u * p) * 16u;
                kst[g][p] = buf_load16_nt(rk, off);
                vst[g][p] = buf_load16_nt(rv, off);
            }
        }
    };
    // kv0: the tile stage_load() was last called for
    auto stage_write = [&](unsigned kv0) {
        if (kv0 < start_b) {   // workgroup-uniform, one tile per sequence: rows below the window go to LDS as zeros
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
#pragma unroll
                for (int p = 0; p < kLoads; ++p) {
                    if constexpr (kFp8) {   // the raw bytes: the code 0 is +0
                        if (kv0 + (g * kW + wave) * 8u + fp8_row(lane) < start_b) kst[g][p] = vst[g][p] = u32x4{0u, 0u, 0u, 0u};
                    } else {
                        if (kv0 + (g * kW + wave) * 8u + 2u * p + h < start_b) kst[g][p] = vst[g][p] = u32x4{0u, 0u, 0u, 0u};
                    }
                }
        }
#pragma unroll
        for (int g = 0; g < kGroups; ++g)
#pragma unroll
            for (int p = 0; p < kLoads; ++p) {
                if constexpr (kFp8) {   // one load is the row's chunks 2 c and 2 c + 1, c = j + 8 p: the even round, then the odd one
                    const unsigned at = g * (kW * 8 * kRowBytes) + p * 256u;
                    u32x4 klo, khi, vlo, vhi;
                    fp8x16_widen<T>(kst[g][p], klo, khi);
                    fp8x16_widen<T>(vst[g][p], vlo, vhi);
                    lds_write16(smem, at + l_off[0], klo);
                    lds_write16(smem, at + (l_off[0] ^ 16u), khi);   // `at` is a multiple of 256
                    lds_write16(smem, kImgBytes + at + l_off[0], vlo);
                    lds_write16(smem, kImgBytes + at + (l_off[0] ^ 16u), vhi);
                } else {
                    lds_write16(smem, g * (kW * 8 * kRowBytes) + l_off[p], kst[g][p]);
                    lds_write16(smem, kImgBytes + g * (kW * 8 * kRowBytes) + l_off[p], vst[g][p]);
                }
            }
    };

    // row reads of S^T = K Q^T: lane (r, h) takes chunk 2 ks + h of key kb * 32 + r.  (2 ks + h) ^ x = 2 (ks % 8) ^ (h ^ x) in the
    // low four bits, so one register holds the address and a step XORs (ks % 8) << 5 into it; ks / 8 and kb are immediates
    const unsigned k_rd = r * kRowBytes + ((h ^ swz(r)) << 4);
    // transposed reads of O^T += V^T P^T: lane 4 vq + vp of a 16-lane group supplies row vq, columns 4 vp .. 4 vp + 3 of the block of
    // keys 16 q4 + 8 jj + 4 h .. + 3 and columns 64 wave + 32 db + 16 vg .. + 15; the block's two chunks are looked up one by one
    const unsigned i16 = lane & 15u, vq = i16 >> 2, vp = i16 & 3u, vg = (lane >> 4) & 1u;
    unsigned v_rd[2][kDBlocks];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int db = 0; db < kDBlocks; ++db)
            v_rd[jj][db] = kImgBytes + img_off(8u * jj + 4u * h + vq, 8u * wave + 4u * db + 2u * vg + (vp >> 1)) + (vp & 1u) * 8u;

    f32x16 o[kDBlocks];
    f32x16 zero16;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero16[i] = 0.0f;
#pragma unroll
    for (int db = 0; db < kDBlocks; ++db) o[db] = zero16;
    float m_ref = -INFINITY, l_part = 0.0f;

    // 0 for a split that lies past the sequence's last key: it touches no table entry and no K/V row
    const int ntiles = key0 >= nkeys ? 0 : (int)((key1 - key0 + kTile - 1) / kTile);
    if (ntiles > 0) {   // workgroup-uniform
        fetch_pages(key0);
        stage_load(key0);
        fetch_pages(key0 + (unsigned)min(1, ntiles - 1) * kTile);
        stage_write(key0);
        __syncthreads();
    }
    for (int t = 0; t < ntiles; ++t) {
        const unsigned kv0 = key0 + (unsigned)t * kTile;
        if (t + 1 < ntiles) stage_load(kv0 + kTile);
        fetch_pages(key0 + (unsigned)min(t + 2, ntiles - 1) * kTile);   // a last tile re-reads its own entries

        f32x16 s[2];
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks)   // consecutive MFMAs alternate accumulators
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const u32x4 kf = lds_read16(smem, (k_rd ^ ((unsigned)(ks & 7) << 5)) + (unsigned)(ks >> 3) * 256u + kb * 32u * kRowBytes);
                s[kb] = T::mfma32(kf, qf[ks], ks == 0 ? zero16 : s[kb]);
            }
        if constexpr (kFp8) {
            // The order of the 32 row reads and their MFMAs, pinned: four reads ahead, then one read per MFMA.  Left to itself the
            // scheduler spends the 32 freed staging registers on 16 reads in flight in the partial kernels and spills a Q fragment
            // for it (4 VGPRs of scratch); the direct kernels come out read-by-read either way.  0x100: DS read, 0x008: MFMA.
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
            for (int i = 0; i < 2 * kKSteps - 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        if (a.cap2 > 0.0f) {   // wave-uniform; before the masks, so a masked key stays at -inf
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    s[kb][i] = __builtin_fmaf(cap_n2, __builtin_amdgcn_rcpf(1.0f + fast_exp2(s[kb][i] * cap_k1)), a.cap2);
        }
        // keys outside [lo, hi) -> -inf: one unsigned compare per score, in the tiles that reach past the smallest upper limit or
        // start below the largest lower one
        if (kv0 + kTile > lim_lo || kv0 < lo_hi) {
            const unsigned lo = (unsigned)max(row_end - a.window, 0);
            const unsigned hi = a.causal ? min((unsigned)max(row_end, 0), key1) : key1;
            const unsigned seen = hi > lo ? hi - lo : 0u;   // a split that ends below lo: nothing
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned key = kv0 + (unsigned)(kb * 32 + (i & 3) + 8 * (i >> 2)) + 4u * h;
                    if (key - lo >= seen) s[kb][i] = -INFINITY;
                }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int e = 0; e < 32; e += 2) tmax = max3(tmax, s[e >> 4][e & 15], s[(e + 1) >> 4][(e + 1) & 15]);
        tmax *= cs;
        // the lazy reference maximum of the split stream: m_ref stays at -inf until the row meets a key, moves only when some row's
        // tile maximum exceeds it by more than kThr (P <= 2^8 fits fp16), and a row at -inf takes alpha = 0
        if (__any(tmax > m_ref + kThr)) {
            const float mx = fmaxf(tmax, swap_halves(tmax));
            const float m_new = fmaxf(mx, m_ref);
            const float alpha = m_ref == -INFINITY ? 0.0f : fast_exp2(m_ref - m_new);
            m_ref = m_new;
#pragma unroll
            for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
            l_part *= alpha;
        }
        u32x4 pk[4];
        float ls0 = 0.0f, ls1 = 0.0f;
        const float neg_m = m_ref == -INFINITY ? 0.0f : -m_ref;   // every s of such a row is -inf: p = 2^(-inf + 0) = 0
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int kb = q4 >> 1, b8 = (q4 & 1) * 8;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float p0 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w], cs, neg_m));
                const float p1 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w + 1], cs, neg_m));
                pk[q4][w] = T::pack2(p0, p1);
                if (w & 1) ls1 = T::sum2(pk[q4][w], ls1);   // sums of the ROUNDED weights (fa_common.hpp)
                else ls0 = T::sum2(pk[q4][w], ls0);
            }
        }
        l_part += ls0 + ls1;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
            for (int db = 0; db < kDBlocks; ++db) {
                u32x4 vf;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const u32x2 half = lds_read_tr8(smem, q4 * 16u * kRowBytes + v_rd[jj][db]);
                    vf[2 * jj] = half[0];
                    vf[2 * jj + 1] = half[1];
                }
                o[db] = T::mfma32(vf, pk[q4], o[db]);
            }
        if (t + 1 < ntiles) {   // workgroup-uniform: every wave has read the tile, then the next one lands
            __syncthreads();
            stage_write(kv0 + kTile);
            __syncthreads();
        }
    }

    const float l = l_part + swap_halves(l_part);
    const bool row_live = p_row < live;
    if constexpr (kPartial) {
        // workspace row ((b, hkv, sp), p): 256 floats of O^T (unnormalised), then m (log2 units), then l.  The workspace holds
        // nqb * 32 rows per (b, hkv, sp); only the live ones are written, and only those are read (one token per sequence leaves
        // G of the block's 32 rows live: the dead rows would be most of the partials' traffic)
        float* row = a.ws + (((size_t)bh * (unsigned)a.S + sp) * ((size_t)a.nqb * kRows) + p_row) * kWsRow;
        if (row_live) {
#pragma unroll
            for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned col = (wave * kDBlocks + db) * 32u + 8u * g + 4u * h;
                    const f32x4 v = {o[db][4 * g], o[db][4 * g + 1], o[db][4 * g + 2], o[db][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(row + col) = v;
                }
            if (h == 0 && wave == 0) *reinterpret_cast<f32x2*>(row + kD) = f32x2{m_ref, l};
        }
    } else {
        float inv = l == 0.0f ? 0.0f : 1.0f / l;   // a row without a key: O = 0
        if constexpr (kFp8) {
            if (a.v_scale) inv *= a.v_scale[hkv];
        }
        if (a.lse && h == 0 && wave == 0 && row_live)
            a.lse[((size_t)hkv * (unsigned)a.G + row_hd) * (size_t)a.total_q + (size_t)s_tok + row_i] =
                l == 0.0f ? -INFINITY : (m_ref + __log2f(l)) * kLn2;
        constexpr unsigned es = kOutF32 ? 4u : 2u;
        unsigned oend;
        const __amdgpu_buffer_rsrc_t ro = packed_rsrc(a.O, s_tok, n_q, hkv * (unsigned)a.G, (unsigned)a.G, a.o_st, a.o_sh, kD, es, oend);
        const unsigned ooff = row_live ? (row_i * (unsigned)a.o_st + row_hd * (unsigned)a.o_sh) * es : oend;
#pragma unroll
        for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned col = (wave * kDBlocks + db) * 32u + 8u * g + 4u * h;
                const float x0 = o[db][4 * g] * inv, x1 = o[db][4 * g + 1] * inv, x2 = o[db][4 * g + 2] * inv, x3 = o[db][4 * g + 3] * inv;
                if constexpr (kOutF32) {
                    const f32x4 v = {x0, x1, x2, x3};
                    buf_store16(ro, ooff + col * 4u, __builtin_bit_cast(u32x4, v));
                } else {
                    buf_store8(ro, ooff + col * 2u, u32x2{T::pack2(x0, x1), T::pack2(x2, x3)});
                }
            }
    }
}

// The merge behind a split: one wave per padded row (b, hkv, head hd of the group, token i < max_q), a lane per 4 output columns.
// A row with i >= n_b returns without writing: no token of no sequence is written.  A partial with m = -inf (a split without a
// visible key) takes the weight 0; a row of such partials is O = 0, lse = -inf.  kFp8: v_scale[hkv] joins the final division.
template <typename T, bool kOutF32, bool kFp8>
__global__ __launch_bounds__(64)
void fa_kv256_merge_kernel(kv256::Dev a)
{
    using namespace kv256;
    const unsigned per_head = (unsigned)a.G * (unsigned)a.max_q;
    const unsigned bh = blockIdx.x / per_head, p = blockIdx.x % per_head;
    const unsigned b = bh / (unsigned)a.Hkv, hkv = bh % (unsigned)a.Hkv;
    const unsigned hd = p / (unsigned)a.max_q, i = p % (unsigned)a.max_q;
    int s_tok;
    unsigned n_q;
    packed_rows(a.cu_q, b, a.total_q, a.max_q, s_tok, n_q);
    if (i >= n_q) return;
    const size_t stride_s = (size_t)a.nqb * kRows * kWsRow;
    const float* base = a.ws + (size_t)bh * (unsigned)a.S * stride_s + (size_t)(hd * n_q + i) * kWsRow;
    float M = -INFINITY;
    for (int s = 0; s < a.S; ++s) M = fmaxf(M, base[(size_t)s * stride_s + kD]);
    float L = 0.0f;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const unsigned c4 = threadIdx.x * 4u;
#pragma unroll 4
    for (int s = 0; s < a.S; ++s) {
        const float* row = base + (size_t)s * stride_s;
        const float m = row[kD];
        const float w = m == -INFINITY ? 0.0f : fast_exp2(m - M);
        L += row[kD + 1] * w;
        acc += *reinterpret_cast<const f32x4*>(row + c4) * w;
    }
    float inv = L == 0.0f ? 0.0f : 1.0f / L;
    if constexpr (kFp8) {
        if (a.v_scale) inv *= a.v_scale[hkv];
    }
    const size_t tok = (size_t)s_tok + i, hq = (size_t)hkv * (unsigned)a.G + hd;
    if (a.lse && threadIdx.x == 0) a.lse[hq * (size_t)a.total_q + tok] = L == 0.0f ? -INFINITY : (M + __log2f(L)) * kLn2;
    const size_t off = tok * (size_t)a.o_st + hq * (size_t)a.o_sh + c4;
    if constexpr (kOutF32) {
        *reinterpret_cast<f32x4*>(static_cast<float*>(a.O) + off) = acc * inv;
    } else {
        *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(a.O) + off) = u32x2{T::pack2(acc[0] * inv, acc[1] * inv), T::pack2(acc[2] * inv, acc[3] * inv)};
    }
}

// The one or two launches of a checked call.
template <typename T, bool kOutF32, bool kFp8>
hipError_t kv256_launch(const kv256::Dev& a, bool paged, hipStream_t stream)
{
    const dim3 grid((unsigned)a.B * (unsigned)a.Hkv * (unsigned)a.nqb * (unsigned)a.S), block(64 * kv256::kW);
    void (*kernel)(kv256::Dev);
    if (a.S > 1) kernel = paged ? fa_kv256_decode_kernel<T, kOutF32, true, true, kFp8> : fa_kv256_decode_kernel<T, kOutF32, true, false, kFp8>;
    else kernel = paged ? fa_kv256_decode_kernel<T, kOutF32, false, true, kFp8> : fa_kv256_decode_kernel<T, kOutF32, false, false, kFp8>;
    FA_LAUNCH(kernel, grid, block, (size_t)kv256::kLdsBytes, stream, a);   // 64 KiB: the default limit of dynamic LDS
    const hipError_t e = launch_status();
    if (e != hipSuccess || a.S <= 1) return e;
    FA_LAUNCH((fa_kv256_merge_kernel<T, kOutF32, kFp8>), dim3((unsigned)a.B * (unsigned)a.Hkv * (unsigned)a.G * (unsigned)a.max_q), dim3(64), 0,
              stream, a);
    return launch_status();
}
// fa_fwd_kv256_fp8.hip: kv256_launch<., ., true>, the fp8 unit's instantiations behind the checks and the plan of fa_fwd_kv256.hip
hipError_t kv256_launch_fp8(const kv256::Dev& a, bool bf16, bool f32, bool paged, hipStream_t stream);

}  // namespace fa
