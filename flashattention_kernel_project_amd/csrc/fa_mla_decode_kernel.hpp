// fa_mla_decode_kernel.hpp -- device code of the MLA decode entries: the kernel template of fa_mla_decode (fa_mla_decode.hip, 16-bit
// latent cache) and of fa_mla_decode_fp8 (fa_mla_decode_fp8.hip, kFp8: rows of 576 e4m3fn codes and one scale), the merge kernel
// behind a split, and the launcher both units instantiate.  One row per token serves all Hq heads: the logits run over the whole row,
// the output over its first 512 elements.  A kernel of its own on the plan of the split-KV stream (fa_fwd_split_kernel.hpp): the Hq
// heads of a sequence's tokens are folded into the rows of a workgroup, lengths, cu_seqlens and the block table are read on the device,
// the 64-key tiles of a sequence are dealt to S splits, and a private merge kernel finishes behind a split.  What is new is the tile:
// ONE row-major LDS image of [keys][576] is read by rows for S^T = C Q^T and through ds_read_b64_tr_b16 on its first 512 columns for
// O^T += V^T P^T.  Everything kFp8 adds sits behind `if constexpr (kFp8)`: the 16-bit instantiations keep their code.  Private to
// csrc/.  DESIGN.md sections 7.22 and 7.24, profiles/mla_decode.txt, profiles/mla_decode_fp8.txt.
#pragma once
#include "../../include/fa_mi355.h"
#include "fa_dispatch.hpp"
#include "fa_fwd_split_kernel.hpp"   // fp8x2_widen

namespace fa {

namespace mla {
constexpr int kDqk = FA_MLA_DQK, kDv = FA_MLA_DC;
constexpr int kW = 4;                    // waves per workgroup
constexpr int kRowBytes = kDqk * 2;      // 1152: one latent row in LDS, and in memory for a 16-bit cache
constexpr int kRowBytes8 = kDqk;         // 576: one latent row of an fp8 cache in memory
constexpr int kChunks = kDqk / 8;        // 72 16-byte chunks per row
constexpr int kKSteps = kDqk / 16;       // 36 steps of the 32x32x16 instruction over the reduction dimension of S^T
constexpr int kSplitTile = 64;           // the unit the splits deal out, whatever the LDS tile is
constexpr int kWsRow = kDv + 4;          // floats per workspace row: O^T, m, l and two of padding (rows stay 16-byte aligned)
#ifndef FA_MLA_ROW_BLOCKS
#define FA_MLA_ROW_BLOCKS 2              // 32-row blocks per workgroup; the other 4 / FA_MLA_ROW_BLOCKS waves of a block split the 512 columns
#endif
#ifndef FA_MLA_TILE
#define FA_MLA_TILE 32                   // keys per LDS tile: 32 (two buffers of 36 KiB), or 64 (72 KiB each; spills)
#endif
constexpr int kRB = FA_MLA_ROW_BLOCKS, kDS = kW / kRB;
constexpr int kRows = 32 * kRB;          // query rows per workgroup
constexpr int kTile = FA_MLA_TILE;
constexpr int kDBlocks = kDv / 32 / kDS; // 32-column blocks of O^T per wave
constexpr int kGroups = kTile / 8 / kW;  // 8-row groups of a tile each wave stages
constexpr int kGroupLoads = 8 * kChunks / 64;   // 9 loads per lane and group: 16 bytes each, 8 bytes each of an fp8 cache
constexpr int kTileBytes = kTile * kRowBytes;
constexpr int kLdsBytes = 2 * kTileBytes;
static_assert(kRB * kDS == kW && kGroups >= 1 && kSplitTile % kTile == 0, "geometry");

// The LDS image: row-major rows of 1152 bytes; inside every aligned group of eight 16-byte chunks the chunk index is XORed with a
// value of the row.  1152 = 4 * 256 + 128, so consecutive rows start half a bank row apart: with x(row) below, the 16 rows one lane
// group of a ds_read_b128 row read takes (same chunk) fall into 16 different slots, and so do the 4 rows x 4 chunks a 32-lane half
// of a ds_read_b64_tr_b16 takes (rows 4n .. 4n+3: the row pairs differ in x's bit 2, the rows of a pair in the half bank row).
__device__ __forceinline__ unsigned swz(unsigned row) { return (((row >> 1) & 1u) << 2) | ((row >> 2) & 3u); }
__device__ __forceinline__ unsigned img_off(unsigned row, unsigned chunk)
{
    return row * kRowBytes + (((chunk & ~7u) | ((chunk & 7u) ^ swz(row))) << 4);
}

struct Dev {
    const uint16_t* Q;
    void* O;
    float* lse;
    const char* C;
    float* ws;
    const int *cu_q, *seqlens, *table;
    int B, Hq, total_q, max_q, cap;
    int max_pages, num_pages, lg_page;   // paged only
    long long q_st, q_sh, o_st, o_sh;    // elements
    float scale_log2e;
    int causal, S, nqb;
    const float* c_scale;                // kFp8 only: the cache's one scale on the device, or nullptr (1.0)
};

// eight raw bytes of a read-once stream (buf_load16_nt's hint on the 64-bit load)
__device__ __forceinline__ u32x2 buf_load8_nt(__amdgpu_buffer_rsrc_t r, unsigned voff)
{
    return __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, 2);
}
// the staged registers of one load: a 16-byte chunk of T, or the 8 codes that become one
template <bool kFp8> struct Staged { using type = u32x4; };
template <> struct Staged<true> { using type = u32x2; };
}  // namespace mla

constexpr float kMlaLn2 = 0.6931471805599453f;

// Rows: the live rows of sequence b are (token i, head hd), i < n_b, folded as p = i * Hq + hd into row blocks of kRows; workgroup
// (b, qb, sp) owns block qb and split sp.  A wave owns 32 rows (lane & 31) and, with kDS = 2, one half of the 512 output columns: the
// two waves of a row block compute the same S^T and the same (m, l) from the same LDS bytes and differ in the V columns they take.
// A lane past the live rows loads Q from past the view (zeros), takes the limit of the last live row, so that it votes for a new
// reference maximum only where a live row votes, and stores nothing.
// Keys: the tile's rows come through one buffer descriptor per (wave, 8-row group), 64-bit base, ending at the split's last key: rows
// at or past it read as zeros whatever memory holds.  Eight aligned rows lie inside one page (>= 16 keys), so the page number is
// wave-uniform; the numbers of the tile after next are fetched while the current one computes, with the entry index clamped to the
// split's last live page.  Contiguous and paged kernels differ in that base alone: the bits are the same.
// kFp8: a row in memory is 576 codes.  The group's descriptor has a record of rows * 576 bytes and the lane's nine loads are EIGHT
// bytes each under the same index map -- load idx = lane + 64 p is chunk idx % 72 of row idx / 72, at byte idx * 8 of the group -- so
// a zero byte (the code of +0) stands where the 16-bit kernel reads a zero element, and the NaN codes of a dead row or a freed page
// lie outside the record.  The raw bytes are carried across the tile's arithmetic (18 registers, not 36) and widened exactly to T in
// stage_write(): the LDS image and everything that reads it are the 16-bit kernel's.  The cache's scale is read once per workgroup;
// it joins the logit factor (clamped after the product, its sign into the Q flip) and 1 / l in the epilogue.
template <typename T, bool kOutF32, bool kPartial, bool kPaged, bool kFp8>
__global__ __launch_bounds__(64 * mla::kW, 1)
void fa_mla_decode_kernel(mla::Dev a)
{
    using namespace mla;
    constexpr unsigned kMemRow = kFp8 ? kRowBytes8 : kRowBytes;   // a row's bytes in memory
    constexpr unsigned kLoadBytes = kFp8 ? 8u : 16u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned sp = blockIdx.x % (unsigned)a.S, rest = blockIdx.x / (unsigned)a.S;
    const unsigned qb = rest % (unsigned)a.nqb, b = rest / (unsigned)a.nqb;
    const unsigned tid = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const unsigned rb = wave / (unsigned)kDS, dh = wave % (unsigned)kDS;

    // the sequence's rows (wave-uniform): fa_forward_varlen's clamps, cut to max_q
    const int s_tok = min(max(a.cu_q[b], 0), a.total_q);
    const unsigned n_q = (unsigned)min(min(max(a.cu_q[b + 1], s_tok), a.total_q) - s_tok, a.max_q);
    const unsigned live = n_q * (unsigned)a.Hq;
    if (qb * (unsigned)kRows >= live) return;   // workgroup-uniform: no live row here (n_b = 0: the whole sequence); nothing was read
    const unsigned nkeys = a.seqlens ? (unsigned)min(max(a.seqlens[b], 0), a.cap) : (unsigned)a.cap;
    const unsigned chunk = (((nkeys + kSplitTile - 1) / kSplitTile + (unsigned)a.S - 1) / (unsigned)a.S) * kSplitTile;
    const unsigned key0 = sp * chunk, key1 = min(nkeys, key0 + chunk);

    // the lane's row: token i, head hd of the sequence's view of Q
    const unsigned p_row = qb * (unsigned)kRows + rb * 32u + r;
    const bool has_rows = qb * (unsigned)kRows + rb * 32u < live;   // wave-uniform
    const unsigned pc = min(p_row, live - 1u), row_i = pc / (unsigned)a.Hq, row_hd = pc - row_i * (unsigned)a.Hq;
    const unsigned qend = (unsigned)((unsigned long long)((long long)(n_q - 1) * a.q_st + (long long)(a.Hq - 1) * a.q_sh + kDqk) * 2u);
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(a.Q + (long long)s_tok * a.q_st, qend);
    const unsigned qoff = p_row < live ? (row_i * (unsigned)a.q_st + row_hd * (unsigned)a.q_sh) * 2u : qend;

    // first key the row does NOT see, and the smallest such limit of any row of the sequence
    unsigned lim = key1, lim_lo = key1;
    if (a.causal) {
        const int first = (int)nkeys - (int)n_q + 1;
        lim = min((unsigned)max(first + (int)row_i, 0), key1);
        lim_lo = min((unsigned)max(first, 0), key1);
    }
    // kFp8: the cache's scale (wave-uniform, kept in a scalar register), and the factor of the logits with it
    [[maybe_unused]] float cs = 1.0f;
    float sl2 = a.scale_log2e;
    if constexpr (kFp8) {
        cs = to_sgpr(a.c_scale ? *a.c_scale : 1.0f);
        sl2 *= cs;
    }
    const float c = fmaxf(fabsf(sl2), 1.17549435e-38f);   // a scale of 0 must not meet a masked -inf as 0 * -inf
    const unsigned q_flip = sl2 < 0.0f ? 0x80008000u : 0u;
    u32x4 qf[kKSteps];
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) {
        u32x4 raw = buf_load16(rq, qoff + (16u * s + 8u * h) * 2u);
#pragma unroll
        for (int w = 0; w < 4; ++w) raw[w] ^= q_flip;
        qf[s] = raw;
    }

    // staging: group g of the tile's 8-row groups that this wave loads is group g * kW + wave; lane idx = lane + 64 p of a group is
    // chunk idx % 72 of row idx / 72, which in memory is byte idx * 16 of the group (kFp8: byte idx * 8)
    unsigned l_off[kGroupLoads];
#pragma unroll
    for (int p = 0; p < kGroupLoads; ++p) {
        const unsigned idx = lane + 64u * p;
        l_off[p] = img_off(wave * 8u + idx / (unsigned)kChunks, idx % (unsigned)kChunks);   // swz repeats every 16 rows: g adds 32 rows
    }
    const char* cbase = a.C;
    if constexpr (!kPaged) cbase += (size_t)b * (unsigned)a.cap * kMemRow;
    typename Staged<kFp8>::type st[kGroups][kGroupLoads];
    [[maybe_unused]] int pg[kGroups];
    [[maybe_unused]] auto fetch_pages = [&](unsigned kv0) {
        if constexpr (kPaged) {
            const int* tbl = a.table + (size_t)b * (unsigned)a.max_pages;
            const unsigned last = (key1 - 1u) >> a.lg_page;   // only called with key1 > key0
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
                pg[g] = __builtin_amdgcn_readfirstlane(tbl[min((kv0 + (g * kW + wave) * 8u) >> a.lg_page, last)]);
        }
    };
    auto stage_load = [&](unsigned kv0) {
#pragma unroll
        for (int g = 0; g < kGroups; ++g) {
            const unsigned kg = kv0 + (g * kW + wave) * 8u;               // the group's first key
            unsigned rows = kg < key1 ? min(8u, key1 - kg) : 0u;          // its rows below the split's end
            size_t first = kg;                                            // the row of `cbase` the group starts at
            if constexpr (kPaged) {
                if ((unsigned)pg[g] >= (unsigned)a.num_pages) rows = 0u;  // a bad page number: no record, every load reads 0
                first = rows ? ((size_t)(unsigned)pg[g] << a.lg_page) + (kg & ((1u << a.lg_page) - 1u)) : 0;
            }
            const __amdgpu_buffer_rsrc_t rc = make_rsrc(cbase + (rows ? first : 0) * kMemRow, rows * kMemRow);
#pragma unroll
            for (int p = 0; p < kGroupLoads; ++p) {
                if constexpr (kFp8) st[g][p] = buf_load8_nt(rc, (lane + 64u * p) * kLoadBytes);
                else st[g][p] = buf_load16_nt(rc, (lane + 64u * p) * kLoadBytes);
            }
        }
    };
    auto stage_write = [&](unsigned buf) {
#pragma unroll
        for (int g = 0; g < kGroups; ++g)
#pragma unroll
            for (int p = 0; p < kGroupLoads; ++p) {
                if constexpr (kFp8) {   // the 8 codes become the chunk's 8 elements of T (fp8x2_widen, exact)
                    const u32x2 raw = st[g][p];
                    const u32x4 wide = {fp8x2_widen<T, false>(raw[0]), fp8x2_widen<T, true>(raw[0]), fp8x2_widen<T, false>(raw[1]),
                                        fp8x2_widen<T, true>(raw[1])};
                    lds_write16(smem, buf * kTileBytes + g * (kW * 8 * kRowBytes) + l_off[p], wide);
                } else {
                    lds_write16(smem, buf * kTileBytes + g * (kW * 8 * kRowBytes) + l_off[p], st[g][p]);
                }
            }
    };

    // row reads of S^T = C Q^T: lane (r, h) takes chunk 2 ks + h of key kb * 32 + r; the XOR touches the chunk's low three bits
    unsigned k_rd[4];
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) k_rd[k4] = r * kRowBytes + (((2u * k4 + h) ^ swz(r)) << 4);
    // transposed reads of O^T += V^T P^T: lane 4 vq + vp of a 16-lane group supplies row vq, columns 4 vp .. 4 vp + 3 of the block of
    // keys 16 q4 + 8 jj + 4 h .. + 3 and columns 32 db + 16 vg .. + 15; the block's two chunks are looked up one by one, since the XOR
    // may swap them
    const unsigned i16 = lane & 15u, vq = i16 >> 2, vp = i16 & 3u, vg = (lane >> 4) & 1u;
    unsigned v_rd[2][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            const unsigned row = 8u * jj + 4u * h + vq;
            v_rd[jj][par] = row * kRowBytes + (((4u * par + 2u * vg + (vp >> 1)) ^ swz(row)) << 4) + (vp & 1u) * 8u +
                            dh * (unsigned)(kDBlocks * 64);
        }

    f32x16 o[kDBlocks];
    f32x16 zero16;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero16[i] = 0.0f;
#pragma unroll
    for (int db = 0; db < kDBlocks; ++db) o[db] = zero16;
    float m_ref = -INFINITY, l_part = 0.0f;

    // 0 for a split that lies past the sequence's last key: it touches no table entry and no cache row
    const int ntiles = key0 >= nkeys ? 0 : (int)((key1 - key0 + kTile - 1) / kTile);
    if (ntiles > 0) {   // workgroup-uniform
        fetch_pages(key0);
        stage_load(key0);
        fetch_pages(key0 + (unsigned)min(1, ntiles - 1) * kTile);
        stage_write(0);
        __syncthreads();
    }
    for (int t = 0; t < ntiles; ++t) {
        const unsigned cur = t & 1u;
        const char* kbuf = smem + cur * kTileBytes;
        const unsigned kv0 = key0 + (unsigned)t * kTile;
        if (t + 1 < ntiles) stage_load(kv0 + kTile);
        fetch_pages(key0 + (unsigned)min(t + 2, ntiles - 1) * kTile);   // a last tile re-reads its own entries

        if (has_rows) {   // a wave without a live row only stages
            constexpr int kKB = kTile / 32;
            f32x16 s[kKB];
#pragma unroll
            for (int ks = 0; ks < kKSteps; ++ks)
#pragma unroll
                for (int kb = 0; kb < kKB; ++kb) {
                    const u32x4 kf = lds_read16(kbuf, kb * 32u * kRowBytes + (unsigned)(ks >> 2) * 128u + k_rd[ks & 3]);
                    s[kb] = T::mfma32(kf, qf[ks], ks == 0 ? zero16 : s[kb]);
                }
            if (kv0 + kTile > lim_lo) {   // keys past the row's limit (without causal: past the split's end) -> -inf
#pragma unroll
                for (int kb = 0; kb < kKB; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const unsigned key = kv0 + (unsigned)(kb * 32 + (i & 3) + 8 * (i >> 2)) + 4u * h;
                        if (key >= lim) s[kb][i] = -INFINITY;
                    }
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < kKB; ++kb)
#pragma unroll
                for (int e = 0; e < 16; e += 2) tmax = max3(tmax, s[kb][e], s[kb][e + 1]);
            tmax *= c;
            // the lazy reference maximum of the split stream: m_ref stays at -inf until the row meets a key, moves only when some
            // row's tile maximum exceeds it by more than kThr (P <= 2^8 fits fp16), and a row at -inf takes alpha = 0
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
            u32x4 pk[2 * kKB];
            float ls0 = 0.0f, ls1 = 0.0f;
            const float neg_m = m_ref == -INFINITY ? 0.0f : -m_ref;   // every s of such a row is -inf: p = 2^(-inf + 0) = 0
#pragma unroll
            for (int q4 = 0; q4 < 2 * kKB; ++q4) {
                const int kb = q4 >> 1, b8 = (q4 & 1) * 8;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const float p0 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w], c, neg_m));
                    const float p1 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w + 1], c, neg_m));
                    pk[q4][w] = T::pack2(p0, p1);
                    if (w & 1) ls1 = T::sum2(pk[q4][w], ls1);   // sums of the ROUNDED weights (fa_common.hpp)
                    else ls0 = T::sum2(pk[q4][w], ls0);
                }
            }
            l_part += ls0 + ls1;
#pragma unroll
            for (int q4 = 0; q4 < 2 * kKB; ++q4)
#pragma unroll
                for (int db = 0; db < kDBlocks; ++db) {
                    u32x4 vf;
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const u32x2 half = lds_read_tr8(kbuf, q4 * 16u * kRowBytes + (unsigned)(db >> 1) * 128u + v_rd[jj][db & 1]);
                        vf[2 * jj] = half[0];
                        vf[2 * jj + 1] = half[1];
                    }
                    o[db] = T::mfma32(vf, pk[q4], o[db]);
                }
        }
        if (t + 1 < ntiles) stage_write(cur ^ 1u);
        __syncthreads();
    }

    const float l = l_part + swap_halves(l_part);
    if constexpr (kPartial) {
        // workspace row ((b, sp), p): 512 floats of O^T (unnormalised), then m (log2 units), then l; dead rows of the block are
        // written too (the workspace holds nqb * kRows rows per (b, sp)) and never read
        float* row = a.ws + (((size_t)b * (unsigned)a.S + sp) * ((size_t)a.nqb * kRows) + p_row) * kWsRow;
        if (has_rows) {
#pragma unroll
            for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned col = (dh * kDBlocks + db) * 32u + 8u * g + 4u * h;
                    const f32x4 v = {o[db][4 * g], o[db][4 * g + 1], o[db][4 * g + 2], o[db][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(row + col) = v;
                }
            if (h == 0 && dh == 0) *reinterpret_cast<f32x2*>(row + kDv) = f32x2{m_ref, l};
        }
    } else {
        float inv = l == 0.0f ? 0.0f : 1.0f / l;   // a row without a key: O = 0
        if constexpr (kFp8) inv *= cs;             // O = c_scale * sum p code / l
        const bool row_live = p_row < live;
        if (a.lse && h == 0 && dh == 0 && row_live)
            a.lse[(size_t)row_hd * (size_t)a.total_q + (size_t)s_tok + row_i] = l == 0.0f ? -INFINITY : (m_ref + __log2f(l)) * kMlaLn2;
        constexpr unsigned es = kOutF32 ? 4u : 2u;
        const unsigned oend = (unsigned)((unsigned long long)((long long)(n_q - 1) * a.o_st + (long long)(a.Hq - 1) * a.o_sh + kDv) * es);
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(a.O) + (long long)s_tok * a.o_st * (long long)es, oend);
        const unsigned ooff = row_live ? (row_i * (unsigned)a.o_st + row_hd * (unsigned)a.o_sh) * es : oend;
#pragma unroll
        for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned col = (dh * kDBlocks + db) * 32u + 8u * g + 4u * h;
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

// The merge behind a split: one workgroup of 128 threads per padded row (b, token i < max_q, head hd), a thread per 4 output columns.
// A row with i >= n_b returns without writing: no token of no sequence is written.  A partial with m = -inf (a split without a
// visible key) takes the weight 0; a row of such partials is O = 0, lse = -inf.  kFp8: the cache's scale joins 1 / L.
template <typename T, bool kOutF32, bool kFp8>
__global__ __launch_bounds__(128)
void fa_mla_merge_kernel(mla::Dev a)
{
    using namespace mla;
    const unsigned per_seq = (unsigned)a.max_q * (unsigned)a.Hq;
    const unsigned b = blockIdx.x / per_seq, p = blockIdx.x % per_seq;
    const unsigned i = p / (unsigned)a.Hq, hd = p - i * (unsigned)a.Hq;
    const int s_tok = min(max(a.cu_q[b], 0), a.total_q);
    const unsigned n_q = (unsigned)min(min(max(a.cu_q[b + 1], s_tok), a.total_q) - s_tok, a.max_q);
    if (i >= n_q) return;
    const size_t stride_s = (size_t)a.nqb * kRows * kWsRow;
    const float* base = a.ws + (size_t)b * (unsigned)a.S * stride_s + (size_t)p * kWsRow;
    float M = -INFINITY;
    for (int s = 0; s < a.S; ++s) M = fmaxf(M, base[(size_t)s * stride_s + kDv]);
    float L = 0.0f;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const unsigned c4 = threadIdx.x * 4u;
#pragma unroll 4
    for (int s = 0; s < a.S; ++s) {
        const float* row = base + (size_t)s * stride_s;
        const float m = row[kDv];
        const float w = m == -INFINITY ? 0.0f : fast_exp2(m - M);
        L += row[kDv + 1] * w;
        acc += *reinterpret_cast<const f32x4*>(row + c4) * w;
    }
    float inv = L == 0.0f ? 0.0f : 1.0f / L;
    if constexpr (kFp8) inv *= a.c_scale ? *a.c_scale : 1.0f;
    const size_t tok = (size_t)s_tok + i;
    if (a.lse && threadIdx.x == 0) a.lse[(size_t)hd * (size_t)a.total_q + tok] = L == 0.0f ? -INFINITY : (M + __log2f(L)) * kMlaLn2;
    const size_t off = tok * (size_t)a.o_st + (size_t)hd * (size_t)a.o_sh + c4;
    if constexpr (kOutF32) {
        *reinterpret_cast<f32x4*>(static_cast<float*>(a.O) + off) = acc * inv;
    } else {
        *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(a.O) + off) = u32x2{T::pack2(acc[0] * inv, acc[1] * inv), T::pack2(acc[2] * inv, acc[3] * inv)};
    }
}

// The one or two launches of a checked call; each unit instantiates it for its own kFp8.
template <typename T, bool kOutF32, bool kFp8>
hipError_t mla_launch(const mla::Dev& a, bool paged, hipStream_t stream)
{
    const dim3 grid((unsigned)a.B * (unsigned)a.nqb * (unsigned)a.S), block(64 * mla::kW);
    void (*kernel)(mla::Dev);
    if (a.S > 1) kernel = paged ? fa_mla_decode_kernel<T, kOutF32, true, true, kFp8> : fa_mla_decode_kernel<T, kOutF32, true, false, kFp8>;
    else kernel = paged ? fa_mla_decode_kernel<T, kOutF32, false, true, kFp8> : fa_mla_decode_kernel<T, kOutF32, false, false, kFp8>;
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), mla::kLdsBytes);
    if (e != hipSuccess) return e;
    FA_LAUNCH(kernel, grid, block, (size_t)mla::kLdsBytes, stream, a);
    e = launch_status();
    if (e != hipSuccess || a.S <= 1) return e;
    FA_LAUNCH((fa_mla_merge_kernel<T, kOutF32, kFp8>), dim3((unsigned)a.B * (unsigned)a.max_q * (unsigned)a.Hq), dim3(128), 0, stream, a);
    return launch_status();
}
// (in_dtype, out_dtype) of a checked call -> the instantiation
template <bool kFp8> hipError_t mla_launch_typed(const mla::Dev& a, bool bf16, bool f32, bool paged, hipStream_t stream)
{
    if (bf16) return f32 ? mla_launch<BF16, true, kFp8>(a, paged, stream) : mla_launch<BF16, false, kFp8>(a, paged, stream);
    return f32 ? mla_launch<F16, true, kFp8>(a, paged, stream) : mla_launch<F16, false, kFp8>(a, paged, stream);
}
// fa_mla_decode_fp8.hip: mla_launch_typed<true>, the fp8 unit's instantiations behind the checks of fa_mla_decode.hip
hipError_t mla_launch_fp8(const mla::Dev& a, bool bf16, bool f32, bool paged, hipStream_t stream);

}  // namespace fa
