// fa_mla_sparse_kernel.hpp -- device code of fa_mla_decode_sparse (fa_mla_sparse.hip): MLA decode over per-token key index lists.
// Every head of a token attends to the topk latent rows its list names, gathered from the cache where they lie.  From the dense
// kernel (fa_mla_decode_kernel.hpp, included) come the LDS image (mla::img_off / swz, 32-entry tiles, two buffers), the row reads of
// S^T = C Q^T, the ds_read_b64_tr_b16 reads of O^T += V^T P^T, the lazy maximum, the P packing, the epilogue arithmetic and the merge
// kernel.  What is new is the work split -- a workgroup serves ONE token -- the index pipeline and the gather.  Private to csrc/.
// DESIGN.md section 7.29, profiles/mla_sparse.txt.
#pragma once
#include "fa_mla_decode_kernel.hpp"

namespace fa {

namespace mlas {
constexpr int kMaxTopk = 1 << 20;
typedef __attribute__((address_space(1))) u32x4 gmem_u32x4;   // a row address rebuilt from two scalars is global memory, not flat
// mla::Dev as the merge kernel reads it (nqb = ceil(max_q * Hq / 64): the workspace's rows per (b, split)), and the list
struct Dev {
    mla::Dev d;
    const int* indices;
    long long idx_st;       // entries between two tokens' lists
    int topk, chunk, nhb;   // chunk: entries per split, a multiple of 64; nhb = ceil(Hq / 64) head blocks
};
}  // namespace mlas

// Work: workgroup (b, i, hb, sp) serves token s_b + i, heads 64 hb .. 64 hb + 63 and the entries [sp * chunk, sp * chunk + chunk) of
// the token's list; it returns before reading anything when i >= n_b.  A wave owns 32 heads (lane & 31) and one half of the 512
// output columns, as in the dense kernel.  c_i is workgroup-uniform: an entry is visible iff 0 <= j < c_i, for staging and masking.
// Index pipeline: entry r = lane & 31 of a tile is the lane's (both halves hold the same).  fetch() loads the index, predicated on
// the entry lying in the split, tests visibility, and -- paged, predicated on visibility -- loads the table entry; the lane then
// holds the 64-bit address of its row, or of nothing.  It runs two tiles ahead of the arithmetic.  take() turns that into
// wave-uniform values: the ballot of the visible entries (the -inf pattern of the tile), the ballot of the rows to load (visible and
// on a good page) and, by readlane, the addresses of the 8 rows this wave stages.
// Gather: the wave's 8 rows are 8 x 72 chunks; load p of a lane is chunk idx % 72 of row idx / 72, idx = lane + 64 p -- the dense
// kernel's map, so the ds_write_b128 rounds are its rounds and stay conflict-free under swz.  The 64 lanes of a
// load span at most two rows, both known at compile time: each is one global load from the row's scalar base with 16 * lane as the
// offset, under the lanes of that row and the row's load bit.  A lane whose bit is clear keeps zeros: no address is formed for a
// masked entry or a bad page.  No non-temporal hint: the second head block and neighbouring tokens read the same rows again.
// A tile without a visible entry is not skipped: o + 0 is not o for an accumulator at -0.
template <typename T, bool kOutF32, bool kPartial, bool kPaged>
__global__ __launch_bounds__(64 * mla::kW, 1)
void fa_mla_sparse_kernel(mlas::Dev p)
{
    using namespace mla;
    static_assert(kTile == 32 && kRB == 2 && kDS == 2 && kGroups == 1, "the sparse kernel is written for the 32-entry tile");
    const mla::Dev& a = p.d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned sp = blockIdx.x % (unsigned)a.S, rest = blockIdx.x / (unsigned)a.S;
    const unsigned hb = rest % (unsigned)p.nhb, rest2 = rest / (unsigned)p.nhb;
    const unsigned i = rest2 % (unsigned)a.max_q, b = rest2 / (unsigned)a.max_q;
    const unsigned tid = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const unsigned rb = wave / (unsigned)kDS, dh = wave % (unsigned)kDS;

    // the sequence's rows: fa_mla_decode's clamps
    const int s_tok = min(max(a.cu_q[b], 0), a.total_q);
    const unsigned n_q = (unsigned)min(min(max(a.cu_q[b + 1], s_tok), a.total_q) - s_tok, a.max_q);
    if (i >= n_q) return;   // workgroup-uniform: no such row; nothing was read
    const unsigned nkeys = a.seqlens ? (unsigned)min(max(a.seqlens[b], 0), a.cap) : (unsigned)a.cap;
    const unsigned c_i = a.causal ? (unsigned)max((int)nkeys - (int)n_q + 1 + (int)i, 0) : nkeys;   // <= nkeys <= 2^30
    const size_t tok = (size_t)s_tok + i;
    const unsigned e0 = sp * (unsigned)p.chunk, e1 = min((unsigned)p.topk, e0 + (unsigned)p.chunk);
    const int ntiles = e0 >= (unsigned)p.topk ? 0 : (int)((e1 - e0 + kTile - 1) / kTile);

    // the lane's row: head hd of the token
    const unsigned hd = hb * (unsigned)kRows + rb * 32u + r;
    const bool row_live = hd < (unsigned)a.Hq;
    const bool has_rows = hb * (unsigned)kRows + rb * 32u < (unsigned)a.Hq;   // wave-uniform
    const unsigned qend = (unsigned)((unsigned long long)((long long)(a.Hq - 1) * a.q_sh + kDqk) * 2u);
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(a.Q + (long long)tok * a.q_st, qend);
    const unsigned qoff = row_live ? hd * (unsigned)a.q_sh * 2u : qend;   // a dead lane reads zeros

    const float sl2 = a.scale_log2e;
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

    // ---- the index pipeline -----------------------------------------------------------------------------------------------------------
    const int* irow = p.indices + (long long)tok * p.idx_st;
    const char* cbase = a.C;
    if constexpr (!kPaged) cbase += (size_t)b * (unsigned)a.cap * kRowBytes;
    unsigned long long nx_addr = 0;     // the lane's entry of the fetched tile: its row's address (0: nothing to load) ...
    bool nx_vis = false;                // ... and whether the entry is visible
    auto fetch = [&](unsigned t) {
        const unsigned e = e0 + t * kTile + r;
        int j = -1;
        if (e < e1) j = irow[e];
        nx_vis = (unsigned)j < c_i;     // a negative j is a large unsigned number
        bool ok = nx_vis;
        size_t slot = (unsigned)j;
        if constexpr (kPaged) {
            int pg = -1;
            if (nx_vis) pg = a.table[(size_t)b * (unsigned)a.max_pages + ((unsigned)j >> a.lg_page)];   // j < c_i <= max_pages * page_size
            ok = (unsigned)pg < (unsigned)a.num_pages;   // false for a masked entry too
            slot = ((size_t)(unsigned)pg << a.lg_page) + ((unsigned)j & ((1u << a.lg_page) - 1u));
        }
        nx_addr = ok ? (unsigned long long)(uintptr_t)cbase + slot * kRowBytes : 0ull;
    };
    unsigned vis_next = 0, ld_bits = 0;           // wave-uniform: the taken tile's visible entries, and its 8 load bits of this wave
    unsigned long long rows[8];                   // wave-uniform: the addresses of the wave's 8 rows
    auto take = [&]() {
        vis_next = (unsigned)__ballot(nx_vis);
        const unsigned lo = (unsigned)nx_addr, hi = (unsigned)(nx_addr >> 32);
#pragma unroll
        for (int R = 0; R < 8; ++R) {
            const unsigned l = __builtin_amdgcn_readlane(lo, wave * 8u + R), u = __builtin_amdgcn_readlane(hi, wave * 8u + R);
            rows[R] = ((unsigned long long)u << 32) | l;
        }
        ld_bits = ((unsigned)__ballot(nx_addr != 0ull) >> (wave * 8u)) & 0xFFu;
    };

    // ---- the gather -------------------------------------------------------------------------------------------------------------------
    unsigned l_off[kGroupLoads];
#pragma unroll
    for (int q = 0; q < kGroupLoads; ++q) {
        const unsigned idx = lane + 64u * q;
        l_off[q] = img_off(wave * 8u + idx / (unsigned)kChunks, idx % (unsigned)kChunks);
    }
    u32x4 st[kGroupLoads];
    auto stage_load = [&]() {
        // 16 * lane is made here, behind an empty asm: as a loop invariant the compiler adds each load's constant to it ahead of the
        // loop, seventeen 64-bit per-lane addresses that do not fit the register file
        unsigned lane16 = lane * 16u;
        asm volatile("" : "+v"(lane16));
#pragma unroll
        for (int q = 0; q < kGroupLoads; ++q) {
            // the one or two rows of this load are constants: each is one load from a scalar base with the lane's 16 * lane as the
            // 32-bit offset and the rest in the instruction's immediate, under the lanes of that row and the row's load bit
            constexpr int kCh = kChunks;
            const int R0 = (64 * q) / kCh, R1 = (64 * q + 63) / kCh;
            const bool up = R1 != R0 && lane + 64u * q >= (unsigned)(R1 * kCh);
            u32x4 v = {0u, 0u, 0u, 0u};
            if (!up && ((ld_bits >> R0) & 1u))
                v = *reinterpret_cast<const mlas::gmem_u32x4*>((uintptr_t)(rows[R0] + (long long)((64 * q - R0 * kCh) * 16)) + (size_t)lane16);
            if (up && ((ld_bits >> R1) & 1u))
                v = *reinterpret_cast<const mlas::gmem_u32x4*>((uintptr_t)(rows[R1] + (long long)((64 * q - R1 * kCh) * 16)) + (size_t)lane16);
            st[q] = v;
        }
    };
    auto stage_write = [&](unsigned buf) {
#pragma unroll
        for (int q = 0; q < kGroupLoads; ++q) lds_write16(smem, buf * kTileBytes + l_off[q], st[q]);
    };

    // row reads of S^T and transposed reads of O^T: the dense kernel's
    unsigned k_rd[4];
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) k_rd[k4] = r * kRowBytes + (((2u * k4 + h) ^ swz(r)) << 4);
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
    for (int x = 0; x < 16; ++x) zero16[x] = 0.0f;
#pragma unroll
    for (int db = 0; db < kDBlocks; ++db) o[db] = zero16;
    float m_ref = -INFINITY, l_part = 0.0f;

    unsigned vis_cur = 0;
    if (ntiles > 0) {   // workgroup-uniform
        fetch(0);
        take();
        stage_load();
        vis_cur = vis_next;
        fetch(1);
        stage_write(0);
        __syncthreads();
    }
    for (int t = 0; t < ntiles; ++t) {
        const unsigned cur = t & 1u;
        const char* kbuf = smem + cur * kTileBytes;
        if (t + 1 < ntiles) {
            take();         // tile t + 1, fetched one iteration ago
            stage_load();
        }
        fetch((unsigned)t + 2u);   // past the split's end: every entry masked, nothing read

        if (has_rows) {   // a wave without a live head only stages
            f32x16 s;
#pragma unroll
            for (int ks = 0; ks < kKSteps; ++ks) {
                const u32x4 kf = lds_read16(kbuf, (unsigned)(ks >> 2) * 128u + k_rd[ks & 3]);
                s = T::mfma32(kf, qf[ks], ks == 0 ? zero16 : s);
            }
            if (vis_cur != 0xFFFFFFFFu) {   // wave-uniform; register x of half h is entry (x & 3) + 8 (x >> 2) + 4 h
                const unsigned m = vis_cur >> (4u * h);
#pragma unroll
                for (int x = 0; x < 16; ++x)
                    if (!((m >> ((x & 3) + 8 * (x >> 2))) & 1u)) s[x] = -INFINITY;
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; e += 2) tmax = max3(tmax, s[e], s[e + 1]);
            tmax *= c;
            if (__any(tmax > m_ref + kThr)) {   // the lazy reference maximum, as in the dense kernel
                const float mx = fmaxf(tmax, swap_halves(tmax));
                const float m_new = fmaxf(mx, m_ref);
                const float alpha = m_ref == -INFINITY ? 0.0f : fast_exp2(m_ref - m_new);
                m_ref = m_new;
#pragma unroll
                for (int db = 0; db < kDBlocks; ++db)
#pragma unroll
                    for (int x = 0; x < 16; ++x) o[db][x] *= alpha;
                l_part *= alpha;
            }
            u32x4 pk[2];
            float ls0 = 0.0f, ls1 = 0.0f;
            const float neg_m = m_ref == -INFINITY ? 0.0f : -m_ref;
#pragma unroll
            for (int q4 = 0; q4 < 2; ++q4) {
                const int b8 = q4 * 8;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const float p0 = fast_exp2(__builtin_fmaf(s[b8 + 2 * w], c, neg_m));
                    const float p1 = fast_exp2(__builtin_fmaf(s[b8 + 2 * w + 1], c, neg_m));
                    pk[q4][w] = T::pack2(p0, p1);
                    if (w & 1) ls1 = T::sum2(pk[q4][w], ls1);
                    else ls0 = T::sum2(pk[q4][w], ls0);
                }
            }
            l_part += ls0 + ls1;
#pragma unroll
            for (int q4 = 0; q4 < 2; ++q4)
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
        vis_cur = vis_next;
        __syncthreads();
    }

    const float l = l_part + swap_halves(l_part);
    if constexpr (kPartial) {
        // workspace row ((b, sp), i * Hq + hd): the merge kernel's layout; only live heads are written -- a dead lane's row index
        // would be a row of the next token
        float* row = a.ws + (((size_t)b * (unsigned)a.S + sp) * ((size_t)a.nqb * kRows) + (size_t)i * (unsigned)a.Hq + hd) * kWsRow;
        if (row_live) {
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
        const float inv = l == 0.0f ? 0.0f : 1.0f / l;   // a token without a visible entry: O = 0
        if (a.lse && h == 0 && dh == 0 && row_live)
            a.lse[(size_t)hd * (size_t)a.total_q + tok] = l == 0.0f ? -INFINITY : (m_ref + __log2f(l)) * kMlaLn2;
        constexpr unsigned es = kOutF32 ? 4u : 2u;
        const unsigned oend = (unsigned)((unsigned long long)((long long)(a.Hq - 1) * a.o_sh + kDv) * es);
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(a.O) + (long long)tok * a.o_st * (long long)es, oend);
        const unsigned ooff = row_live ? hd * (unsigned)a.o_sh * es : oend;
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

// fa_mla_decode.hip: the launch of its 16-bit merge kernels, so that this unit holds no second copy of them
hipError_t mla_merge_launch(const mla::Dev& a, bool bf16, bool f32, hipStream_t stream);

// The one or two launches of a checked call; the merge behind a split is the dense entry's kernel on the same workspace layout.
template <typename T, bool kOutF32>
hipError_t mla_sparse_launch(const mlas::Dev& p, bool paged, hipStream_t stream)
{
    const mla::Dev& a = p.d;
    const dim3 grid((unsigned)a.B * (unsigned)a.max_q * (unsigned)p.nhb * (unsigned)a.S), block(64 * mla::kW);
    void (*kernel)(mlas::Dev);
    if (a.S > 1) kernel = paged ? fa_mla_sparse_kernel<T, kOutF32, true, true> : fa_mla_sparse_kernel<T, kOutF32, true, false>;
    else kernel = paged ? fa_mla_sparse_kernel<T, kOutF32, false, true> : fa_mla_sparse_kernel<T, kOutF32, false, false>;
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), mla::kLdsBytes);
    if (e != hipSuccess) return e;
    FA_LAUNCH(kernel, grid, block, (size_t)mla::kLdsBytes, stream, p);
    e = launch_status();
    if (e != hipSuccess || a.S <= 1) return e;
    return mla_merge_launch(a, T::id == BF16::id, kOutF32, stream);
}

}  // namespace fa
