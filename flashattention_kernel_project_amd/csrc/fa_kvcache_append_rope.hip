// fa_kvcache_append_rope.hip -- the _rope forms of the four append entries: the new token's K is rotated at its key position
// p = L_b + t on the way into the cache (16 bit or e4m3fn, contiguous or paged), V goes in as the plain entries write it, and the
// step's Q rows [B, Hkv*G, Nnew, D] are rotated at the same positions, all in one launch.  The cos / sin tables are the caller's
// (fp32 [max_pos, rot_dim / 2]) and, like lengths, block table and scales, are read on the device only.  DESIGN.md section 7.8.
#include "fa_kvcache_append.hpp"

#include <limits.h>

// The arithmetic is a contract of bytes: every product and every sum is rounded to fp32 on its own.  hipcc contracts a * b + c
// into a fused multiply-add in device code by default (and honours this pragma); from here to the end of the unit it does not.
// (rope1() of fa_kvcache_append.hpp, where the products and sums are, carries the same pragma in its body.)
#pragma clang fp contract(off)

namespace fa {

// One launch for K, V and Q.  blockIdx.x picks the tensor -- [0, kv_blocks) K, [kv_blocks, 2 kv_blocks) V, the rest Q -- so the
// choice is uniform over a workgroup; within a tensor thread g owns 16-byte chunk g of the contiguous source, as in
// fa_kvcache_append_kernel.  V is that kernel's copy or quantisation.  In K and Q a chunk at or past rot_dim passes through
// (quantised on an fp8 cache).  kInterleaved: the pairs (x[2i], x[2i+1]) lie inside the chunk.  Half-split: pair i is
// (x[i], x[i + rot_dim/2]), and the thread of a chunk in the first half owns the pair of chunks (c, c + rot_dim/16): it loads both,
// writes both and reads the eight table values once; the threads of the second half retire.  No thread reads a chunk another thread
// writes, which is what lets Qout be Q.  Position p = L_b + t and the table row min(p, max_pos - 1) are the same for a whole row.
template <typename T, int D, bool kPaged, bool kFp8, bool kInterleaved>
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_rope_kernel(const uint16_t* __restrict__ Knew, const uint16_t* __restrict__ Vnew, void* __restrict__ Kdst,
                              void* __restrict__ Vdst, const uint16_t* Q, uint16_t* Qout, AppendDev a, RopeDev r)
{
    constexpr int kLgChunks = D == 64 ? 3 : 4;   // log2 of the 16-byte chunks per row
    const unsigned which = blockIdx.x < r.kv_blocks ? 0u : (blockIdx.x < 2 * r.kv_blocks ? 1u : 2u);   // K, V, Q
    const bool is_q = which == 2, is_v = which == 1;
    const unsigned g = (blockIdx.x - which * r.kv_blocks) * (unsigned)kAppendThreads + threadIdx.x;
    if (g >= (is_q ? r.qchunks : a.chunks)) return;
    const unsigned row = g >> kLgChunks, c = g & ((1u << kLgChunks) - 1);
    const unsigned heads = is_q ? (unsigned)a.Hkv * (unsigned)r.G : (unsigned)a.Hkv;   // checked on the host: fits an int
    const unsigned bh = row / (unsigned)a.Nnew, t = row - bh * (unsigned)a.Nnew;
    const unsigned b = bh / heads, h = bh - b * heads;
    const unsigned p = append_len(a.seqlens, a.Ncap, b) + t;   // L <= Ncap < 2^31 and t < Nnew < 2^31: no wrap
    size_t dst_row = 0;                        // destination row of K or V, counted in rows of D elements
    if (!is_q) {
        if (p >= (unsigned)a.Ncap) return;     // dropped: not written, nothing loaded
        int page = 0;
        if constexpr (kPaged) {
            page = append_page(a.table, a.max_pages, a.lg_page, b, p);
            if ((unsigned)page >= (unsigned)a.num_pages) return;
        }
        dst_row = append_dst_row<kPaged>(page, a.Hkv, a.lg_page, a.Ncap, h, bh, p);
    }

    if (is_v) {   // fa_kvcache_append_kernel's body
        const u32x4* src = reinterpret_cast<const u32x4*>(Vnew) + g;
        constexpr bool kNt = FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1);
        const u32x4 v = kNt ? __builtin_nontemporal_load(src) : *src;
        char* dst = static_cast<char*>(Vdst);
        if constexpr (kFp8) {
            const float s = a.v_scale ? a.v_scale[h] : 1.0f;
            const u32x2 o = {quant4<T>(v[0], v[1], s), quant4<T>(v[2], v[3], s)};
            *reinterpret_cast<u32x2*>(dst + dst_row * D + c * 8) = o;
        } else {
            *reinterpret_cast<u32x4*>(dst + dst_row * (D * 2) + c * 16) = v;
        }
        return;
    }

    // K or Q: one body, instantiated for each (the choice is uniform over the workgroup)
    if (is_q) {
        rope_row<T, false, kInterleaved, false>(reinterpret_cast<const u32x4*>(Q) + g, reinterpret_cast<char*>(Qout) + (size_t)row * (D * 2),
                                                c, p, 1.0f, r);
    } else {
        const float s = (kFp8 && a.k_scale) ? a.k_scale[h] : 1.0f;
        rope_row<T, kFp8, kInterleaved, (FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1))>(
            reinterpret_cast<const u32x4*>(Knew) + g, static_cast<char*>(Kdst) + dst_row * (kFp8 ? D : D * 2), c, p, s, r);
    }
}

template <typename T, int D, bool kPaged, bool kFp8, bool kInterleaved>
static hipError_t launch_rope(const KvAppendArgs& a, const AppendDev& dev, const RopeDev& r, unsigned blocks)
{
    FA_LAUNCH((fa_kvcache_append_rope_kernel<T, D, kPaged, kFp8, kInterleaved>), dim3(blocks), dim3(kAppendThreads), 0, a.stream,
              static_cast<const uint16_t*>(a.Knew), static_cast<const uint16_t*>(a.Vnew), a.K, a.V,
              static_cast<const uint16_t*>(a.Q), static_cast<uint16_t*>(a.Qout), dev, r);
    const hipError_t e = launch_status();
    return e != hipSuccess ? e : kvcache_append_lens(a, dev.Ncap);
}

template <typename T, int D>
static hipError_t rope_forms(const KvAppendArgs& a, const AppendDev& dev, const RopeDev& r, unsigned blocks)
{
    const int form = (a.paged ? 4 : 0) | (a.fp8 ? 2 : 0) | (a.interleaved ? 1 : 0);
    switch (form) {
    case 0: return launch_rope<T, D, false, false, false>(a, dev, r, blocks);
    case 1: return launch_rope<T, D, false, false, true>(a, dev, r, blocks);
    case 2: return launch_rope<T, D, false, true, false>(a, dev, r, blocks);
    case 3: return launch_rope<T, D, false, true, true>(a, dev, r, blocks);
    case 4: return launch_rope<T, D, true, false, false>(a, dev, r, blocks);
    case 5: return launch_rope<T, D, true, false, true>(a, dev, r, blocks);
    case 6: return launch_rope<T, D, true, true, false>(a, dev, r, blocks);
    default: return launch_rope<T, D, true, true, true>(a, dev, r, blocks);
    }
}

// `a` has passed kvcache_append_dispatch's checks (fa_kvcache_append.hip); the rotary arguments are judged here, before the device
// is touched -- for the _rope entries below and for fa_kvcache_append_ex with a token count per sequence.
hipError_t kvcache_append_rope_check(const KvAppendArgs& a, unsigned long long& qchunks)
{
    if (!a.rope_cos || !a.rope_sin) return hipErrorInvalidValue;
    if (a.rot_dim < 16 || a.rot_dim > a.D || a.rot_dim % 16 != 0) return hipErrorInvalidValue;
    if (a.max_pos <= 0 || a.G <= 0 || (a.interleaved != 0 && a.interleaved != 1)) return hipErrorInvalidValue;
    const unsigned long long heads = (unsigned long long)a.B * a.Hkv * (unsigned long long)a.G;   // B * Hkv fits an int: checked
    if (heads > (unsigned long long)INT_MAX) return hipErrorInvalidValue;
    // a thread's chunk number is 32 bit in Q too
    qchunks = heads * (unsigned long long)a.Nnew * (unsigned)(a.D / 8);
    if (qchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if ((a.Q == nullptr) != (a.Qout == nullptr)) return hipErrorInvalidValue;
    if (a.Q && a.Q != a.Qout) {   // the same buffer or disjoint ones; never a partial overlap
        const uintptr_t in = reinterpret_cast<uintptr_t>(a.Q), out = reinterpret_cast<uintptr_t>(a.Qout);
        const uintptr_t bytes = (uintptr_t)qchunks * 16;
        if (in < out + bytes && out < in + bytes) return hipErrorInvalidValue;
    }
    return hipSuccess;
}

hipError_t kvcache_append_rope(const KvAppendArgs& a, int Ncap, int lg_page)
{
    unsigned long long qchunks = 0;
    const hipError_t bad = kvcache_append_rope_check(a, qchunks);
    if (bad != hipSuccess) return bad;
    const unsigned chunks = (unsigned)((unsigned long long)a.B * a.Hkv * (unsigned long long)a.Nnew * (unsigned)(a.D / 8));
    const AppendDev dev = {a.seqlens, a.table, a.k_scale, a.v_scale, chunks, a.Hkv, a.Nnew, Ncap, a.max_pages, a.num_pages, lg_page};
    const unsigned kv_blocks = (chunks + kAppendThreads - 1) / kAppendThreads;
    const unsigned q_blocks = a.Q ? (unsigned)((qchunks + kAppendThreads - 1) / kAppendThreads) : 0u;
    const RopeDev r = {a.rope_cos, a.rope_sin, a.Q ? (unsigned)qchunks : 0u, kv_blocks, a.G, a.max_pos, a.rot_dim / 2, a.rot_dim / 8};
    const unsigned blocks = 2 * kv_blocks + q_blocks;   // at most 3 * 2^23: from (B, Hkv, G, Nnew, D) and whether there is a Q
    if (a.dtype == 1) return a.D == 64 ? rope_forms<BF16, 64>(a, dev, r, blocks) : rope_forms<BF16, 128>(a, dev, r, blocks);
    return a.D == 64 ? rope_forms<F16, 64>(a, dev, r, blocks) : rope_forms<F16, 128>(a, dev, r, blocks);
}

}  // namespace fa
