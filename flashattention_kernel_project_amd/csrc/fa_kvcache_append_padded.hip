// fa_kvcache_append_padded.hip -- the padded appends that do more than copy: the _rope forms of the four append entries, and
// fa_kvcache_append_ex with a token count per sequence (seqlens_new), rotary or not.  _rope: the new token's K is rotated at its key
// position p = L_b + t on the way into the cache (16 bit or e4m3fn, contiguous or paged), V goes in as the plain entries write it, and
// the step's Q rows [B, Hkv*G, Nnew, D] are rotated at the same positions, all in one launch; the cos / sin tables are the caller's
// (fp32 [max_pos, rot_dim / 2]) and, like lengths, block table and scales, are read on the device only.  seqlens_new: of the Nnew
// padded tokens of sequence b only the first m_b = min(max(seqlens_new[b], 0), Nnew) are written, and the length grows by m_b.  One
// kernel template serves all of it on the helpers of fa_kvcache_append.hpp, so every kept token's bytes are those of the flat entry
// of the form.  DESIGN.md sections 7.8 and 7.10.
#include "fa_kvcache_append.hpp"

// The rotary arithmetic is a contract of bytes: every product and every sum is rounded to fp32 on its own.  hipcc contracts a * b + c
// into a fused multiply-add in device code by default (and honours this pragma); from here to the end of the unit it does not.
// (rope1() of fa_kvcache_append.hpp, where the products and sums are, carries the same pragma in its body.)
#pragma clang fp contract(off)

namespace fa {

// One launch for K, V and Q.  blockIdx.x picks the tensor -- [0, kv_blocks) K, [kv_blocks, 2 kv_blocks) V, the rest Q -- so the
// choice is uniform over a workgroup; within a tensor thread g owns 16-byte chunk g of the contiguous source, as in
// fa_kvcache_append_kernel.  kRope: 0 no rotation (no Q blocks are launched), 1 half-split pairs, 2 interleaved pairs.  V, and K
// without rotation, is that kernel's copy or quantisation.  In a rotated K and in Q a chunk at or past rot_dim passes through
// (quantised on an fp8 cache).  Interleaved: the pairs (x[2i], x[2i+1]) lie inside the chunk.  Half-split: pair i is
// (x[i], x[i + rot_dim/2]), and the thread of a chunk in the first half owns the pair of chunks (c, c + rot_dim/16): it loads both,
// writes both and reads the eight table values once; the threads of the second half retire.  No thread reads a chunk another thread
// writes, which is what lets Qout be Q.  Position p = L_b + t and the table row min(p, max_pos - 1) are the same for a whole row.
// Cnt: nothing (the _rope entries: kRope 1 or 2, every sequence appends Nnew tokens), or one const int*, the counts.  A token
// t >= m_b retires before its position is formed: no length is added to it, no table entry is read for it, no address is formed
// from it.  Its Q row (rotary forms) is copied to Qout as it is, chunk by chunk, unless Qout is Q.  A trailing pack and not a null
// pointer, so that the count-less instantiations have the _rope kernels' argument list and code.
template <typename T, int D, bool kPaged, bool kFp8, int kRope, typename... Cnt>
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_padded_kernel(const uint16_t* __restrict__ Knew, const uint16_t* __restrict__ Vnew, void* __restrict__ Kdst,
                                void* __restrict__ Vdst, const uint16_t* Q, uint16_t* Qout, AppendDev a, RopeDev r,
                                Cnt __restrict__... seqlens_new)
{
    static_assert(sizeof...(Cnt) <= 1 && (std::is_same_v<Cnt, const int*> && ...), "at most one count vector");
    static_assert(sizeof...(Cnt) == 1 || kRope != 0, "without counts and without rotation the call is fa_kvcache_append_kernel's");
    constexpr int kLgChunks = D == 64 ? 3 : 4;   // log2 of the 16-byte chunks per row
    const unsigned which = blockIdx.x < r.kv_blocks ? 0u : (blockIdx.x < 2 * r.kv_blocks ? 1u : 2u);   // K, V, Q
    const bool is_q = which == 2, is_v = which == 1;
    const unsigned g = (blockIdx.x - which * r.kv_blocks) * (unsigned)kAppendThreads + threadIdx.x;
    if (g >= (is_q ? r.qchunks : a.chunks)) return;
    const unsigned row = g >> kLgChunks, c = g & ((1u << kLgChunks) - 1);
    const unsigned heads = is_q ? (unsigned)a.Hkv * (unsigned)r.G : (unsigned)a.Hkv;   // checked on the host: fits an int
    const unsigned bh = row / (unsigned)a.Nnew, t = row - bh * (unsigned)a.Nnew;
    const unsigned b = bh / heads, h = bh - b * heads;
    if constexpr (sizeof...(Cnt) == 1) {
        const int raw = (seqlens_new, ...)[b];
        const unsigned m = (unsigned)(raw < 0 ? 0 : (raw > a.Nnew ? a.Nnew : raw));
        if (t >= m) {   // a padding token
            if constexpr (kRope != 0) {
                if (is_q && Qout != Q) reinterpret_cast<u32x4*>(Qout)[g] = reinterpret_cast<const u32x4*>(Q)[g];
            }
            return;
        }
    }
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

    if (is_v || kRope == 0) {
        append_chunk<T, D, kFp8>(reinterpret_cast<const u32x4*>(is_v ? Vnew : Knew) + g, static_cast<char*>(is_v ? Vdst : Kdst), dst_row, c,
                                 is_v ? a.v_scale : a.k_scale, h);
        return;
    }

    if constexpr (kRope != 0) {   // K or Q of a rotary form: one body, instantiated for each (the choice is uniform over the workgroup)
        if (is_q) {
            rope_row<T, false, kRope == 2, false>(reinterpret_cast<const u32x4*>(Q) + g,
                                                  reinterpret_cast<char*>(Qout) + (size_t)row * (D * 2), c, p, 1.0f, r);
        } else {
            const float s = (kFp8 && a.k_scale) ? a.k_scale[h] : 1.0f;
            rope_row<T, kFp8, kRope == 2, (FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1))>(
                reinterpret_cast<const u32x4*>(Knew) + g, static_cast<char*>(Kdst) + dst_row * (kFp8 ? D : D * 2), c, p, s, r);
        }
    }
}

template <typename F, int kRope, typename... Cnt>
static hipError_t launch_padded(const KvAppendArgs& a, const AppendDev& dev, const RopeDev& r, unsigned blocks, Cnt... cnt)
{
    FA_LAUNCH((fa_kvcache_append_padded_kernel<typename F::T, F::D, F::kPaged, F::kFp8, kRope, Cnt...>), dim3(blocks), dim3(kAppendThreads), 0,
              a.stream, static_cast<const uint16_t*>(a.Knew), static_cast<const uint16_t*>(a.Vnew), a.K, a.V,
              static_cast<const uint16_t*>(a.Q), static_cast<uint16_t*>(a.Qout), dev, r, cnt...);
    const hipError_t e = launch_status();
    return e != hipSuccess ? e : kvappend_lens(a.seqlens, a.seqlens_new, nullptr, a.seqlens_out, a.B, a.Nnew, dev.Ncap, a.stream);
}

// `a` has passed kvcache_append_dispatch's checks (fa_kvcache_append.hip, the counts' buffer among them) and has a seqlens_new, a
// `rope`, or both; the rotary arguments are judged here, before the device is touched.  The grid follows (B, Hkv, G, Nnew, D) and
// whether there is a Q, never the counts.
hipError_t kvcache_append_padded(const KvAppendArgs& a, int Ncap, int lg_page)
{
    unsigned long long qchunks = 0;
    if (a.rope) {
        const hipError_t bad = kvappend_rope_check(a.rope_cos, a.rope_sin, a.rot_dim, a.D, a.max_pos, a.G, a.interleaved, (long long)a.B * a.Hkv);
        if (bad != hipSuccess) return bad;
        // a thread's chunk number is 32 bit in Q too
        qchunks = (unsigned long long)a.B * a.Hkv * (unsigned long long)a.G * (unsigned long long)a.Nnew * (unsigned)(a.D / 8);
        if (qchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        if ((a.Q == nullptr) != (a.Qout == nullptr)) return hipErrorInvalidValue;
        // Q and Qout: the same buffer or disjoint ones; never a partial overlap
        if (a.Q && a.Q != a.Qout && ranges_overlap(a.Q, (size_t)qchunks * 16, a.Qout, (size_t)qchunks * 16)) return hipErrorInvalidValue;
    }
    const unsigned chunks = (unsigned)((unsigned long long)a.B * a.Hkv * (unsigned long long)a.Nnew * (unsigned)(a.D / 8));
    const AppendDev dev = {a.seqlens, a.table, a.k_scale, a.v_scale, chunks, a.Hkv, a.Nnew, Ncap, a.max_pages, a.num_pages, lg_page};
    const unsigned kv_blocks = (chunks + kAppendThreads - 1) / kAppendThreads;
    const bool has_q = a.rope && a.Q;
    const unsigned q_blocks = has_q ? (unsigned)((qchunks + kAppendThreads - 1) / kAppendThreads) : 0u;
    const RopeDev r = {a.rope_cos, a.rope_sin, has_q ? (unsigned)qchunks : 0u, kv_blocks, a.rope ? a.G : 1, a.max_pos, a.rot_dim / 2,
                       a.rot_dim / 8};
    const unsigned blocks = 2 * kv_blocks + q_blocks;   // at most 3 * 2^23
    return append_form(a.dtype, a.D, a.paged, a.fp8, [&](auto form) {
        return append_rope_mode(a.rope, a.interleaved != 0, [&](auto mode) {
            using F = decltype(form);
            if (a.seqlens_new) return launch_padded<F, mode()>(a, dev, r, blocks, a.seqlens_new);
            if constexpr (mode() != 0) return launch_padded<F, mode()>(a, dev, r, blocks);
            return hipErrorInvalidValue;   // no counts and no rotation: the plain kernel's, which kvcache_append_dispatch keeps
        });
    });
}

}  // namespace fa
