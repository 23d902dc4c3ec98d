// fa_kvcache_append_ragged.hip -- fa_kvcache_append_ex with a token count per sequence (seqlens_new): of the Nnew padded tokens of
// sequence b only the first m_b = min(max(seqlens_new[b], 0), Nnew) are written, and the length grows by m_b.  One kernel template
// serves all eight forms (contiguous or paged, 16 bit or e4m3fn, plain or rotary): it is fa_kvcache_append_rope_kernel's layout --
// K, V and Q blocks in one launch -- with the rotation optional, on the helpers of fa_kvcache_append.hpp, so every kept token's
// bytes are those of the flat entry of the form.  The two flat units keep their device code.  DESIGN.md section 7.10.
#include "fa_kvcache_append.hpp"

// the rotary arithmetic is a contract of bytes: no fused multiply-add anywhere in this unit (fa_kvcache_append_rope.hip)
#pragma clang fp contract(off)

namespace fa {

// kRope: 0 no rotation (no Q blocks are launched), 1 half-split pairs, 2 interleaved pairs.  A token t >= m_b retires before its
// position is formed: no length is added to it, no table entry is read for it, no address is formed from it.  Its Q row (rotary
// forms) is copied to Qout as it is, chunk by chunk, unless Qout is Q.
template <typename T, int D, bool kPaged, bool kFp8, int kRope>
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_ragged_kernel(const uint16_t* __restrict__ Knew, const uint16_t* __restrict__ Vnew, void* __restrict__ Kdst,
                                void* __restrict__ Vdst, const uint16_t* Q, uint16_t* Qout, AppendDev a, RopeDev r,
                                const int* __restrict__ seqlens_new)
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
    const int raw = seqlens_new[b];
    const unsigned m = (unsigned)(raw < 0 ? 0 : (raw > a.Nnew ? a.Nnew : raw));
    if (t >= m) {   // a padding token
        if constexpr (kRope != 0) {
            if (is_q && Qout != Q) reinterpret_cast<u32x4*>(Qout)[g] = reinterpret_cast<const u32x4*>(Q)[g];
        }
        return;
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

    constexpr bool kNt = FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1);
    if (is_v || kRope == 0) {   // fa_kvcache_append_kernel's body: the copy, or the quantisation by the head's scale
        const u32x4* src = reinterpret_cast<const u32x4*>(is_v ? Vnew : Knew) + g;
        const u32x4 v = kNt ? __builtin_nontemporal_load(src) : *src;
        char* dst = static_cast<char*>(is_v ? Vdst : Kdst);
        if constexpr (kFp8) {
            const float* sp = is_v ? a.v_scale : a.k_scale;
            const float s = sp ? sp[h] : 1.0f;
            const u32x2 o = {quant4<T>(v[0], v[1], s), quant4<T>(v[2], v[3], s)};
            *reinterpret_cast<u32x2*>(dst + dst_row * D + c * 8) = o;
        } else {
            *reinterpret_cast<u32x4*>(dst + dst_row * (D * 2) + c * 16) = v;
        }
        return;
    }

    if constexpr (kRope != 0) {   // K or Q of a rotary form: fa_kvcache_append_rope_kernel's two calls
        if (is_q) {
            rope_row<T, false, kRope == 2, false>(reinterpret_cast<const u32x4*>(Q) + g,
                                                  reinterpret_cast<char*>(Qout) + (size_t)row * (D * 2), c, p, 1.0f, r);
        } else {
            const float s = (kFp8 && a.k_scale) ? a.k_scale[h] : 1.0f;
            rope_row<T, kFp8, kRope == 2, kNt>(reinterpret_cast<const u32x4*>(Knew) + g,
                                               static_cast<char*>(Kdst) + dst_row * (kFp8 ? D : D * 2), c, p, s, r);
        }
    }
}

// The lengths after the append, min(L_b + m_b, Ncap): fa_kvcache_append_lens_kernel with the sequence's own count.  Behind the copy
// on the same stream, so `out` may be `in` itself; `cnt` never overlaps `out` (checked on the host).
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_ragged_lens_kernel(const int* in, const int* __restrict__ cnt, int* out, int B, int Nnew, int Ncap)
{
    const unsigned i = blockIdx.x * (unsigned)kAppendThreads + threadIdx.x;
    if (i >= (unsigned)B) return;
    const int L = (int)append_len(in, Ncap, i);
    const int raw = cnt[i];
    const long long n = (long long)L + (raw < 0 ? 0 : (raw > Nnew ? Nnew : raw));
    out[i] = n < Ncap ? (int)n : Ncap;
}

template <typename T, int D, bool kPaged, bool kFp8, int kRope>
static hipError_t launch_ragged(const KvAppendArgs& a, const AppendDev& dev, const RopeDev& r, unsigned blocks)
{
    FA_LAUNCH((fa_kvcache_append_ragged_kernel<T, D, kPaged, kFp8, kRope>), dim3(blocks), dim3(kAppendThreads), 0, a.stream,
              static_cast<const uint16_t*>(a.Knew), static_cast<const uint16_t*>(a.Vnew), a.K, a.V,
              static_cast<const uint16_t*>(a.Q), static_cast<uint16_t*>(a.Qout), dev, r, a.seqlens_new);
    hipError_t e = launch_status();
    if (e != hipSuccess || !a.seqlens_out) return e;
    FA_LAUNCH(fa_kvcache_append_ragged_lens_kernel, dim3(((unsigned)a.B + kAppendThreads - 1) / kAppendThreads), dim3(kAppendThreads), 0,
              a.stream, a.seqlens, a.seqlens_new, a.seqlens_out, a.B, a.Nnew, dev.Ncap);
    return launch_status();
}

template <typename T, int D, int kRope>
static hipError_t ragged_forms(const KvAppendArgs& a, const AppendDev& dev, const RopeDev& r, unsigned blocks)
{
    if (a.paged)
        return a.fp8 ? launch_ragged<T, D, true, true, kRope>(a, dev, r, blocks) : launch_ragged<T, D, true, false, kRope>(a, dev, r, blocks);
    return a.fp8 ? launch_ragged<T, D, false, true, kRope>(a, dev, r, blocks) : launch_ragged<T, D, false, false, kRope>(a, dev, r, blocks);
}

template <typename T, int D>
static hipError_t ragged_rope_modes(const KvAppendArgs& a, const AppendDev& dev, const RopeDev& r, unsigned blocks)
{
    if (!a.rope) return ragged_forms<T, D, 0>(a, dev, r, blocks);
    return a.interleaved ? ragged_forms<T, D, 2>(a, dev, r, blocks) : ragged_forms<T, D, 1>(a, dev, r, blocks);
}

// `a` has passed kvcache_append_dispatch's checks (fa_kvcache_append.hip) and has a seqlens_new; what that adds is judged here, and
// with `rope` the rotary arguments by the _rope entries' own check, all before the device is touched.  The grid is the flat
// entry's: it follows (B, Hkv, G, Nnew, D) and whether there is a Q, never the counts.
hipError_t kvcache_append_ragged(const KvAppendArgs& a, int Ncap, int lg_page)
{
    if (a.seqlens_out) {   // the counts are read by the lengths kernel while it writes: no overlap at all, identity included
        const uintptr_t cnt = reinterpret_cast<uintptr_t>(a.seqlens_new), out = reinterpret_cast<uintptr_t>(a.seqlens_out);
        const uintptr_t bytes = (uintptr_t)a.B * sizeof(int);
        if (cnt < out + bytes && out < cnt + bytes) return hipErrorInvalidValue;
    }
    unsigned long long qchunks = 0;
    if (a.rope) {
        const hipError_t bad = kvcache_append_rope_check(a, qchunks);
        if (bad != hipSuccess) return bad;
    }
    const unsigned chunks = (unsigned)((unsigned long long)a.B * a.Hkv * (unsigned long long)a.Nnew * (unsigned)(a.D / 8));
    const AppendDev dev = {a.seqlens, a.table, a.k_scale, a.v_scale, chunks, a.Hkv, a.Nnew, Ncap, a.max_pages, a.num_pages, lg_page};
    const unsigned kv_blocks = (chunks + kAppendThreads - 1) / kAppendThreads;
    const bool has_q = a.rope && a.Q;
    const unsigned q_blocks = has_q ? (unsigned)((qchunks + kAppendThreads - 1) / kAppendThreads) : 0u;
    const RopeDev r = {a.rope_cos, a.rope_sin, has_q ? (unsigned)qchunks : 0u, kv_blocks, a.rope ? a.G : 1, a.max_pos, a.rot_dim / 2,
                       a.rot_dim / 8};
    const unsigned blocks = 2 * kv_blocks + q_blocks;
    if (a.dtype == 1) return a.D == 64 ? ragged_rope_modes<BF16, 64>(a, dev, r, blocks) : ragged_rope_modes<BF16, 128>(a, dev, r, blocks);
    return a.D == 64 ? ragged_rope_modes<F16, 64>(a, dev, r, blocks) : ragged_rope_modes<F16, 128>(a, dev, r, blocks);
}

}  // namespace fa
