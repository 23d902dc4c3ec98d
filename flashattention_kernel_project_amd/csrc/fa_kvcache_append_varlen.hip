// fa_kvcache_append_varlen.hip -- fa_kvcache_append_varlen: the append of a token-packed batch.  Knew, Vnew (total_new, Hkv, d) and, with
// rotary, Q (total_new, Hkv*G, d) are read through their own token and head strides, as views of the projection's buffer lie, and cut
// into sequences by cu_seqlens_new on the device.  One kernel template serves all eight forms (contiguous or paged, 16 bit or e4m3fn,
// plain or rotary) on the helpers of fa_kvcache_append.hpp, so every kept token's bytes are those fa_kvcache_append_ex writes from the
// padded head-major copy of the same rows.  The search of cu_seqlens_new, the lengths kernel and the host checks are the write
// side's shared ones.  DESIGN.md section 7.16.
#include "../../include/fa_mi355.h"
#include "fa_kvcache_append.hpp"

// the rotary arithmetic is a contract of bytes: no fused multiply-add anywhere in this unit (fa_kvcache_append_padded.hip)
#pragma clang fp contract(off)

// The thread order over (token, head, chunk) inside a tensor: 0 = token-major (a wave reads the heads of a token in a row, as the
// projection wrote them), 1 = head-major (a wave writes consecutive rows of one head's cache).  Both measured in
// profiles/kvcache_append_varlen.txt; the default is what ships.
#ifndef FA_APPEND_VARLEN_ORDER
#define FA_APPEND_VARLEN_ORDER 0
#endif

namespace fa {

namespace {

// The packed sources.  Strides are counted in 16-byte chunks (the host checked that they are multiples of 8 elements).
struct PackedDev {
    const int* cu;     // [B + 1] on the device
    int B, total;      // total: HOST, the token rows of every source
    long long k_t, k_h, v_t, v_h, q_t, q_h, qo_t, qo_h;
};

}  // namespace

// kRope: 0 no rotation (no Q blocks are launched), 1 half-split pairs, 2 interleaved pairs.  A row that no sequence owns retires
// before anything is formed from it: nothing is loaded, nothing is written, its Qout row stays as it was.  For an owned row
// i = t - s_b lies in [0, m_b) whatever the vector holds, and from there on the steps are fa_kvcache_append_padded_kernel's.
// Pos: nothing, or -- fa_kvcache_append_varlen_ex with positions, rotary forms only -- one const int*: the table row of token t is
// then positions[t] clamped into [0, max_pos), read once the row has an owner, while the destination stays slot p.  A trailing pack
// and not a flag with an argument of its own, so that the plain instantiations keep their argument list and their code.
template <typename T, int D, bool kPaged, bool kFp8, int kRope, bool kHeadMajor, typename... Pos>
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_varlen_kernel(const uint16_t* __restrict__ Knew, const uint16_t* __restrict__ Vnew, void* __restrict__ Kdst,
                                void* __restrict__ Vdst, const uint16_t* Q, uint16_t* Qout, AppendDev a, RopeDev r, PackedDev k,
                                Pos... positions)
{
    static_assert(sizeof...(Pos) <= 1 && (std::is_same_v<Pos, const int*> && ...), "at most one position vector");
    static_assert(sizeof...(Pos) == 0 || kRope != 0, "positions belong to the rotary forms");
    constexpr int kLgChunks = D == 64 ? 3 : 4;   // log2 of the 16-byte chunks per row
    const unsigned which = blockIdx.x < r.kv_blocks ? 0u : (blockIdx.x < 2 * r.kv_blocks ? 1u : 2u);   // K, V, Q
    const bool is_q = which == 2, is_v = which == 1;
    const unsigned g = (blockIdx.x - which * r.kv_blocks) * (unsigned)kAppendThreads + threadIdx.x;
    if (g >= (is_q ? r.qchunks : a.chunks)) return;
    const unsigned row = g >> kLgChunks, c = g & ((1u << kLgChunks) - 1);
    const unsigned heads = is_q ? (unsigned)a.Hkv * (unsigned)r.G : (unsigned)a.Hkv;   // checked on the host: fits an int
    unsigned t, hh;   // the token row and the head of its tensor
    if constexpr (kHeadMajor) {
        hh = row / (unsigned)k.total;
        t = row - hh * (unsigned)k.total;
    } else {
        t = row / heads;
        hh = row - t * heads;
    }
    // The sequence of the row.  The wave's first lane searches for all (uniform: scalar registers); a lane whose row that sequence
    // does not own -- the wave crosses a boundary, or wraps to the next head -- searches for itself.
    const unsigned t0 = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    unsigned b = seq_search(k.cu, (unsigned)k.B, k.total, t0), s;
    if (!seq_owns(k.cu, b, k.total, t, s)) {
        b = seq_search(k.cu, (unsigned)k.B, k.total, t);
        if (!seq_owns(k.cu, b, k.total, t, s)) return;   // a row of no sequence
    }
    const unsigned i = t - s;                                   // < m_b <= total
    const unsigned p = append_len(a.seqlens, a.Ncap, b) + i;    // L <= Ncap < 2^31 and i < 2^31: no wrap
    const unsigned h = is_q ? hh / (unsigned)r.G : hh;          // the K/V head
    size_t dst_row = 0;                        // destination row of K or V, counted in rows of D elements
    if (!is_q) {
        if (p >= (unsigned)a.Ncap) return;     // dropped: not written, nothing loaded
        int page = 0;
        if constexpr (kPaged) {
            page = append_page(a.table, a.max_pages, a.lg_page, b, p);
            if ((unsigned)page >= (unsigned)a.num_pages) return;
        }
        dst_row = append_dst_row<kPaged>(page, a.Hkv, a.lg_page, a.Ncap, h, b * (unsigned)a.Hkv + h, p);
    }

    if (is_v || kRope == 0) {
        const u32x4* src = reinterpret_cast<const u32x4*>(is_v ? Vnew : Knew) +
                           ((size_t)t * (size_t)(is_v ? k.v_t : k.k_t) + (size_t)hh * (size_t)(is_v ? k.v_h : k.k_h) + c);
        append_chunk<T, D, kFp8>(src, static_cast<char*>(is_v ? Vdst : Kdst), dst_row, c, is_v ? a.v_scale : a.k_scale, h);
        return;
    }

    if constexpr (kRope != 0) {   // K or Q of a rotary form: fa_kvcache_append_padded_kernel's two calls
        constexpr bool kNt = FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1);
        unsigned rp = p;   // the table row: the slot, or the token's entry of the vector (rope_row clamps it at max_pos - 1)
        if constexpr (sizeof...(Pos) == 1) {
            const int at = (positions, ...)[t];
            rp = at < 0 ? 0u : (unsigned)at;
        }
        if (is_q) {
            const u32x4* src = reinterpret_cast<const u32x4*>(Q) + ((size_t)t * (size_t)k.q_t + (size_t)hh * (size_t)k.q_h + c);
            char* dst = reinterpret_cast<char*>(Qout) + ((size_t)t * (size_t)k.qo_t + (size_t)hh * (size_t)k.qo_h) * 16;
            rope_row<T, false, kRope == 2, false>(src, dst, c, rp, 1.0f, r);
        } else {
            const float sc = (kFp8 && a.k_scale) ? a.k_scale[h] : 1.0f;
            const u32x4* src = reinterpret_cast<const u32x4*>(Knew) + ((size_t)t * (size_t)k.k_t + (size_t)hh * (size_t)k.k_h + c);
            rope_row<T, kFp8, kRope == 2, kNt>(src, static_cast<char*>(Kdst) + dst_row * (kFp8 ? D : D * 2), c, rp, sc, r);
        }
    }
}

namespace {

struct VarlenAppendCall {
    const fa_kvappend_varlen_desc* d;
    AppendDev dev;
    RopeDev r;
    PackedDev k;
    unsigned blocks;
};

// Pos: nothing, or the position vector (rotary forms only)
template <typename F, int kRope, typename... Pos>
hipError_t launch_varlen(const VarlenAppendCall& c, Pos... positions)
{
    const fa_kvappend_varlen_desc* d = c.d;
    hipStream_t stream = static_cast<hipStream_t>(d->stream);
    FA_LAUNCH((fa_kvcache_append_varlen_kernel<typename F::T, F::D, F::kPaged, F::kFp8, kRope, FA_APPEND_VARLEN_ORDER != 0, Pos...>),
              dim3(c.blocks), dim3(kAppendThreads), 0, stream, static_cast<const uint16_t*>(d->Knew), static_cast<const uint16_t*>(d->Vnew),
              d->K, d->V, static_cast<const uint16_t*>(d->Q), static_cast<uint16_t*>(d->Qout), c.dev, c.r, c.k, positions...);
    const hipError_t e = launch_status();
    return e != hipSuccess ? e : kvappend_lens(d->seqlens_k, nullptr, d->cu_seqlens_new, d->seqlens_out, d->B, d->total_new, c.dev.Ncap, stream);
}

// fa_varlen_desc's rules for a packed tensor (total, H, d) of 16-bit elements, without its 32-bit bound: the addresses here are 64 bit
bool packed_ok(const void* p, int d, long long st, long long sh)
{
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15u)) return false;
    return st >= d && sh >= 0 && st % 8 == 0 && sh % 8 == 0;
}

// the bytes from the tensor's base to the end of its last row
unsigned __int128 packed_extent(int total, long long H, int d, long long st, long long sh)
{
    return ((unsigned __int128)(total - 1) * (unsigned long long)st + (unsigned __int128)(H - 1) * (unsigned long long)sh + (unsigned)d) * 2u;
}

// ranges_overlap for extents that strides of 2^63 elements can reach
bool ranges_overlap(const void* x, unsigned __int128 xbytes, const void* y, unsigned __int128 ybytes)
{
    const unsigned __int128 a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y);
    return a < b + ybytes && b < a + xbytes;
}

}  // namespace

// Every check, then the one or two launches.  The grid follows (total_new, Hkv, G, d) and whether there is a Q: host integers only.
// positions (fa_kvcache_append_varlen_ex; null: none) selects the position instantiations of the same kernel.
static hipError_t append_varlen_checked(const ::fa_kvappend_varlen_desc* d, const int* positions)
{
    if (!d || d->size != sizeof(fa_kvappend_varlen_desc)) return hipErrorInvalidValue;
    if (positions && (!d->rope_cos || (reinterpret_cast<uintptr_t>(positions) & 3u))) return hipErrorInvalidValue;
    if (d->kv_dtype != FA_KV_16BIT && d->kv_dtype != FA_KV_FP8_E4M3) return hipErrorInvalidValue;
    const bool fp8 = d->kv_dtype == FA_KV_FP8_E4M3, paged = d->block_table != nullptr, rope = d->rope_cos != nullptr;
    if (!fp8 && (d->k_scale || d->v_scale)) return hipErrorInvalidValue;               // a 16-bit cache has no scales
    if (!rope && (d->Q || d->Qout || d->rope_sin)) return hipErrorInvalidValue;        // arguments of the rotary forms
    if (!d->cu_seqlens_new || d->total_new <= 0) return hipErrorInvalidValue;
    int Ncap = 0, lg_page = 0;
    const hipError_t bad = kvwrite_check(write_cache_of(*d, d->Knew, d->Vnew), Ncap, lg_page);
    if (bad != hipSuccess) return bad;
    if (!packed_ok(d->Knew, d->d, d->k_stride_t, d->k_stride_h) || !packed_ok(d->Vnew, d->d, d->v_stride_t, d->v_stride_h))
        return hipErrorInvalidValue;
    // a thread's chunk number is 32 bit (so is the grid)
    const unsigned long long chunks = (unsigned long long)d->total_new * (unsigned)d->Hkv * (unsigned)(d->d / 8);
    if (chunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (!lens_out_ok(d->seqlens_k, d->seqlens_out, d->B, d->cu_seqlens_new, ((size_t)d->B + 1) * sizeof(int))) return hipErrorInvalidValue;
    unsigned long long qchunks = 0;
    const int G = rope ? d->G : 1;
    if (rope) {
        const hipError_t bad_rope = kvappend_rope_check(d->rope_cos, d->rope_sin, d->rot_dim, d->d, d->max_pos, G, d->interleaved,
                                                        (long long)d->B * d->Hkv);
        if (bad_rope != hipSuccess) return bad_rope;
        qchunks = (unsigned long long)d->total_new * (unsigned)d->Hkv * (unsigned long long)G * (unsigned)(d->d / 8);
        if (qchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        if ((d->Q == nullptr) != (d->Qout == nullptr)) return hipErrorInvalidValue;
        if (d->Q) {
            if (!packed_ok(d->Q, d->d, d->q_stride_t, d->q_stride_h) || !packed_ok(d->Qout, d->d, d->qo_stride_t, d->qo_stride_h))
                return hipErrorInvalidValue;
            const bool in_place = d->Q == d->Qout && d->q_stride_t == d->qo_stride_t && d->q_stride_h == d->qo_stride_h;
            const long long Hq = (long long)d->Hkv * G;
            if (!in_place && ranges_overlap(d->Q, packed_extent(d->total_new, Hq, d->d, d->q_stride_t, d->q_stride_h), d->Qout,
                                            packed_extent(d->total_new, Hq, d->d, d->qo_stride_t, d->qo_stride_h)))
                return hipErrorInvalidValue;
        }
    }
    const bool has_q = rope && d->Q;
    const unsigned kv_blocks = ((unsigned)chunks + kAppendThreads - 1) / kAppendThreads;
    const unsigned q_blocks = has_q ? (unsigned)((qchunks + kAppendThreads - 1) / kAppendThreads) : 0u;
    const VarlenAppendCall c = {
        d,
        {d->seqlens_k, d->block_table, d->k_scale, d->v_scale, (unsigned)chunks, d->Hkv, d->total_new, Ncap, paged ? d->max_pages : 0,
         paged ? d->num_pages : 0, lg_page},
        {d->rope_cos, d->rope_sin, has_q ? (unsigned)qchunks : 0u, kv_blocks, G, rope ? d->max_pos : 0, rope ? d->rot_dim / 2 : 0,
         rope ? d->rot_dim / 8 : 0},
        {d->cu_seqlens_new, d->B, d->total_new, d->k_stride_t / 8, d->k_stride_h / 8, d->v_stride_t / 8, d->v_stride_h / 8,
         has_q ? d->q_stride_t / 8 : 0, has_q ? d->q_stride_h / 8 : 0, has_q ? d->qo_stride_t / 8 : 0, has_q ? d->qo_stride_h / 8 : 0},
        2 * kv_blocks + q_blocks};   // at most 3 * 2^23 blocks
    return append_form(d->dtype, d->d, paged, fp8, [&](auto form) {
        return append_rope_mode(rope, d->interleaved != 0, [&](auto mode) {
            using F = decltype(form);
            if constexpr (mode() != 0)   // the position instantiations exist for the rotary forms only
                if (positions) return launch_varlen<F, mode()>(c, positions);
            return launch_varlen<F, mode()>(c);
        });
    });
}

hipError_t kvcache_append_varlen(const ::fa_kvappend_varlen_desc* d) { return append_varlen_checked(d, nullptr); }

hipError_t kvcache_append_varlen_ex(const ::fa_kvappend_varlen_desc* d, const ::fa_kvappend_varlen_opts* opts)
{
    if (opts && opts->size != sizeof(fa_kvappend_varlen_opts)) return hipErrorInvalidValue;
    return append_varlen_checked(d, opts ? opts->positions : nullptr);
}

}  // namespace fa
