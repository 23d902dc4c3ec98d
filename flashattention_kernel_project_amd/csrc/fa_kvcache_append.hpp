// fa_kvcache_append.hpp -- what the write side of the KV cache shares.  Three append translation units (fa_kvcache_append.hip: the
// plain entries, the lengths kernel and the host checks of all; fa_kvcache_append_padded.hip: the padded entries that rotate or
// take a token count per sequence; fa_kvcache_append_varlen.hip: token-packed sources), fa_mla_append.hip and fa_kvcache_commit.hip
// take from here, on the device: the kernels' argument pack, the length clamp, the page lookup with its 64-bit destination row, the
// search of cu_seqlens_new, the e4m3fn quantisation, the store of one chunk and the rotation of one; on the host: the form switch
// and the interval test.  Private to csrc/.  Everything is in an unnamed namespace: each unit gets its own copy and all of it is
// inlined.  DESIGN.md section 7.23 has the map.
#pragma once
#include "fa_dispatch.hpp"

// Non-temporal hint on the source loads (read once): 1 = on the 16-bit copy only, where it measured 7-13 % faster at Nnew = 4096;
// 2 = on the fp8 kernels too (measured: no gain); 0 = nowhere.  Never on the stores: at Nnew = 1 the decode that follows reads them.
#ifndef FA_APPEND_NT_LOAD
#define FA_APPEND_NT_LOAD 1
#endif

namespace fa {

namespace {

struct AppendDev {
    const int* seqlens;     // [B] on the device, or nullptr: every sequence is EMPTY (a prefill into a fresh cache)
    const int* table;       // [B][max_pages] page numbers on the device (paged only)
    const float* k_scale;   // [Hkv] on the device, or nullptr (1.0) (fp8 only)
    const float* v_scale;
    unsigned chunks;        // 16-byte source chunks per tensor: B * Hkv * Nnew * D / 8
    int Hkv, Nnew, Ncap;
    int max_pages, num_pages, lg_page;
};

constexpr int kAppendThreads = 256;
constexpr float kE4m3Max = 448.0f;

// A quotient x / s made ready for the conversion: a NaN is taken out (its code is set by nan_code below) and the rest is clamped to
// +-448, so what reaches the conversion is finite and in range and neither the clamp's nor the conversion's treatment of NaN and
// overflow matters.
__device__ __forceinline__ float quant_operand(float q)
{
    q = (q != q) ? 0.0f : q;
    q = q > kE4m3Max ? kE4m3Max : q;
    return q < -kE4m3Max ? -kE4m3Max : q;
}
// 0x7F in byte `i` where the quotient is a NaN (OR-ed over the converted code: 0x7F or 0xFF, both NaN in e4m3fn)
__device__ __forceinline__ unsigned nan_code(float q, int i) { return (q != q) ? (0x7Fu << (8 * i)) : 0u; }
// the four quotients q_i = x_i / s -> four e4m3fn codes, round to nearest even (v_cvt_pk_fp8_f32: OCP e4m3fn on gfx950)
__device__ __forceinline__ unsigned quant_codes(float q0, float q1, float q2, float q3)
{
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(quant_operand(q0), quant_operand(q1), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(quant_operand(q2), quant_operand(q3), w, true);
    return (unsigned)w | nan_code(q0, 0) | nan_code(q1, 1) | nan_code(q2, 2) | nan_code(q3, 3);
}
// four elements of T (two packed words) -> four e4m3fn codes of x / s
template <typename T> __device__ __forceinline__ unsigned quant4(unsigned w0, unsigned w1, float s)
{
    // exact widening, then IEEE division (v_div_scale / v_div_fmas / v_div_fixup; fp32 denormals kept), never a reciprocal
    const float q0 = T::lo(w0) / s, q1 = T::hi(w0) / s, q2 = T::lo(w1) / s, q3 = T::hi(w1) / s;
    return quant_codes(q0, q1, q2, q3);
}
// the same of four fp32 values (the rotated K of the _rope entries)
__device__ __forceinline__ unsigned quant4f(float x0, float x1, float x2, float x3, float s)
{
    return quant_codes(x0 / s, x1 / s, x2 / s, x3 / s);
}

// The position helpers of every kernel but fa_kvcache_append_kernel, which keeps the same three steps written out in its body:
// called through these (by reference or by value) its fp8 kernels come out with another instruction order, and that unit's device
// code is to stay as measured (profiles/kvcache_append_rope.txt has the diff).

// L_b = min(max(seqlens[b], 0), Ncap); no lengths: 0
__device__ __forceinline__ unsigned append_len(const int* seqlens, int Ncap, unsigned b)
{
    unsigned L = 0;
    if (seqlens) {
        const int raw = seqlens[b];
        L = (unsigned)(raw < 0 ? 0 : (raw > Ncap ? Ncap : raw));
    }
    return L;
}
// The page of key position p < Ncap of sequence b (p < Ncap: inside the table's row).  A number outside [0, num_pages) drops the
// token before any address is formed from it.
__device__ __forceinline__ int append_page(const int* table, int max_pages, int lg_page, unsigned b, unsigned p)
{
    return table[(size_t)b * (unsigned)max_pages + (p >> lg_page)];
}
// The destination row of position p of K/V head h of sequence b (bh = b * Hkv + h), counted in rows of D elements; `page` (paged
// only) is inside [0, num_pages).  64 bit: pools exceed 4 GiB.
template <bool kPaged>
__device__ __forceinline__ size_t append_dst_row(int page, int Hkv, int lg_page, int Ncap, unsigned h, unsigned bh, unsigned p)
{
    if constexpr (kPaged)
        return (((size_t)(unsigned)page * (unsigned)Hkv + h) << lg_page) + (p & ((1u << lg_page) - 1));
    return (size_t)bh * (unsigned)Ncap + p;
}

// One 16-byte chunk of a row that is not rotated: `src` is the chunk's source address, `dst` the tensor's base, `scale` the tensor's
// [Hkv] scales or null (1.0).  The copy, or the quantisation by the head's scale.  fa_kvcache_append_kernel keeps these lines
// written out as well: through this call its code changes (profiles/append_write_refactor.txt).
template <typename T, int D, bool kFp8>
__device__ __forceinline__ void append_chunk(const u32x4* src, char* dst, size_t dst_row, unsigned c, const float* scale, unsigned h)
{
    constexpr bool kNt = FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1);
    const u32x4 v = kNt ? __builtin_nontemporal_load(src) : *src;
    if constexpr (kFp8) {
        const float s = scale ? scale[h] : 1.0f;
        const u32x2 o = {quant4<T>(v[0], v[1], s), quant4<T>(v[2], v[3], s)};
        *reinterpret_cast<u32x2*>(dst + dst_row * D + c * 8) = o;
    } else {
        *reinterpret_cast<u32x4*>(dst + dst_row * (D * 2) + c * 16) = v;
    }
}

// ---- token-packed sources (fa_kvcache_append_varlen.hip, fa_mla_append.hip): the sequence of a row, from cu_seqlens_new ----

// cu[j] clamped into [0, total]
__device__ __forceinline__ unsigned cu_at(const int* cu, unsigned j, int total)
{
    const int raw = cu[j];
    return (unsigned)(raw < 0 ? 0 : (raw > total ? total : raw));
}

// The largest b in [0, B) whose clamped start is <= t (0 when none is): log2(B) reads of cu, every index inside [0, B).  Among
// sequences that start at one row -- empty ones and the one behind them -- this is the last, the only one that can own the row.
__device__ __forceinline__ unsigned seq_search(const int* cu, unsigned B, int total, unsigned t)
{
    unsigned lo = 0, hi = B;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (cu_at(cu, mid, total) <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// Does sequence b own row t?  s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b+1], s_b, total): on true, s <= t < e <= total.
__device__ __forceinline__ bool seq_owns(const int* cu, unsigned b, int total, unsigned t, unsigned& s)
{
    s = cu_at(cu, b, total);
    const unsigned e = cu_at(cu, b + 1, total);   // e < s (a non-monotone vector) owns nothing: t >= s excludes t < e
    return s <= t && t < e;
}

// ---- the rotary part: fa_kvcache_append_padded.hip and fa_kvcache_append_varlen.hip ----

struct RopeDev {
    const float* cos;      // [max_pos][half] fp32 on the device
    const float* sin;
    unsigned qchunks;      // 16-byte chunks of Q: B * Hkv * G * Nnew * D / 8 (0: no Q)
    unsigned kv_blocks;    // workgroups per K/V tensor
    int G, max_pos;
    int half;              // rot_dim / 2: pairs per row = fp32 per table row
    int rot_chunks;        // rot_dim / 8: the 16-byte chunks of a row that are rotated
};

// four table values from a row, 4-byte aligned like the caller's table (no hint: the row serves every head of the sequence)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// own * c + other * s with each product and the sum rounded to fp32 on its own.  a - b is a + (-b) for every input, and
// fp32((-x) * s) is -fp32(x * s), so the pair's first element passes `other` negated: y1 = x1 c - x2 s, y2 = x2 c + x1 s.
__device__ __forceinline__ float rope1(float own, float other, float c, float s)
{
#pragma clang fp contract(off)   // no fused multiply-add, whatever the including unit's setting
    const float a = own * c;
    const float b = other * s;
    return a + b;
}

template <typename T> __device__ __forceinline__ void widen8(const u32x4 v, float (&x)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = T::lo(v[i]);
        x[2 * i + 1] = T::hi(v[i]);
    }
}

// Eight rotated fp32 values leave as one chunk: 16 bytes of T (one rounding to nearest even) for Q and a 16-bit cache, 8 bytes of
// e4m3fn codes of y / s for an fp8 cache (no 16-bit rounding in between).  `dst` is the chunk's address.
template <typename T, bool kCodes> __device__ __forceinline__ void store8(char* dst, const float (&y)[8], float s)
{
    if constexpr (kCodes) {
        const u32x2 o = {quant4f(y[0], y[1], y[2], y[3], s), quant4f(y[4], y[5], y[6], y[7], s)};
        *reinterpret_cast<u32x2*>(dst) = o;
    } else {
        const u32x4 o = {T::pack2(y[0], y[1]), T::pack2(y[2], y[3]), T::pack2(y[4], y[5]), T::pack2(y[6], y[7])};
        *reinterpret_cast<u32x4*>(dst) = o;
    }
}

// Chunk c of one K or Q row at position p: `src` is the chunk's source address, `dst_row` the first byte of the destination row.
// kCodes: the destination holds e4m3fn codes of y / s (8 bytes per chunk), else T (16 bytes per chunk; s is unused).
template <typename T, bool kCodes, bool kInterleaved, bool kNt>
__device__ __forceinline__ void rope_row(const u32x4* src, char* dst_row, unsigned c, unsigned p, float s, const RopeDev& r)
{
    constexpr unsigned kOut = kCodes ? 8 : 16;   // bytes per chunk at the destination
    const unsigned rot_chunks = (unsigned)r.rot_chunks, half_chunks = rot_chunks / 2;
    if (!kInterleaved && c >= half_chunks && c < rot_chunks) return;   // a pair's second chunk: the first one's thread has it
    const u32x4 v = kNt ? __builtin_nontemporal_load(src) : *src;
    if (c >= rot_chunks) {   // the pass-through part: every bit kept in 16 bit, quantised as the plain entry does on an fp8 cache
        if constexpr (kCodes) {
            const u32x2 o = {quant4<T>(v[0], v[1], s), quant4<T>(v[2], v[3], s)};
            *reinterpret_cast<u32x2*>(dst_row + c * 8) = o;
        } else {
            *reinterpret_cast<u32x4*>(dst_row + c * 16) = v;
        }
        return;
    }
    const unsigned tr = p < (unsigned)r.max_pos ? p : (unsigned)r.max_pos - 1;   // clamp, never fault
    const size_t trow = (size_t)tr * (unsigned)r.half;
    float x[8], y[8];
    widen8<T>(v, x);
    if constexpr (kInterleaved) {
        const f32x4u cs = *reinterpret_cast<const f32x4u*>(r.cos + trow + c * 4);
        const f32x4u sn = *reinterpret_cast<const f32x4u*>(r.sin + trow + c * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[2 * i] = rope1(x[2 * i], -x[2 * i + 1], cs[i], sn[i]);
            y[2 * i + 1] = rope1(x[2 * i + 1], x[2 * i], cs[i], sn[i]);
        }
        store8<T, kCodes>(dst_row + c * kOut, y, s);
    } else {
        const u32x4 v2 = kNt ? __builtin_nontemporal_load(src + half_chunks) : src[half_chunks];
        float x2[8], y2[8];
        widen8<T>(v2, x2);
        const f32x4u cs0 = *reinterpret_cast<const f32x4u*>(r.cos + trow + c * 8);
        const f32x4u cs1 = *reinterpret_cast<const f32x4u*>(r.cos + trow + c * 8 + 4);
        const f32x4u sn0 = *reinterpret_cast<const f32x4u*>(r.sin + trow + c * 8);
        const f32x4u sn1 = *reinterpret_cast<const f32x4u*>(r.sin + trow + c * 8 + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float cc = i < 4 ? cs0[i & 3] : cs1[i & 3], ss = i < 4 ? sn0[i & 3] : sn1[i & 3];
            y[i] = rope1(x[i], -x2[i], cc, ss);
            y2[i] = rope1(x2[i], x[i], cc, ss);
        }
        store8<T, kCodes>(dst_row + c * kOut, y, s);
        store8<T, kCodes>(dst_row + (c + half_chunks) * kOut, y2, s);
    }
}

// ---- the host side ----

// Do [x, x + xbytes) and [y, y + ybytes) share a byte?  Each caller states its own rule around it: identity allowed, or not.
inline bool ranges_overlap(const void* x, size_t xbytes, const void* y, size_t ybytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y);
    return a < b + ybytes && b < a + xbytes;
}

// The rule of every lengths kernel's buffers: what it reads besides `in` -- counts, bounds, accept words; null: nothing -- shares no
// byte with `out`, identity included, and `in` is `out` itself or shares no byte with it.  No `out`: nothing is written.
inline bool lens_out_ok(const int* in, const int* out, int B, const void* also, size_t also_bytes)
{
    const size_t bytes = (size_t)B * sizeof(int);
    if (!out) return true;
    if (also && ranges_overlap(also, also_bytes, out, bytes)) return false;
    return !in || in == out || !ranges_overlap(in, bytes, out, bytes);
}

// The KvWriteCache of a descriptor (fa_kvappend_varlen_desc, fa_kvcommit_desc: one set of field names); a block table makes it paged.
template <typename Desc> KvWriteCache write_cache_of(const Desc& d, const void* src_k, const void* src_v)
{
    return {src_k, src_v, d.K, d.V, d.seqlens_k, d.block_table, d.B, d.Hkv, d.Ncap, d.d, d.dtype, d.num_pages, d.page_size, d.max_pages,
            d.block_table != nullptr};
}

// The form of a copy kernel as compile-time tags: the source's element type, the row length, the cache's addressing and element.
template <typename T_, int D_, bool kPaged_, bool kFp8_> struct AppendForm {
    using T = T_;
    static constexpr int D = D_;
    static constexpr bool kPaged = kPaged_, kFp8 = kFp8_;
};
template <typename F> hipError_t on_flag(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// (dtype, D, paged, fp8) of a checked call -> f(AppendForm<...>{}): the one switch of the three append units
template <typename F> hipError_t append_form(int dtype, int D, bool paged, bool fp8, F&& f)
{
    return on_flag(dtype == 1, [&](auto bf) {
        return on_flag(D == 64, [&](auto d64) {
            return on_flag(paged, [&](auto pg) {
                return on_flag(fp8, [&](auto q) { return f(AppendForm<std::conditional_t<bf(), BF16, F16>, d64() ? 64 : 128, pg(), q()>{}); });
            });
        });
    });
}
// the rotary mode of a call -> f(integral constant): 0 no rotation, 1 half-split pairs, 2 interleaved pairs
template <typename F> hipError_t append_rope_mode(bool rope, bool interleaved, F&& f)
{
    if (!rope) return f(std::integral_constant<int, 0>{});
    return interleaved ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 1>{});
}

}  // namespace

}  // namespace fa
