// fa_kvcache_append.hpp -- the device side the four append translation units share (fa_kvcache_append.hip: the plain entries;
// fa_kvcache_append_rope.hip: the _rope entries; fa_kvcache_append_ragged.hip: fa_kvcache_append_ex with a token count per sequence;
// fa_kvcache_append_varlen.hip: fa_kvcache_append_varlen on token-packed sources):
// the kernels' argument pack, the length clamp, the page lookup with its 64-bit destination row, the e4m3fn quantisation, and the
// rotation of one row chunk.  fa_kvcache_commit.hip, which moves rows the appends placed, takes the clamp and the page lookup from here
// too.  Private to csrc/.  Everything is in an unnamed namespace: each unit gets its own
// copy, all of it is inlined, and the kernels' symbols stay what they were when the helpers lived in fa_kvcache_append.hip.
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

// The position helpers of the _rope kernel.  fa_kvcache_append_kernel keeps the same three steps written out in its body: called
// through these (by reference or by value) its fp8 kernels come out with another instruction order, and that unit's device code
// is to stay as measured (profiles/kvcache_append_rope.txt has the diff).

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

// ---- the rotary part: shared by fa_kvcache_append_rope.hip and fa_kvcache_append_ragged.hip ----

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

}  // namespace

}  // namespace fa
