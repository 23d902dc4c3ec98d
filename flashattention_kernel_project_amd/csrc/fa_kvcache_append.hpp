// fa_kvcache_append.hpp -- the device side the two append translation units share (fa_kvcache_append.hip: the plain entries;
// fa_kvcache_append_rope.hip: the _rope entries): the kernels' argument pack, the length clamp, the page lookup with its 64-bit
// destination row, and the e4m3fn quantisation.  Private to csrc/.  Everything is in an unnamed namespace: each unit gets its own
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

}  // namespace

}  // namespace fa
