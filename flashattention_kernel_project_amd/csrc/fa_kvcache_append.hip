// fa_kvcache_append.hip -- the write half of a decode step (fa_kvcache_append, _paged, _fp8, _paged_fp8): Nnew new K and V rows per
// sequence are copied behind the sequence's current length, into a contiguous cache or through a block table into a page pool, as
// they are or quantised to e4m3fn with the head's scale.  Lengths, table and scales are read on the device, so a captured
// append -> decode pair follows a growing cache.  DESIGN.md section 7.5 has the reasoning.  Also here, for the whole write side
// (DESIGN.md 7.23): the lengths kernel behind every append's copy, the cache check and the rotary-argument check.
#include "fa_kvcache_append.hpp"

#include <limits.h>

namespace fa {

// One thread moves one 16-byte chunk (8 elements) of a source row; blockIdx.y: 0 = K, 1 = V.  The source tensors are contiguous
// [B, Hkv, Nnew, D], so thread g of a tensor reads bytes [16 g, 16 g + 16): the loads of a wave are 1 KiB in a row.  Length, page
// number and scale are the same for the D / 8 threads of a row: each is fetched once by the row (one address per row, broadcast
// by the memory pipeline), never per element.  A token at or past the capacity, or in a page whose table entry is outside
// [0, num_pages), is dropped before any address is formed from it.  The body is written out, not put together from append_len,
// append_page, append_dst_row and append_chunk of the header as every other copy kernel is: through any of them the fp8 kernels
// of this unit come out in another instruction order, and the flat append is the one the decode step's time was measured with.
template <typename T, int D, bool kPaged, bool kFp8>
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_kernel(const uint16_t* __restrict__ Knew, const uint16_t* __restrict__ Vnew, void* __restrict__ Kdst,
                         void* __restrict__ Vdst, AppendDev a)
{
    constexpr int kLgChunks = D == 64 ? 3 : 4;   // log2 of the 16-byte chunks per row
    const unsigned g = blockIdx.x * (unsigned)kAppendThreads + threadIdx.x;
    if (g >= a.chunks) return;
    const bool is_v = blockIdx.y != 0;
    const unsigned row = g >> kLgChunks, c = g & ((1u << kLgChunks) - 1);
    const unsigned bh = row / (unsigned)a.Nnew, t = row - bh * (unsigned)a.Nnew;
    const unsigned b = bh / (unsigned)a.Hkv, h = bh - b * (unsigned)a.Hkv;
    unsigned L = 0;
    if (a.seqlens) {
        const int raw = a.seqlens[b];
        L = (unsigned)(raw < 0 ? 0 : (raw > a.Ncap ? a.Ncap : raw));
    }
    const unsigned p = L + t;   // L <= Ncap < 2^31 and t < Nnew < 2^31: no wrap
    if (p >= (unsigned)a.Ncap) return;
    size_t dst_row;             // destination row, counted in rows of D elements
    if constexpr (kPaged) {
        const int page = a.table[(size_t)b * (unsigned)a.max_pages + (p >> a.lg_page)];   // p < Ncap: inside the table's row
        if ((unsigned)page >= (unsigned)a.num_pages) return;
        dst_row = (((size_t)(unsigned)page * (unsigned)a.Hkv + h) << a.lg_page) + (p & ((1u << a.lg_page) - 1));   // 64 bit: pools exceed 4 GiB
    } else {
        dst_row = (size_t)bh * (unsigned)a.Ncap + p;
    }
    const u32x4* src = reinterpret_cast<const u32x4*>(is_v ? Vnew : Knew) + g;
    constexpr bool kNt = FA_APPEND_NT_LOAD >= (kFp8 ? 2 : 1);
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
}

// The lengths after an append, min(L_i + m_i, cap), for all four append kernels: m_i from the clamped bounds of `cu` (n: the total),
// else the clamped count, else n.  A kernel of its own behind the copy on the same stream: every read of the lengths by the copy
// has retired before this one starts, so `out` may be `in` itself; `cnt` and `cu` never overlap `out` (checked on the host).
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_lens_kernel(const int* in, const int* __restrict__ cnt, const int* __restrict__ cu, int* out, int B, int n, int cap)
{
    const unsigned i = blockIdx.x * (unsigned)kAppendThreads + threadIdx.x;
    if (i >= (unsigned)B) return;
    const unsigned L = append_len(in, cap, i);
    unsigned m = (unsigned)n;
    if (cu) {
        const unsigned s = cu_at(cu, i, n), e = cu_at(cu, i + 1, n);
        m = e > s ? e - s : 0u;
    } else if (cnt) {
        const int raw = cnt[i];
        m = (unsigned)(raw < 0 ? 0 : (raw > n ? n : raw));
    }
    const long long sum = (long long)L + m;
    out[i] = sum < cap ? (int)sum : cap;
}

hipError_t kvappend_lens(const int* in, const int* cnt, const int* cu, int* out, int B, int n, int cap, hipStream_t stream)
{
    if (!out) return hipSuccess;
    FA_LAUNCH(fa_kvcache_append_lens_kernel, dim3(((unsigned)B + kAppendThreads - 1) / kAppendThreads), dim3(kAppendThreads), 0, stream, in,
              cnt, cu, out, B, n, cap);
    return launch_status();
}

hipError_t kvwrite_check(const KvWriteCache& w, int& Ncap, int& lg_page)
{
    // null pointers, B, Hkv, the capacity and its bound, d, dtype; the page geometry
    const KvPagedArgs chk = {.c = {.Q = w.src_k, .K = w.K, .V = w.V, .O = const_cast<void*>(w.src_v), .seqlens = w.seqlens, .B = w.B,
                                   .Hkv = w.Hkv, .G = 1, .Nq = 1, .Ncap = w.paged ? 0 : w.Ncap, .D = w.D, .scale = 1.0f, .in_dtype = w.dtype},
                             .table = w.table, .num_pages = w.paged ? w.num_pages : 0, .page_size = w.paged ? w.page_size : 0,
                             .max_pages = w.paged ? w.max_pages : 0};
    KvPagedArgs with_cap = chk;
    lg_page = 0;
    const hipError_t bad = w.paged ? kvpaged_check(chk, with_cap, lg_page) : kvcache_check(chk.c);
    Ncap = with_cap.c.Ncap;
    return bad;
}

hipError_t kvappend_rope_check(const float* cos, const float* sin, int rot_dim, int D, int max_pos, int G, int interleaved, long long heads)
{
    if (!cos || !sin) return hipErrorInvalidValue;
    if (rot_dim < 16 || rot_dim > D || rot_dim % 16 != 0) return hipErrorInvalidValue;
    if (max_pos <= 0 || G <= 0 || (interleaved != 0 && interleaved != 1)) return hipErrorInvalidValue;
    return heads * G > (long long)INT_MAX ? hipErrorInvalidValue : hipSuccess;   // heads fits an int (kvcache_check): no wrap
}

hipError_t kvcache_append_dispatch(const KvAppendArgs& a)
{
    if (a.Nnew <= 0) return hipErrorInvalidValue;
    int Ncap = 0, lg_page = 0;
    const hipError_t bad = kvwrite_check({.src_k = a.Knew, .src_v = a.Vnew, .K = a.K, .V = a.V, .seqlens = a.seqlens, .table = a.table,
                                          .B = a.B, .Hkv = a.Hkv, .Ncap = a.Ncap, .D = a.D, .dtype = a.dtype, .num_pages = a.num_pages,
                                          .page_size = a.page_size, .max_pages = a.max_pages, .paged = a.paged}, Ncap, lg_page);
    if (bad != hipSuccess) return bad;
    // a thread's chunk number is 32 bit (so is the grid): sources of 2^31 chunks (32 GiB) and more per tensor are refused
    const unsigned long long chunks = (unsigned long long)a.B * a.Hkv * (unsigned long long)a.Nnew * (unsigned)(a.D / 8);
    if (chunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (!lens_out_ok(a.seqlens, a.seqlens_out, a.B, a.seqlens_new, (size_t)a.B * sizeof(int))) return hipErrorInvalidValue;
    // a rotation or a token count per sequence: their own checks and kernels (fa_kvcache_append_padded.hip)
    if (a.seqlens_new || a.rope) return kvcache_append_padded(a, Ncap, lg_page);
    const AppendDev dev = {a.seqlens, a.table, a.k_scale, a.v_scale, (unsigned)chunks, a.Hkv, a.Nnew, Ncap, a.max_pages, a.num_pages, lg_page};
    return append_form(a.dtype, a.D, a.paged, a.fp8, [&](auto form) {
        using F = decltype(form);
        // a 16-bit cache takes the source bits as they are: the F16 instantiation serves fp16 and bf16
        using T = std::conditional_t<F::kFp8, typename F::T, F16>;
        const unsigned blocks = (dev.chunks + kAppendThreads - 1) / kAppendThreads;   // from (B, Hkv, Nnew, D) alone
        FA_LAUNCH((fa_kvcache_append_kernel<T, F::D, F::kPaged, F::kFp8>), dim3(blocks, 2), dim3(kAppendThreads), 0, a.stream,
                  static_cast<const uint16_t*>(a.Knew), static_cast<const uint16_t*>(a.Vnew), a.K, a.V, dev);
        const hipError_t e = launch_status();
        return e != hipSuccess ? e : kvappend_lens(a.seqlens, nullptr, nullptr, a.seqlens_out, a.B, a.Nnew, Ncap, a.stream);
    });
}

}  // namespace fa
