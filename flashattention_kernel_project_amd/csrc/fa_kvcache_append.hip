// fa_kvcache_append.hip -- the write half of a decode step (fa_kvcache_append, _paged, _fp8, _paged_fp8): Nnew new K and V rows per
// sequence are copied behind the sequence's current length, into a contiguous cache or through a block table into a page pool, as
// they are or quantised to e4m3fn with the head's scale.  Lengths, table and scales are read on the device, so a captured
// append -> decode pair follows a growing cache.  DESIGN.md section 7.5 has the reasoning.  The device helpers are shared with the
// _rope entries' unit through fa_kvcache_append.hpp.
#include "fa_kvcache_append.hpp"

namespace fa {

// One thread moves one 16-byte chunk (8 elements) of a source row; blockIdx.y: 0 = K, 1 = V.  The source tensors are contiguous
// [B, Hkv, Nnew, D], so thread g of a tensor reads bytes [16 g, 16 g + 16): the loads of a wave are 1 KiB in a row.  Length, page
// number and scale are the same for the D / 8 threads of a row: each is fetched once by the row (one address per row, broadcast
// by the memory pipeline), never per element.  A token at or past the capacity, or in a page whose table entry is outside
// [0, num_pages), is dropped before any address is formed from it.
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

// The lengths after the append, min(L_b + Nnew, Ncap).  A kernel of its own behind the copy on the same stream: every read of
// seqlens by the copy has retired before this one starts, so `out` may be `in` itself.
__global__ void __launch_bounds__(kAppendThreads)
fa_kvcache_append_lens_kernel(const int* in, int* out, int B, int Nnew, int Ncap)
{
    const unsigned i = blockIdx.x * (unsigned)kAppendThreads + threadIdx.x;
    if (i >= (unsigned)B) return;
    int L = 0;
    if (in) {
        const int raw = in[i];
        L = raw < 0 ? 0 : (raw > Ncap ? Ncap : raw);
    }
    const long long n = (long long)L + Nnew;
    out[i] = n < Ncap ? (int)n : Ncap;
}

// the launch of the kernel above, for both append units; Ncap: the checked capacity
hipError_t kvcache_append_lens(const KvAppendArgs& a, int Ncap)
{
    if (!a.seqlens_out) return hipSuccess;
    FA_LAUNCH(fa_kvcache_append_lens_kernel, dim3(((unsigned)a.B + kAppendThreads - 1) / kAppendThreads), dim3(kAppendThreads), 0,
              a.stream, a.seqlens, a.seqlens_out, a.B, a.Nnew, Ncap);
    return launch_status();
}

template <typename T, int D, bool kPaged, bool kFp8>
static hipError_t launch_append(const KvAppendArgs& a, const AppendDev& dev)
{
    const unsigned blocks = (dev.chunks + kAppendThreads - 1) / kAppendThreads;   // from (B, Hkv, Nnew, D) alone
    FA_LAUNCH((fa_kvcache_append_kernel<T, D, kPaged, kFp8>), dim3(blocks, 2), dim3(kAppendThreads), 0, a.stream,
              static_cast<const uint16_t*>(a.Knew), static_cast<const uint16_t*>(a.Vnew), a.K, a.V, dev);
    const hipError_t e = launch_status();
    return e != hipSuccess ? e : kvcache_append_lens(a, dev.Ncap);
}

template <bool kPaged, bool kFp8>
static hipError_t append_types(const KvAppendArgs& a, const AppendDev& dev)
{
    // a 16-bit cache takes the source bits as they are: one instantiation serves fp16 and bf16
    if constexpr (kFp8)
        if (a.dtype == 1)
            return a.D == 64 ? launch_append<BF16, 64, kPaged, kFp8>(a, dev) : launch_append<BF16, 128, kPaged, kFp8>(a, dev);
    return a.D == 64 ? launch_append<F16, 64, kPaged, kFp8>(a, dev) : launch_append<F16, 128, kPaged, kFp8>(a, dev);
}

hipError_t kvcache_append_dispatch(const KvAppendArgs& a)
{
    if (a.Nnew <= 0) return hipErrorInvalidValue;
    // the decode entries' checks on the cache this append feeds (null pointers, B, Hkv, Ncap, d, dtype, the bound on Ncap; the page
    // geometry), with the new rows in the place of Q and O
    KvPagedArgs chk = {{a.Knew, a.K, a.V, const_cast<void*>(a.Vnew), nullptr, a.seqlens, a.B, a.Hkv, 1, 1, a.Ncap, a.D, 1.0f, 0, a.dtype, 0,
                        nullptr, 0, a.stream}, a.table, a.num_pages, a.page_size, a.max_pages};
    int lg_page = 0;
    KvPagedArgs with_cap = chk;
    const hipError_t bad = a.paged ? kvpaged_check(chk, with_cap, lg_page) : kvcache_check(chk.c);
    if (bad != hipSuccess) return bad;
    const int Ncap = with_cap.c.Ncap;
    // a thread's chunk number is 32 bit (so is the grid): sources of 2^31 chunks (32 GiB) and more per tensor are refused
    const unsigned long long chunks = (unsigned long long)a.B * a.Hkv * (unsigned long long)a.Nnew * (unsigned)(a.D / 8);
    if (chunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (a.seqlens_out && a.seqlens && a.seqlens_out != a.seqlens) {   // the same buffer or disjoint ones; never a partial overlap
        const uintptr_t in = reinterpret_cast<uintptr_t>(a.seqlens), out = reinterpret_cast<uintptr_t>(a.seqlens_out);
        const uintptr_t bytes = (uintptr_t)a.B * sizeof(int);
        if (in < out + bytes && out < in + bytes) return hipErrorInvalidValue;
    }
    // a token count per sequence: its own checks and kernels, rotary or not (fa_kvcache_append_ragged.hip)
    if (a.seqlens_new) return kvcache_append_ragged(a, Ncap, lg_page);
    if (a.rope) return kvcache_append_rope(a, Ncap, lg_page);   // its own checks, then its own kernels (fa_kvcache_append_rope.hip)
    const AppendDev dev = {a.seqlens, a.table, a.k_scale, a.v_scale, (unsigned)chunks, a.Hkv, a.Nnew, Ncap, a.max_pages, a.num_pages, lg_page};
    if (a.paged) return a.fp8 ? append_types<true, true>(a, dev) : append_types<true, false>(a, dev);
    return a.fp8 ? append_types<false, true>(a, dev) : append_types<false, false>(a, dev);
}

}  // namespace fa
