// fa_mla_append.hip -- fa_mla_append: the write half of fa_mla_decode.  A token-packed batch of latent rows (total_new, 576), read
// through its token stride and cut into sequences by cu_seqlens_new on the device, is copied bit for bit behind each sequence's keys
// in the latent cache, contiguous or paged.  A copy kernel on the model of fa_kvcache_append_varlen.hip, on the same helpers of
// fa_kvcache_append.hpp: one thread per 16-byte chunk, the row's sequence found by a search of cu_seqlens_new, and the appends'
// lengths kernel behind the copy.  No rotary and no heads: a latent row is one row for all heads and arrives rotated.
// fa_mla_append_fp8 is the same kernel with the store changed (kFp8): the chunk's 8 elements leave as 8 e4m3fn codes of x / c_scale,
// through the write side's quant4, into rows of 576 bytes.  DESIGN.md sections 7.22 and 7.24.
#include "../../include/fa_mi355.h"
#include "fa_kvcache_append.hpp"

namespace fa {

namespace {

constexpr int kMlaAppendThreads = 256;
constexpr unsigned kMlaChunks = FA_MLA_DQK / 8;   // 72 16-byte chunks per latent row

struct MlaAppendDev {
    const u32x4* src;      // Cnew
    char* dst;             // C
    const int *cu, *seqlens, *table;
    int B, total, cap;
    int max_pages, num_pages, lg_page;   // paged only
    long long st;          // the token stride of Cnew in 16-byte chunks
    unsigned chunks;       // total * 72
    const float* c_scale;  // kFp8 only: the cache's one scale on the device, or nullptr (1.0)
};

}  // namespace

// A row that no sequence owns retires before anything is loaded; so does a token at or past the capacity, and one whose page number
// lies outside the pool -- no address is formed from it.
// kFp8: T is Cnew's type and the chunk is quantised on its way out; else the copy, which does not look at the elements.
template <bool kPaged, bool kFp8, typename T>
__global__ void __launch_bounds__(kMlaAppendThreads)
fa_mla_append_kernel(MlaAppendDev a)
{
    const unsigned g = blockIdx.x * (unsigned)kMlaAppendThreads + threadIdx.x;
    if (g >= a.chunks) return;
    const unsigned t = g / kMlaChunks, c = g - t * kMlaChunks;
    const unsigned b = seq_search(a.cu, (unsigned)a.B, a.total, t);
    const unsigned s = cu_at(a.cu, b, a.total), e = cu_at(a.cu, b + 1, a.total);
    if (!(s <= t && t < e)) return;                             // a row of no sequence (e < s owns nothing)
    const unsigned p = append_len(a.seqlens, a.cap, b) + (t - s);  // L <= cap <= 2^30 and t - s < 2^24: no wrap
    if (p >= (unsigned)a.cap) return;                           // dropped
    size_t row;
    if constexpr (kPaged) {
        const int page = append_page(a.table, a.max_pages, a.lg_page, b, p);
        if ((unsigned)page >= (unsigned)a.num_pages) return;
        row = ((size_t)(unsigned)page << a.lg_page) + (p & ((1u << a.lg_page) - 1u));
    } else {
        row = (size_t)b * (unsigned)a.cap + p;
    }
    const u32x4 v = __builtin_nontemporal_load(a.src + ((size_t)t * (size_t)a.st + c));
    if constexpr (kFp8) {
        const float s8 = a.c_scale ? *a.c_scale : 1.0f;
        const u32x2 codes = {quant4<T>(v[0], v[1], s8), quant4<T>(v[2], v[3], s8)};
        *reinterpret_cast<u32x2*>(a.dst + (row * kMlaChunks + c) * 8u) = codes;   // row * 576 + c * 8
    } else {
        *reinterpret_cast<u32x4*>(a.dst + (row * kMlaChunks + c) * 16u) = v;
    }
}

namespace {

// both entries: the checks and the two launches (c_scale is looked at with fp8 only)
hipError_t mla_append_any(const ::fa_mla_append_desc* d, bool fp8, const float* c_scale)
{
    if (!d || d->size != sizeof(fa_mla_append_desc)) return hipErrorInvalidValue;
    if (!d->Cnew || !d->C || !d->cu_seqlens_new) return hipErrorInvalidValue;
    if (d->B <= 0 || d->total_new <= 0 || d->total_new > (1 << 24)) return hipErrorInvalidValue;   // a thread's chunk number is 32 bit
    if (d->dtype != FA_DTYPE_F16 && d->dtype != FA_DTYPE_BF16) return hipErrorInvalidValue;
    int cap = 0, lg_page = 0;
    if (!mla_geometry(d->block_table, d->Ncap, d->num_pages, d->page_size, d->max_pages, cap, lg_page)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d->Cnew) | reinterpret_cast<uintptr_t>(d->C)) & 15u) return hipErrorInvalidValue;
    if (fp8 && (reinterpret_cast<uintptr_t>(c_scale) & 3u)) return hipErrorInvalidValue;
    if (d->new_stride_t < FA_MLA_DQK || d->new_stride_t % 8) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d->cu_seqlens_new) | reinterpret_cast<uintptr_t>(d->seqlens_k) | reinterpret_cast<uintptr_t>(d->seqlens_out)) & 3u)
        return hipErrorInvalidValue;
    if (!lens_out_ok(d->seqlens_k, d->seqlens_out, d->B, d->cu_seqlens_new, ((size_t)d->B + 1) * sizeof(int))) return hipErrorInvalidValue;
    const bool paged = d->block_table != nullptr;
    const unsigned chunks = (unsigned)d->total_new * kMlaChunks;
    const MlaAppendDev a = {static_cast<const u32x4*>(d->Cnew), static_cast<char*>(d->C), d->cu_seqlens_new, d->seqlens_k, d->block_table,
                            d->B, d->total_new, cap, paged ? d->max_pages : 0, paged ? d->num_pages : 0, lg_page, d->new_stride_t / 8,
                            chunks, fp8 ? c_scale : nullptr};
    hipStream_t stream = static_cast<hipStream_t>(d->stream);
    const dim3 grid((chunks + kMlaAppendThreads - 1) / kMlaAppendThreads), block(kMlaAppendThreads);
    void (*kernel)(MlaAppendDev);
    if (!fp8) kernel = paged ? fa_mla_append_kernel<true, false, F16> : fa_mla_append_kernel<false, false, F16>;
    else if (d->dtype == FA_DTYPE_BF16) kernel = paged ? fa_mla_append_kernel<true, true, BF16> : fa_mla_append_kernel<false, true, BF16>;
    else kernel = paged ? fa_mla_append_kernel<true, true, F16> : fa_mla_append_kernel<false, true, F16>;
    FA_LAUNCH(kernel, grid, block, 0, stream, a);
    const hipError_t e = launch_status();
    return e != hipSuccess ? e : kvappend_lens(d->seqlens_k, nullptr, d->cu_seqlens_new, d->seqlens_out, d->B, d->total_new, cap, stream);
}

}  // namespace

hipError_t mla_append_dispatch(const ::fa_mla_append_desc* d) { return mla_append_any(d, false, nullptr); }

hipError_t mla_append_fp8_dispatch(const ::fa_mla_append_desc* d, const float* c_scale) { return mla_append_any(d, true, c_scale); }

}  // namespace fa
