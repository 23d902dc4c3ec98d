// fa_kvcache_commit.hip -- fa_kvcache_commit: the commit step of tree speculation.  fa_kvcache_append_varlen_ex put a step's tokens at
// slots L_b .. L_b + n_b - 1 in tree order; after verification one root-to-node path is kept, named by one 64-bit word per sequence,
// and this entry moves that path's K/V rows to the consecutive slots L_b .. L_b + a_b - 1 and writes the new lengths.  One kernel
// template serves the four cache forms (contiguous or paged; the element size is all that a 16-bit or e4m3fn cache differs in) on the
// position helpers of fa_kvcache_append.hpp.  DESIGN.md section 7.19.
#include "../../include/fa_mi355.h"
#include "fa_kvcache_append.hpp"

namespace fa {

namespace {

constexpr int kCommitThreads = 256;
constexpr int kCommitRows = 64;   // the bits of a word: the most rows a sequence moves

struct CommitDev {
    const int* seqlens;                   // [B] on the device, or nullptr: every L_b is 0
    const unsigned long long* words;      // [B] on the device
    const int* table;                     // [B][max_pages] on the device (paged only)
    int Hkv, Ncap, max_new;               // Ncap: the capacity, of a pool max_pages * page_size
    int max_pages, num_pages, lg_page;
};

// w_b: the word without the bits at or above max_new and without the bits of tokens the append dropped at the capacity (L <= cap)
__device__ __forceinline__ unsigned long long commit_word(const CommitDev& a, unsigned b, unsigned L)
{
    const unsigned room = (unsigned)a.Ncap - L;
    const unsigned n = room < (unsigned)a.max_new ? room : (unsigned)a.max_new;   // 0 .. 64
    const unsigned long long keep = n >= 64 ? ~0ull : ((1ull << n) - 1);
    return a.words[b] & keep;
}

}  // namespace

// One workgroup per (sequence, K/V head, tensor): grid (B * Hkv, 2).  A row is 1 << kLgChunks chunks of 16 bytes; item g of the
// workgroup is chunk g % chunks of move g / chunks, so a wave reads whole source rows and writes consecutive destination rows, both
// in full 16-byte lanes.  The 64 moves of the widest row (16 chunks) are 1024 items: four per thread, held in registers across the
// barrier that stands between the last load and the first store -- slot L + 1 of the word {1,3} is the source of move 0 and the
// destination of move 1, in two different threads.
// K and V are read and written through the same pointer: no __restrict__.
template <int kLgChunks, bool kPaged>
__global__ void __launch_bounds__(kCommitThreads)
fa_kvcache_commit_kernel(void* K, void* V, CommitDev a)
{
    constexpr unsigned kChunks = 1u << kLgChunks;
    constexpr int kItems = kCommitRows * (int)kChunks / kCommitThreads;   // 1, 2 or 4 per thread
    static_assert(kItems >= 1 && kItems * kCommitThreads == kCommitRows * (int)kChunks, "whole items per thread");
    __shared__ unsigned char src_of[kCommitRows];   // i_j: the bit of rank j

    const unsigned bh = blockIdx.x, b = bh / (unsigned)a.Hkv, h = bh - b * (unsigned)a.Hkv;
    const unsigned L = append_len(a.seqlens, a.Ncap, b);
    const unsigned long long w = commit_word(a, b, L);
    // a low-bit prefix (0 included): every move is i_j == j.  Uniform over the workgroup, ahead of both barriers; no table entry and
    // no cache byte is read.
    if ((w & (w + 1)) == 0) return;
    const unsigned t = threadIdx.x;
    if (t < (unsigned)kCommitRows && ((w >> t) & 1)) src_of[__popcll(w & ((1ull << t) - 1))] = (unsigned char)t;
    __syncthreads();

    const unsigned count = (unsigned)__popcll(w);
    char* base = static_cast<char*>(blockIdx.y ? V : K);
    u32x4 v[kItems];
    size_t dst[kItems];
    bool live[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const unsigned g = t + (unsigned)k * kCommitThreads, j = g >> kLgChunks, c = g & (kChunks - 1);
        live[k] = false;
        dst[k] = 0;
        v[k] = u32x4{0, 0, 0, 0};
        if (j >= count) continue;
        const unsigned i = src_of[j];
        if (i == j) continue;                        // in place already
        const unsigned ps = L + i, pd = L + j;       // pd < ps < capacity: w holds no bit at or past capacity - L
        int page_s = 0, page_d = 0;
        if constexpr (kPaged) {
            page_s = append_page(a.table, a.max_pages, a.lg_page, b, ps);
            page_d = append_page(a.table, a.max_pages, a.lg_page, b, pd);
            if ((unsigned)page_s >= (unsigned)a.num_pages || (unsigned)page_d >= (unsigned)a.num_pages) continue;   // the move is skipped
        }
        const size_t src = append_dst_row<kPaged>(page_s, a.Hkv, a.lg_page, a.Ncap, h, bh, ps);
        dst[k] = (append_dst_row<kPaged>(page_d, a.Hkv, a.lg_page, a.Ncap, h, bh, pd) << (kLgChunks + 4)) + c * 16;
        v[k] = *reinterpret_cast<const u32x4*>(base + (src << (kLgChunks + 4)) + c * 16);
        live[k] = true;
    }
    // every source is in registers before any destination is written: the loads have returned (the counter wait), in every wave (the
    // barrier)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kItems; ++k)
        if (live[k]) *reinterpret_cast<u32x4*>(base + dst[k]) = v[k];
}

// The lengths after the commit, L_b + popcount(w_b).  Behind the copy on the same stream, so `out` may be `in` itself; the words never
// overlap `out` (checked on the host).
__global__ void __launch_bounds__(kCommitThreads)
fa_kvcache_commit_lens_kernel(int* out, CommitDev a, int B)
{
    const unsigned i = blockIdx.x * (unsigned)kCommitThreads + threadIdx.x;
    if (i >= (unsigned)B) return;
    const unsigned L = append_len(a.seqlens, a.Ncap, i);
    out[i] = (int)(L + (unsigned)__popcll(commit_word(a, i, L)));
}

namespace {

template <int kLgChunks>
hipError_t launch_commit(const ::fa_kvcommit_desc* d, const CommitDev& dev, bool paged)
{
    const dim3 grid((unsigned)d->B * (unsigned)d->Hkv, 2);   // B * Hkv fits an int (kvcache_check)
    hipStream_t stream = static_cast<hipStream_t>(d->stream);
    if (paged)
        FA_LAUNCH((fa_kvcache_commit_kernel<kLgChunks, true>), grid, dim3(kCommitThreads), 0, stream, d->K, d->V, dev);
    else
        FA_LAUNCH((fa_kvcache_commit_kernel<kLgChunks, false>), grid, dim3(kCommitThreads), 0, stream, d->K, d->V, dev);
    const hipError_t e = launch_status();
    if (e != hipSuccess || !d->seqlens_out) return e;
    FA_LAUNCH(fa_kvcache_commit_lens_kernel, dim3(((unsigned)d->B + kCommitThreads - 1) / kCommitThreads), dim3(kCommitThreads), 0, stream,
              d->seqlens_out, dev, d->B);
    return launch_status();
}

}  // namespace

// Every check, then the one or two launches.  The grid follows (B, Hkv) and the kernel (d, kv_dtype, paged): host integers only.
hipError_t kvcache_commit(const ::fa_kvcommit_desc* d)
{
    if (!d || d->size != sizeof(fa_kvcommit_desc)) return hipErrorInvalidValue;
    if (!d->K || !d->V || !d->accept_mask) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(d->accept_mask) & 7u) return hipErrorInvalidValue;
    if (d->max_new < 1 || d->max_new > kCommitRows) return hipErrorInvalidValue;
    if (d->kv_dtype != FA_KV_16BIT && d->kv_dtype != FA_KV_FP8_E4M3) return hipErrorInvalidValue;
    const bool fp8 = d->kv_dtype == FA_KV_FP8_E4M3, paged = d->block_table != nullptr;
    // no new rows here: the caches stand in for them
    int Ncap = 0, lg_page = 0;
    const hipError_t bad = kvwrite_check(write_cache_of(*d, d->K, d->V), Ncap, lg_page);
    if (bad != hipSuccess) return bad;
    if (!lens_out_ok(d->seqlens_k, d->seqlens_out, d->B, d->accept_mask, (size_t)d->B * sizeof(unsigned long long))) return hipErrorInvalidValue;
    const CommitDev dev = {d->seqlens_k, d->accept_mask, d->block_table, d->Hkv, Ncap, d->max_new,
                           paged ? d->max_pages : 0, paged ? d->num_pages : 0, lg_page};
    const int row_bytes = fp8 ? d->d : d->d * 2;   // 64, 128 or 256
    if (row_bytes == 64) return launch_commit<2>(d, dev, paged);
    return row_bytes == 128 ? launch_commit<3>(d, dev, paged) : launch_commit<4>(d, dev, paged);
}

}  // namespace fa
