// fa_mla_decode.hip -- fa_mla_decode: absorbed-query attention over a latent KV cache (multi-head latent attention).  One row of 576
// 16-bit elements per token serves all Hq heads: the logits run over the whole row, the output over its first 512 elements.  The
// kernel template, the merge kernel and the launcher are in fa_mla_decode_kernel.hpp; this unit owns the host checks and the plan of
// both MLA decode entries and instantiates the 16-bit kernels.  fa_mla_decode_fp8 (rows of 576 e4m3fn codes) passes the same checks
// here and launches what fa_mla_decode_fp8.hip instantiates.  DESIGN.md sections 7.22 and 7.24, profiles/mla_decode.txt.
#include "fa_mla_decode_kernel.hpp"

namespace fa {

// capacity and page geometry of a latent cache, shared with fa_mla_append: false for what both entries refuse
bool mla_geometry(const int* block_table, int Ncap, int num_pages, int page_size, int max_pages, int& cap, int& lg_page)
{
    constexpr int kMaxCap = 1 << 30;
    lg_page = 0;
    if (!block_table) {
        if (Ncap <= 0 || Ncap > kMaxCap) return false;
        cap = Ncap;
        return true;
    }
    if (num_pages <= 0 || max_pages <= 0 || page_size < 16 || (page_size & (page_size - 1))) return false;
    if ((long long)max_pages * page_size > kMaxCap) return false;
    if (reinterpret_cast<uintptr_t>(block_table) & 3u) return false;
    cap = max_pages * page_size;
    while ((1 << lg_page) < page_size) ++lg_page;
    return true;
}

namespace {

// What the checks leave behind: the capacity, the split count and the grid, from host integers alone.
struct MlaPlan {
    int cap, lg_page, S, nqb;
    bool paged;
};

// The number of splits for a shape: enough workgroups for two per CU of a 256-CU device -- one workgroup is resident per CU at
// 144 KiB of LDS -- but at least four 64-key tiles per split.  The split stream's rule (split_count) on this kernel's figures.
int mla_split_count(long long base, int cap)
{
    const int tiles = (cap + mla::kSplitTile - 1) / mla::kSplitTile;
    constexpr int target = 512, min_tiles = 4;
    long long s = (target + base - 1) / base;
    if (s > tiles / min_tiles) s = tiles / min_tiles;
    if (s < 1) s = 1;
    const int chunk_tiles = (int)((tiles + s - 1) / s);   // every split holds at least one tile of a full sequence
    return (tiles + chunk_tiles - 1) / chunk_tiles;
}

// every check that needs no workspace; on success the plan is filled in
bool mla_plan(const ::fa_mla_decode_desc* d, MlaPlan& p)
{
    if (!d || d->size != sizeof(fa_mla_decode_desc)) return false;
    if (!d->Q || !d->O || !d->C || !d->cu_seqlens_q) return false;
    if (d->B <= 0 || d->total_q <= 0 || d->max_q <= 0 || d->Hq < 1 || d->Hq > 128) return false;
    if (d->in_dtype != FA_DTYPE_F16 && d->in_dtype != FA_DTYPE_BF16) return false;
    if (d->out_dtype != FA_OUT_F32 && d->out_dtype != FA_OUT_SAME) return false;
    if (d->causal != 0 && d->causal != 1) return false;
    p.paged = d->block_table != nullptr;
    if (!mla_geometry(d->block_table, d->Ncap, d->num_pages, d->page_size, d->max_pages, p.cap, p.lg_page)) return false;
    const int tiles = (p.cap + mla::kSplitTile - 1) / mla::kSplitTile;
    if (d->num_splits < 0 || d->num_splits > tiles) return false;
    const uintptr_t align = reinterpret_cast<uintptr_t>(d->Q) | reinterpret_cast<uintptr_t>(d->O) | reinterpret_cast<uintptr_t>(d->C);
    if (align & 15u) return false;
    if ((reinterpret_cast<uintptr_t>(d->cu_seqlens_q) | reinterpret_cast<uintptr_t>(d->seqlens_k) | reinterpret_cast<uintptr_t>(d->lse)) & 3u)
        return false;
    if (d->q_stride_t < mla::kDqk || d->o_stride_t < mla::kDv || d->q_stride_h < 0 || d->o_stride_h < 0) return false;
    if (d->q_stride_t % 8 || d->q_stride_h % 8 || d->o_stride_t % 8 || d->o_stride_h % 8) return false;
    // a sequence's view -- up to max_q tokens over the Hq heads -- is addressed with 32-bit byte offsets
    const unsigned es = d->out_dtype == FA_OUT_F32 ? 4u : 2u;
    const int rows = d->max_q < d->total_q ? d->max_q : d->total_q;
    const unsigned __int128 qv = ((unsigned __int128)(rows - 1) * (unsigned long long)d->q_stride_t +
                                  (unsigned __int128)(d->Hq - 1) * (unsigned long long)d->q_stride_h + mla::kDqk) * 2u;
    const unsigned __int128 ov = ((unsigned __int128)(rows - 1) * (unsigned long long)d->o_stride_t +
                                  (unsigned __int128)(d->Hq - 1) * (unsigned long long)d->o_stride_h + mla::kDv) * es;
    if (qv > 0xFFFFFFFFull || ov > 0xFFFFFFFFull) return false;
    const long long rows_seq = (long long)d->max_q * d->Hq;
    const long long nqb = (rows_seq + mla::kRows - 1) / mla::kRows;
    const long long base = (long long)d->B * nqb;
    p.S = d->num_splits ? d->num_splits : mla_split_count(base, p.cap);
    if (base * p.S > 0x7FFFFFFFll || (long long)d->B * rows_seq > 0x7FFFFFFFll) return false;   // the grids
    p.nqb = (int)nqb;
    return true;
}

size_t mla_ws_bytes(const ::fa_mla_decode_desc* d, const MlaPlan& p)
{
    return p.S <= 1 ? 0 : (size_t)d->B * p.S * p.nqb * mla::kRows * mla::kWsRow * sizeof(float);
}

// both entries: the checks, then the kernels of the cache's element (c_scale is looked at with fp8 only)
hipError_t mla_decode_any(const ::fa_mla_decode_desc* d, bool fp8, const float* c_scale)
{
    MlaPlan p;
    if (!mla_plan(d, p)) return hipErrorInvalidValue;
    if (fp8 && (reinterpret_cast<uintptr_t>(c_scale) & 3u)) return hipErrorInvalidValue;
    const size_t need = mla_ws_bytes(d, p);
    if (need && (!d->workspace || d->workspace_bytes < need || (reinterpret_cast<uintptr_t>(d->workspace) & 15u)))
        return hipErrorInvalidValue;
    const mla::Dev a = {static_cast<const uint16_t*>(d->Q), d->O, d->lse, static_cast<const char*>(d->C), static_cast<float*>(d->workspace),
                        d->cu_seqlens_q, d->seqlens_k, d->block_table, d->B, d->Hq, d->total_q, d->max_q, p.cap,
                        p.paged ? d->max_pages : 0, p.paged ? d->num_pages : 0, p.lg_page, d->q_stride_t, d->q_stride_h, d->o_stride_t,
                        d->o_stride_h, host_scale_log2e(d->scale), d->causal, p.S, p.nqb, fp8 ? c_scale : nullptr};
    hipStream_t stream = static_cast<hipStream_t>(d->stream);
    const bool bf16 = d->in_dtype == FA_DTYPE_BF16, f32 = d->out_dtype == FA_OUT_F32;
    return fp8 ? mla_launch_fp8(a, bf16, f32, p.paged, stream) : mla_launch_typed<false>(a, bf16, f32, p.paged, stream);
}

}  // namespace

size_t mla_decode_workspace_bytes(const ::fa_mla_decode_desc* d)
{
    MlaPlan p;
    return mla_plan(d, p) ? mla_ws_bytes(d, p) : 0;
}

hipError_t mla_decode_dispatch(const ::fa_mla_decode_desc* d) { return mla_decode_any(d, false, nullptr); }

hipError_t mla_decode_fp8_dispatch(const ::fa_mla_decode_desc* d, const float* c_scale) { return mla_decode_any(d, true, c_scale); }

}  // namespace fa
