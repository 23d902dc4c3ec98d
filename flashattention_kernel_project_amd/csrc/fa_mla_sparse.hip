// fa_mla_sparse.hip -- fa_mla_decode_sparse: MLA decode where every token names its keys (an indexer's top-k list of logical key
// positions) over the 16-bit latent cache, contiguous or paged, with splits.  The kernel template and the launcher are in
// fa_mla_sparse_kernel.hpp; this unit owns the entry's checks and plan and instantiates the sixteen kernels (fp16 / bf16 x two output
// types x direct / partial x contiguous / paged) and the merge kernels.  The descriptor's own checks are fa_mla_decode's
// (mla_desc_checks, fa_mla_decode.hip).  DESIGN.md section 7.29, profiles/mla_sparse.txt.
#include "fa_mla_sparse_kernel.hpp"

namespace fa {

namespace {

// What the checks leave behind, from host integers alone: the capacity, the split count and its chunk, the grid's factors.
struct SparsePlan {
    int cap, lg_page, S, chunk, nhb, nqb;
};

// every check that needs no workspace; on success the plan is filled in
bool sparse_plan(const ::fa_mla_decode_desc* d, const int* indices, int topk, long long idx_stride_t, SparsePlan& p)
{
    if (!mla_desc_checks(d, p.cap, p.lg_page)) return false;
    if (!indices || (reinterpret_cast<uintptr_t>(indices) & 3u)) return false;
    if (topk < 1 || topk > mlas::kMaxTopk || idx_stride_t < topk) return false;
    const int tiles = (topk + mla::kSplitTile - 1) / mla::kSplitTile;
    if (d->num_splits < 0 || d->num_splits > tiles) return false;
    p.nhb = (d->Hq + mla::kRows - 1) / mla::kRows;
    const long long base = (long long)d->B * d->max_q * p.nhb;
    p.S = d->num_splits ? d->num_splits : mla_split_count(base, topk);
    const long long rows_seq = (long long)d->max_q * d->Hq;
    if (base * p.S > 0x7FFFFFFFll || (long long)d->B * rows_seq > 0x7FFFFFFFll) return false;   // the grids
    p.chunk = (tiles + p.S - 1) / p.S * mla::kSplitTile;
    p.nqb = (int)((rows_seq + mla::kRows - 1) / mla::kRows);   // the workspace's rows per (b, split), as the merge kernel counts them
    return true;
}

size_t sparse_ws_bytes(const ::fa_mla_decode_desc* d, const SparsePlan& p)
{
    return p.S <= 1 ? 0 : (size_t)d->B * p.S * p.nqb * mla::kRows * mla::kWsRow * sizeof(float);
}

}  // namespace

// the sizing function knows no list: a stand-in pointer and the tightest stride pass the list's checks
size_t mla_sparse_workspace_bytes(const ::fa_mla_decode_desc* d, int topk)
{
    SparsePlan p;
    return sparse_plan(d, reinterpret_cast<const int*>(uintptr_t(4)), topk, topk, p) ? sparse_ws_bytes(d, p) : 0;
}

hipError_t mla_sparse_dispatch(const ::fa_mla_decode_desc* d, const int* indices, int topk, long long idx_stride_t)
{
    SparsePlan p;
    if (!sparse_plan(d, indices, topk, idx_stride_t, p)) return hipErrorInvalidValue;
    const size_t need = sparse_ws_bytes(d, p);
    if (need && (!d->workspace || d->workspace_bytes < need || (reinterpret_cast<uintptr_t>(d->workspace) & 15u)))
        return hipErrorInvalidValue;
    const bool paged = d->block_table != nullptr;
    const mla::Dev a = {static_cast<const uint16_t*>(d->Q), d->O, d->lse, static_cast<const char*>(d->C), static_cast<float*>(d->workspace),
                        d->cu_seqlens_q, d->seqlens_k, d->block_table, d->B, d->Hq, d->total_q, d->max_q, p.cap,
                        paged ? d->max_pages : 0, paged ? d->num_pages : 0, p.lg_page, d->q_stride_t, d->q_stride_h, d->o_stride_t,
                        d->o_stride_h, host_scale_log2e(d->scale), d->causal, p.S, p.nqb, nullptr};
    const mlas::Dev s = {a, indices, idx_stride_t, topk, p.chunk, p.nhb};
    hipStream_t stream = static_cast<hipStream_t>(d->stream);
    const bool f32 = d->out_dtype == FA_OUT_F32;
    if (d->in_dtype == FA_DTYPE_BF16) return f32 ? mla_sparse_launch<BF16, true>(s, paged, stream) : mla_sparse_launch<BF16, false>(s, paged, stream);
    return f32 ? mla_sparse_launch<F16, true>(s, paged, stream) : mla_sparse_launch<F16, false>(s, paged, stream);
}

}  // namespace fa
