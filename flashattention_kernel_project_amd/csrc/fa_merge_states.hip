// fa_merge_states.hip -- fa_merge_states: R attention states (O_r, lse_r) over disjoint key ranges merged into one by the rule the
// decode entries promise, lse = ln sum_r exp(lse_r), O = sum_r O_r exp(lse_r - lse).  One kernel, the parts in its argument block;
// no workspace, no LDS, no scratch.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md section 7.11.
//
// fa_split_combine_kernel (fa_fwd_split_kernel.hpp) is the model -- one wave per output row, lanes = (slice of the part axis) x
// (group of 4 columns), so the R loads of a row are independent -- but nothing of it is used here: that kernel reads the split
// workspace (unnormalised O^T, m and l in log2 units), this one reads what a decode entry RETURNS (normalised O, lse in natural-log
// units, any of three element types, through two row strides).  This unit does not include that header, so the decode
// instantiations keep their code.
#include "../../include/fa_mi355.h"
#include "fa_dispatch.hpp"

#include <math.h>

namespace fa {

constexpr int kMergeWaves = 4;                    // output rows per workgroup, one wave each; the waves never meet
constexpr float kLn2 = 0.6931471805599453f;

struct MergeParts {
    fa_state_part p[FA_MERGE_MAX_PARTS];          // 512 bytes of the kernel's arguments
};

struct MergeF32 {};                               // the third FA_STATE_* next to F16 and BF16 (fa_common.hpp)

// four neighbouring columns of a row, widened exactly
template <typename P>
__device__ __forceinline__ f32x4 load4(const void* row, unsigned c4)
{
    if constexpr (std::is_same_v<P, MergeF32>) {
        return *reinterpret_cast<const f32x4*>(static_cast<const float*>(row) + 4 * c4);
    } else {
        const u32x2 v = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(row) + 4 * c4);
        return f32x4{P::lo(v[0]), P::hi(v[0]), P::lo(v[1]), P::hi(v[1])};
    }
}

// ... and rounded once on the way out
template <typename Out>
__device__ __forceinline__ void store4(void* row, unsigned c4, f32x4 v)
{
    if constexpr (std::is_same_v<Out, MergeF32>) {
        *reinterpret_cast<f32x4*>(static_cast<float*>(row) + 4 * c4) = v;
    } else {
        *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(row) + 4 * c4) = u32x2{Out::pack2(v[0], v[1]), Out::pack2(v[2], v[3])};
    }
}

// One output row once its lse values are on their way: `mine` is lane l's lse of part l (-inf for l >= R), loaded by the caller and
// not used before the O rows are requested here, so the reductions below run under the rows' latency.
// The weights: M = max, w = exp(mine - M) -- ONE hardware exponential per part -- and L = sum, all wave reductions.
// The rows: lane = (sl, c4), c4 one of the D/4 groups of 4 columns, sl one of the kNsl = 64/(D/4) slices of the part axis; slice sl
// takes the parts sl, sl + kNsl, ... in kN unrolled trips.  Every lane loads on every trip -- a lane whose slice has run out of parts
// re-reads part 0's row, which at most the last needed trip asks for -- so there is no predicate around a load, all kN loads are in
// flight before the first use, and every shuffle that hands out a weight has its source lane active.  What a lane must not use is
// selected away, never multiplied.
// The accumulators start at -0: -0 + x = x for every x, a zero of either sign included, so a lone part keeps the sign of a zero.
template <typename P, int D, int kN>
__device__ __forceinline__ f32x4 merge_rows(const MergeParts& parts, int R, unsigned b, unsigned h, unsigned r, float mine, unsigned sl,
                                            unsigned c4, float& M, float& L)
{
    constexpr unsigned kNsl = 64 / (D / 4);
    constexpr long long kRowBytes = (long long)D * (std::is_same_v<P, MergeF32> ? 4 : 2);
    f32x4 v[kN];
#pragma unroll
    for (int t = 0; t < kN; ++t) {
        const unsigned pi = t * kNsl + sl;
        const fa_state_part& p = parts.p[pi < (unsigned)R ? pi : 0u];
        const long long x = (long long)b * p.stride_b + (long long)h * p.stride_h + r;
        v[t] = load4<P>(static_cast<const char*>(p.O) + x * kRowBytes, c4);
    }
    M = mine;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    // a part with lse = -inf has weight 0 by selection (M may be -inf too: -inf - -inf is a NaN); the largest part has exp2(0) = 1
    const float w = mine == -INFINITY ? 0.0f : fast_exp2((mine - M) * kLog2e);
    L = w;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) L += __shfl_xor(L, o, 64);
    f32x4 acc = {-0.0f, -0.0f, -0.0f, -0.0f};
#pragma unroll
    for (int t = 0; t < kN; ++t) {
        const unsigned pi = t * kNsl + sl;
        const bool has = pi < (unsigned)R;
        const float wp = __shfl(w, (int)(has ? pi : 0u), 64);
        const bool use = has && wp != 0.0f;       // weight 0: lse = -inf (or a part 87 below the maximum) -- its row may hold NaNs
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = use ? __builtin_fmaf(wp, v[t][i], acc[i]) : acc[i];
    }
    return acc;
}

// One wave per output row (b, h, r).  Lane l < R requests part l's lse; the rest is merge_rows with as many trips as R needs (1, 2, 4
// or all: a wave-uniform choice), then the slices are summed and the row is divided, rounded once and stored.
template <typename P, typename Out, int D>
__global__ __launch_bounds__(64 * kMergeWaves)
void fa_merge_states_kernel(MergeParts parts, int R, int H, int rows, unsigned total, void* __restrict__ Og,
                            float* __restrict__ lse_out)
{
    constexpr unsigned kCols4 = D / 4;                        // 16 or 32 groups of 4 columns
    constexpr unsigned kNsl = 64 / kCols4;                    // 4 or 2 slices of the part axis
    constexpr int kTrips = FA_MERGE_MAX_PARTS / kNsl;         // 4 or 8
    const unsigned lane = threadIdx.x & 63u;
    const unsigned rowi = blockIdx.x * kMergeWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (rowi >= total) return;                    // wave-uniform
    const unsigned bh = rowi / (unsigned)rows, r = rowi - bh * (unsigned)rows;
    const unsigned b = bh / (unsigned)H, h = bh - b * (unsigned)H;

    float mine = -INFINITY;
    if (lane < (unsigned)R) {
        const fa_state_part& p = parts.p[lane];
        mine = p.lse[(long long)b * p.stride_b + (long long)h * p.stride_h + r];
    }
    const unsigned c4 = lane & (kCols4 - 1), sl = lane / kCols4;
    const unsigned trips = ((unsigned)R + kNsl - 1) / kNsl;   // wave-uniform: 1 .. kTrips
    float M, L;
    f32x4 acc;
    if (trips <= 1) acc = merge_rows<P, D, 1>(parts, R, b, h, r, mine, sl, c4, M, L);
    else if (trips <= 2) acc = merge_rows<P, D, 2>(parts, R, b, h, r, mine, sl, c4, M, L);
    else if (kTrips == 4 || trips <= 4) acc = merge_rows<P, D, 4>(parts, R, b, h, r, mine, sl, c4, M, L);
    else acc = merge_rows<P, D, kTrips>(parts, R, b, h, r, mine, sl, c4, M, L);
    // sum the slices: lanes that differ only in `sl` are kCols4, 2 * kCols4, ... apart
#pragma unroll
    for (unsigned o = kCols4; o < 64u; o <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], (int)o, 64);
    }
    if (sl != 0) return;
    const bool none = L == 0.0f;                  // every part neutral: O = +0 and lse = -inf
    if (lse_out && lane == 0) lse_out[rowi] = none ? -INFINITY : M + __log2f(L) * kLn2;
    f32x4 o4;
#pragma unroll
    for (int i = 0; i < 4; ++i) o4[i] = none ? 0.0f : acc[i] / L;
    char* orow = static_cast<char*>(Og) + (size_t)rowi * D * (std::is_same_v<Out, MergeF32> ? 4 : 2);
    store4<Out>(orow, c4, o4);
}

template <typename F>
static hipError_t with_state_type(int dtype, F&& f)
{
    switch (dtype) {
    case FA_STATE_F16: return f(F16{});
    case FA_STATE_BF16: return f(BF16{});
    case FA_STATE_F32: return f(MergeF32{});
    default: return hipErrorInvalidValue;
    }
}

static bool aligned4(const void* p, int dtype)
{
    return (reinterpret_cast<uintptr_t>(p) & (dtype == FA_STATE_F32 ? 15u : 7u)) == 0;
}

hipError_t merge_states_dispatch(const fa_merge_desc* d)
{
    if (!d || d->size != sizeof(fa_merge_desc)) return hipErrorInvalidValue;
    if (d->R < 1 || d->R > FA_MERGE_MAX_PARTS || !d->O) return hipErrorInvalidValue;
    if (d->B <= 0 || d->H <= 0 || d->rows <= 0 || (d->d != 64 && d->d != 128)) return hipErrorInvalidValue;
    if (d->part_dtype < FA_STATE_F16 || d->part_dtype > FA_STATE_F32 || d->out_dtype < FA_STATE_F16 || d->out_dtype > FA_STATE_F32)
        return hipErrorInvalidValue;
    if (!aligned4(d->O, d->out_dtype)) return hipErrorInvalidValue;
    MergeParts parts = {};
    for (int i = 0; i < d->R; ++i) {
        const fa_state_part& p = d->parts[i];
        if (!p.O || !p.lse || p.stride_b < 0 || p.stride_h < 0 || !aligned4(p.O, d->part_dtype)) return hipErrorInvalidValue;
        parts.p[i] = p;
    }
    // one wave per row, kMergeWaves rows per workgroup: the launch's thread count must stay below 2^32
    constexpr unsigned long long kMaxRows = 1ull << 26;
    const unsigned long long heads = (unsigned long long)d->B * (unsigned long long)d->H;   // < 2^62
    if (heads >= kMaxRows) return hipErrorInvalidValue;
    const unsigned long long total = heads * (unsigned long long)d->rows;                   // < 2^57
    if (total >= kMaxRows) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + kMergeWaves - 1) / kMergeWaves));
    return with_state_type(d->part_dtype, [&](auto pt) {
        return with_state_type(d->out_dtype, [&](auto ot) {
            auto launch = [&](auto kernel) {
                FA_LAUNCH(kernel, grid, dim3(64 * kMergeWaves), 0, static_cast<hipStream_t>(d->stream), parts, d->R, d->H, d->rows,
                          (unsigned)total, d->O, d->lse);
                return launch_status();
            };
            return d->d == 64 ? launch(fa_merge_states_kernel<decltype(pt), decltype(ot), 64>)
                              : launch(fa_merge_states_kernel<decltype(pt), decltype(ot), 128>);
        });
    });
}

}  // namespace fa
