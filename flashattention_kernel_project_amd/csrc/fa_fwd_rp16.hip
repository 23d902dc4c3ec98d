// fa_fwd_rp16.hip -- entry points of the rolling half-tile pipeline (fa_fwd_rp16_kernel.hpp); the kernel families are
// instantiated in fa_fwd_rp16_{d64,d64n,d64ks,d128,d128w,c,cw}.hip.
#include "fa_tile.hpp"
#include "fa_dispatch.hpp"

namespace fa {

#ifdef FA_EXPERIMENTS
hipError_t rp16_set_pass_ids(unsigned* dev_ptr)
{
    hipError_t e = rp16_set_pass_ids_d64(dev_ptr);
    if (e == hipSuccess) e = rp16_set_pass_ids_d64n(dev_ptr);
    if (e == hipSuccess) e = rp16_set_pass_ids_d128(dev_ptr);
    if (e == hipSuccess) e = rp16_set_pass_ids_c(dev_ptr);
    if (e == hipSuccess) e = rp16_set_pass_ids_d128w(dev_ptr);
    if (e == hipSuccess) e = rp16_set_pass_ids_cw(dev_ptr);
    if (e == hipSuccess) e = rp16_set_pass_ids_d64ks(dev_ptr);
    return e;
}
#endif

static bool rp16_shape_ok(int N, int D)
{
    if (D != 64 && D != 128) return false;
    return (unsigned long long)(N + 64 * 8 + 3 * kBlockN) * (unsigned)D * 4ull < (1ull << 32);   // per-head byte offsets are 32 bit
}

// NaN / zero scale: the exact passes define the result
static bool rp16_fold_ok(float scale) { return (scale == scale) && scale * kLog2e != 0.0f; }

// fold: the folded fast pass first (else the exact passes only).  A family that does not exist at this D is an error.
// rp16_family<D, X (16-row blocks per wave), kDma, kCausal, waves, key split>
hipError_t rp16_dispatch(const FwdArgs& a, bool fold, Rp16Family family)
{
    if (!rp16_shape_ok(a.N, a.D)) return hipErrorInvalidValue;
    const bool f = fold && rp16_fold_ok(a.scale);
    if (a.D == 128) {
        switch (family) {
            case Rp16Family::kFull: return rp16_family<128, 2, false, false>(a, f);   // 32-row waves, 256-row workgroups (+ the running-max body on 16-row waves, same launch)
            case Rp16Family::kHalf: return rp16_family<128, 1, false, false>(a, f);
            case Rp16Family::kOneWave: return rp16_family<128, 4, false, false, 4>(a, f);   // four 64-row waves, 512 registers per wave
            default: return hipErrorInvalidValue;
        }
    }
    switch (family) {
        case Rp16Family::kFull: return rp16_family<64, 4, false, false>(a, f);      // 64-row waves, 512-row workgroups (+ the half-width running-max body, same launch)
        case Rp16Family::kHalf: return rp16_family<64, 2, false, false>(a, f);      // small grids: the same
        case Rp16Family::kQuarter: return rp16_family<64, 1, false, false>(a, f);   // pipeline on narrower waves
        case Rp16Family::kKeySplit: return rp16_family<64, 2, false, false, 4, 2>(a, f);   // two groups of FOUR 32-row waves (N % 128 == 0)
#ifdef FA_EXPERIMENTS
        case Rp16Family::kDma: return rp16_family<64, 4, true, false>(a, f);
#endif
        default: return hipErrorInvalidValue;   // (the LDS-DMA variant lost the A/B, 0.552 vs 0.508 ms: experimental build only)
    }
}

// Causal forward on the pipeline (folded fast pass first for both input types), D in {64, 128}; kOneWave: one wave per SIMD
// (d = 128 only).
hipError_t rp16_causal_dispatch(const FwdArgs& a, Rp16Family family)
{
    if (!rp16_shape_ok(a.N, a.D)) return hipErrorInvalidValue;
    const bool fold = rp16_fold_ok(a.scale);
    if (family == Rp16Family::kOneWave)
        return a.D == 128 ? rp16_family<128, 4, false, true, 4>(a, fold) : hipErrorInvalidValue;
    if (family != Rp16Family::kFull) return hipErrorInvalidValue;
    return a.D == 64 ? rp16_family<64, 4, false, true>(a, fold) : rp16_family<128, 2, false, true>(a, fold);
}

}  // namespace fa
