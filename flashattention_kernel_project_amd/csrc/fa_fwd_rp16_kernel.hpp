// fa_fwd_rp16_kernel.hpp -- the rolling half-tile pipeline of fa_fwd_rp.hip on v_mfma_f32_16x16x32 (d = 64).
//
// Why a second shape of the same stream: the d=64 forward runs at the package power cap, where wall time is joules per
// launch divided by the cap (fa_fwd_rp needs 15 % fewer cycles than round 1's phase-ordered 16x16x32 stream and
// lands at the same 0.55 ms, the clock simply settles at 1.80 instead of 2.10 GHz).  Sustained at two waves per SIMD the slot model
// (tools/slot_energy.py, profiles/r02_slot_energy.txt) prices one slot -- two scores per lane -- at
//     32x32x16 + folded vector work      21.7 nJ per SIMD     2 x 16x16x32 + folded      19.6 nJ   (-9 %)
//     32x32x16 + exact vector work       25.7 nJ              2 x 16x16x32 + exact       23.4 nJ   (-9 %)
// although the 16x16x32 form needs a quarter more cycles per slot (it holds the issue port 8 of every 16 cycles).
// So: the same pipeline (QK^T one half tile ahead, PV one behind, the softmax of the half tile in between issued as
// slices between the matrix instructions, branch-free steady state, folded fast pass with the wave reference maximum as
// the accumulators' start value; overflow safety, row sums and the persistent XCD-aware grid as fa_fwd_rp.hip's header
// describes them) with the lane roles and LDS images the 16x16x32 instruction asks for:
//   lane = 16 g + c; the accumulator of S^T = K.Q^T for (16-row query block x, 16-key block kb) holds query 16x + c on
//   the lane and keys 16kb + 4g + i in register i; the packed registers of key blocks 2s, 2s+1 are the B fragment of
//   k-step s of O^T += V^T.P^T; K row-major with the 16-B chunk index XORed by (row >> 1) & 7, V in 256-B blocks
//   [key/8][d/16] x [8 keys][16 cols] for ds_read_b64_tr_b16.
// A step = one half tile (32 keys) = 32 matrix instructions (16 QK^T + 16 PV, four K and four V^T fragments, each
// feeding the wave's four query blocks) around the vector work of 32 scores per lane.
#pragma once
#include "fa_tile.hpp"
#include "fa_dispatch.hpp"

#include <type_traits>
#include <utility>

// The measuring instruments of this kernel: the only preprocessor switches it has.  None selects between product code paths;
// all are set per build through tools/build_variant.sh and default to the product.
//   FA_RP16_ABL     tools/ablate_rp16.sh, tools/sustain_libs.py, tools/ab_libs.py: timing ablations, results are garbage.
//                   1 no LDS fragment reads, 2 no softmax vector work, 4 no matrix instructions, 8 no K/V staging, 16 no tile
//                   barrier, 32 no O stores, 64 no Q loads, 128 no loads of an item's first two K/V tiles, 256 every fragment
//                   read issued twice
//   FA_RP16_GATES   built together with FA_RP16_ABL (=0: an ablated build must not refuse its garbage): which refusal gates of
//                   the folded pass are armed (1 sum overflow, 2 sum too small, 4 reference, 8 Q range)
//   FA_RP16_STAMPS  tools/item_phases.py: 100 MHz timestamps of an item's phases, written over O[first row of the item][0..7]
//                   (fp32 out only)
#ifndef FA_RP16_ABL
#define FA_RP16_ABL 0
#endif
#ifndef FA_RP16_GATES
#define FA_RP16_GATES 15
#endif

namespace fa {

namespace rp16 {
template <int... I, typename F>
__device__ __forceinline__ void sfor_impl(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sfor(F&& f) {
    sfor_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}
template <typename T> struct Mx;
// mfma_v*: the same instruction spelled out with its accumulator in ARCHITECTURAL registers.  A kernel that may use the
// accumulator half of the file (one wave per SIMD) gets every builtin matrix instruction in the form whose C/D live there:
// right for O and the row sums (only matrix instructions touch them), wrong for the scores (one v_accvgpr_read per score).
// The compiler does not know these statements are matrix instructions: the wait states between one of them and the first
// vector instruction that reads its result are the CALLER's (see kAsmQK; tools/mfma_hazard_lint.py checks the listing).
#define FA_MFMA_V(NAME, SFX)                                                                                              \
    static __device__ __forceinline__ void mfma_v_acc(f32x4& acc, u32x4 a, u32x4 b) {                                     \
        asm("v_mfma_f32_16x16x32_" SFX " %0, %1, %2, %0 ; fa_qk" : "+v"(acc) : "v"(a), "v"(b));                           \
    }                                                                                                                     \
    static __device__ __forceinline__ f32x4 mfma_v_init(u32x4 a, u32x4 b, f32x4 c) {                                      \
        f32x4 d;                                                                                                          \
        asm("v_mfma_f32_16x16x32_" SFX " %0, %1, %2, %3 ; fa_qk" : "=&v"(d) : "v"(a), "v"(b), "v"(c));                    \
        return d;                                                                                                         \
    }                                                                                                                     \
    static __device__ __forceinline__ f32x4 mfma_v_zero(u32x4 a, u32x4 b) {                                               \
        f32x4 d;                                                                                                          \
        asm("v_mfma_f32_16x16x32_" SFX " %0, %1, %2, 0 ; fa_qk" : "=&v"(d) : "v"(a), "v"(b));                             \
        return d;                                                                                                         \
    }
template <> struct Mx<F16> {
    static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    FA_MFMA_V(F16, "f16")
};
template <> struct Mx<BF16> {
    static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    FA_MFMA_V(BF16, "bf16")
};
#undef FA_MFMA_V
constexpr int kW = 8;
constexpr int kAheadWide = 2;          // 64-row waves: fragments read ahead of their MFMAs (at most ring - 1), ring of 4 registers
constexpr float kHeadroom = 4.0f;      // exact optimistic pass: reference = the row's max over its first 32 keys + this
constexpr float kHeadroomFold = 1.0f;  // folded pass: the reference already is the maximum over the wave's 64 rows
constexpr float kFoldMax = 16.0f;  // folded pass: largest |reference| (log2 units) it accepts -- Q's fp16 rounding moves a logit by <= |logit| * 2^-11
constexpr float kFoldAim = 6.0f;       // folded pass: log2 of the row sum the reference is placed for
constexpr float kFoldShiftMin = 6.0f;  // ... and how far below the first scores' maximum it may go (weights stay below 2^16)
constexpr int kStageSlot = 8;          // matrix slot (of 32; scaled for narrower steps) of the second step in front of which tile j+2 is written to LDS
// Two tiles per loop iteration and barrier (ring of eight [K tile][V tile] slots, tiles landed three ahead instead of two): for
// the narrow waves a tile is a few hundred issue cycles per wave, and the barrier of eight waves plus the landing of the next
// tile cost as much again (stamps at B4 H8 N1024: 16 tiles took 13.8 us = 2000 cycles each).  D = 64 only (128 KB of LDS).
// (At full width the same form lost: DESIGN.md 3.6 (8).)
constexpr bool pair_tiles(int D, int X, bool dma) { return D == 64 && !dma && X <= 2; }
// The running-max pass of the full-width eight-wave kernels runs INSIDE their launch (see kInLaunch at rp16_body): a workgroup
// collects up to kTailCap row blocks its fast passes refused in a list in LDS and computes them on half-width waves in between.
constexpr int kTailCap = 8;
constexpr bool tail_in_launch(int D, int X, bool dma, bool scan, int wv, int ks) {
    return !scan && !dma && 16 * X * (D / 64) >= 64 && wv == 8 && ks == 1;
}
// where that list lies: behind the ring of the half-width body (Xt = its blocks per wave), which is the larger of the two
constexpr unsigned tail_list_off(int D, int Xt) { return (pair_tiles(D, Xt, false) ? 8u : 4u) * 2u * (unsigned)(kBlockN * D * 2); }
constexpr unsigned kTailListBytes = 8u * kTailCap;   // [head, first row] per entry
}  // namespace rp16

#ifdef FA_EXPERIMENTS
// libfa_mi355_exp.so only (fa_lab_rp16_pass_ids): when set, every workgroup of a non-redo kernel records which pass produced its
// row block -- 0 folded fast pass, 1 exact optimistic pass, 2 running-max pass in the kernel, 3 left to the redo kernel -- at
// [head * blocks per head + block].  The product build carries neither the symbol nor the store.  (One copy per translation
// unit: device symbols do not link across them; fa_fwd_rp16.hip's rp16_set_pass_ids sets them all.)
static __device__ unsigned* g_rp16_pass_ids = nullptr;
static hipError_t rp16_set_pass_ids_tu(unsigned* dev_ptr) { return hipMemcpyToSymbol(HIP_SYMBOL(g_rp16_pass_ids), &dev_ptr, sizeof(dev_ptr)); }
#endif

// kDma: K/V tiles go HBM/L2 -> LDS by LDS-DMA (buffer_load ... lds, one 1-KB piece of the K image and one of the V image
// per wave and tile, the images' permutations applied on the SOURCE address) instead of through registers
// (buffer_load -> VGPR -> ds_write_b128).  This is the loader half of the reference's warp-specialised hand-off
// (flashattn_streaming_16x16_mw_v5_warp_specialize.cu:121-185, _v11.cu:189-258) as far as CDNA4 affords it: the
// register file is allocated per kernel, so a ninth (loader) wave would cut every wave to 170 registers, and a loader
// among the eight idles an eighth of the matrix capacity (fixed roles: 43 vs 37.7 cycles per slot in the slot model),
// so every wave issues the DMA for its own eighth of the tile and the hand-off is the counted wait + the tile barrier.
// D = head dim (64 or 128); X = 16-row query blocks per wave (4 at D = 64: 64 rows, 512-row workgroups; 2 at D = 128: 32 rows,
// 256-row workgroups).  A step always is 32 matrix instructions: 2*D/32 K fragments and D/16 V^T fragments, each feeding X blocks.
// kCausal: query row i attends to keys 0..i.  A workgroup runs the tiles up to its last row's diagonal; the tiles its row
// range crosses go through the masked copy of the step (key > row -> -inf), the ones before it through the branch-free
// loop.  Waves are not skipped individually (the pipeline is shared), which costs the upper rows' waves ~3.5 masked tiles
// per item; query blocks alternate direction from one round of the persistent grid to the next (last-to-first, then
// first-to-last), so that every CU's items add up to the same number of tiles.
// kScan: the half-width running-max body of the full-width instantiations.  Their stream fills the 256 registers a wave gets at
// two waves per SIMD; the running-max bookkeeping on top of it spills the Q fragments (reloaded from scratch every step, and the
// allocator's choices for the fast passes suffer with it: +17 % on the bench shape).  So a full-width workgroup whose optimistic
// passes fail never runs the running-max pass in its item loop; the block is computed on half-width waves, running-max pass
// only, by a kScan = true instantiation.  Which one, and how it learns of the block, depends on the family:
//   * eight waves (kWv = 8: d = 64 X = 4, d = 128 X = 2, plain and causal) -- INSIDE the same launch (kInLaunch, described at
//     rp16_body below): the workgroup lists the block in LDS, stores nothing to it, and its own eight waves run the kScan body
//     over the list.  No marker, no second kernel.
//   * one wave per SIMD (kWv = 4, D = 128 X = 4) -- a REDO KERNEL: four waves cannot host the eight-wave half-width pass.  The
//     workgroup leaves a marker word in the first output element of each half of its row block, and the kScan kernel -- launched
//     right behind it on the same stream -- walks ITS row blocks, finds the marked ones and computes them.  A marker that happens
//     to equal a genuine output word (a NaN pattern no kernel of ours produces) would only cause a block to be computed twice,
//     with the same result; an unmarked failed block cannot occur (the marker store is the failing workgroup's only store to it).
// kWv: waves per workgroup.  8 = two per SIMD, 256 registers each (every shape above).  4 = ONE wave per SIMD with the whole
// 512-register file (accumulators and Q in the upper half): at D = 128 that affords 64-row waves (X = 4), i.e. every LDS
// fragment feeds four matrix instructions instead of two and four waves instead of eight read each tile -- the structure the
// CDNA4 guide documents for d = 128 (cdna_hip_programming.md, "4-wave, one-wave-per-SIMD"), built here on this stream.
// (kWv = 4 with 16-row waves at D = 64 -- 64-row workgroups, two per CU -- was measured for small grids and lost: 23.5 against
// 16.9 us at B4 H8 N1024, every workgroup stages every tile of its head.)
// kKeySplit = 2 (small grids; 16-row waves, D = 64, N a multiple of 128): the workgroup is TWO groups of eight waves over the
// same 128 query rows, group s running the whole algorithm -- its own LDS ring, its own reference, every pass -- over keys
// [s N/2, (s+1) N/2); the votes and barriers are workgroup-wide (both groups run the same number of tiles), and group 1 hands
// (O, l, m) to group 0 through LDS at the end, which merges with 2^(m_s - M) weights and stores.  A wave's chain of tiles
// halves and four waves share a SIMD instead of two -- for grids where a workgroup per CU runs a handful of tiles and waits
// on LDS latency and the barrier most of the time.
// rp16_body: the kernel's body (fa_fwd_rp16_body.inc) as a device function, for the in-launch families only: their kernel is a thin
// wrapper around two of them.  Every other family has the same text as the body of its __global__ function, as before (see the
// .inc file for why).  first_item: the first work item of this workgroup (the persistent loop goes on in steps of the grid).
// Returns the item the loop stopped in front of.
// kInLaunch (full-width families on eight waves, rp16::tail_in_launch): no redo kernel and no marker.  The wrapper runs two
// bodies in turn in ONE launch.  The full-width body (kScan = false) appends a row block its fast passes refuse to a list in LDS
// behind the rings -- (head, first row), already resolved through the XCD remap and the causal direction -- stores nothing to
// it, counts it in n_listed and returns early once the list holds kTailCap entries.  The half-width body (kScan = true: the
// redo kernel's instantiation parameters, so its arithmetic is the redo kernel's) takes the two half-blocks of each of the
// n_listed entries from the list instead of looking for markers; a half-block that begins at or behind row N is skipped.
template <typename T, int D, int X, bool kOutF32, bool kFold, bool kDma, bool kCausal, bool kScan, int kWv, int kKeySplit, bool kInLaunch>
__device__ __forceinline__
unsigned rp16_body(const uint16_t* __restrict__ Qg, const uint16_t* __restrict__ Kg,
                   const uint16_t* __restrict__ Vg, void* __restrict__ Og,
                   int N, int nqb, float scale_log2e, unsigned total_wg, unsigned first_item, unsigned& n_listed)
{
#define FA_RP16_DEVICE_BODY 1
#include "fa_fwd_rp16_body.inc"
#undef FA_RP16_DEVICE_BODY
}

template <typename T, int D, int X, bool kOutF32, bool kFold, bool kDma = false, bool kCausal = false, bool kScan = false, int kWv = 8,
          int kKeySplit = 1>
__global__ __launch_bounds__(64 * kWv * kKeySplit, kWv * kKeySplit / 4)
void fa_fwd_rp16_kernel(const uint16_t* __restrict__ Qg, const uint16_t* __restrict__ Kg,
                        const uint16_t* __restrict__ Vg, void* __restrict__ Og,
                        int N, int nqb, float scale_log2e, unsigned total_wg)
{
    if constexpr (!rp16::tail_in_launch(D, X, kDma, kScan, kWv, kKeySplit)) {
        // (the body itself, not a call of rp16_body: see fa_fwd_rp16_body.inc)
#define FA_RP16_DEVICE_BODY 0
#include "fa_fwd_rp16_body.inc"
#undef FA_RP16_DEVICE_BODY
    } else {
        // the full-width body until its items are done or its list is full; then the half-width running-max body over the list;
        // and back (see kInLaunch).  On data no fast pass refuses the first call ends with an empty list and that is all.
        unsigned item = blockIdx.x;
        do {
            unsigned listed = 0u;
            item = rp16_body<T, D, X, kOutF32, kFold, false, kCausal, false, 8, 1, true>(Qg, Kg, Vg, Og, N, nqb, scale_log2e, total_wg, item, listed);
            if (listed == 0u) break;   // (workgroup-uniform)
            // Every wave is past the full-width body's last LDS read before the half-width body writes its ring, the list is
            // visible, and the stand-in stores of the full-width body (zeros on the first row of a wave's first block) have
            // arrived before ANOTHER wave stores that row's value.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            rp16_body<T, D, X / 2, kOutF32, false, false, kCausal, true, 8, 1, true>(Qg, Kg, Vg, Og, N, nqb, scale_log2e, total_wg, 0u, listed);
            __syncthreads();   // ... and past the half-width body's last read of the ring and the list before either is written again
        } while (item < total_wg);
    }
}

template <typename T, int D, int X, bool kOutF32, bool kFold, bool kDma = false, bool kCausal = false, int kWv = 8, int kKeySplit = 1>
static hipError_t launch_rp16(const FwdArgs& a)
{
    using namespace rp16;
    constexpr int kW = kWv;
    constexpr int lds_bytes = kKeySplit * ((pair_tiles(D, X, kDma) && kKeySplit == 1 && kWv == 8) ? 8 : 4) * 2 * kBlockN * D * 2;   // ring(s) of four (eight) [K tile][V tile] slots
    if (kKeySplit > 1 && a.N % (kBlockN * kKeySplit) != 0) return hipErrorInvalidValue;
    constexpr bool kInLaunch = tail_in_launch(D, X, kDma, false, kWv, kKeySplit);
    // kInLaunch: the larger of the two bodies' rings (the half-width body's) and the list behind it
    constexpr int lds_tail = kInLaunch ? (int)(tail_list_off(D, X / 2) + kTailListBytes) : 0;
    static_assert(!kInLaunch || lds_tail >= lds_bytes, "the half-width body's ring is the larger one");
    static_assert(lds_tail + 64 <= 160 * 1024, "a CU has 160 KB of LDS");
    constexpr int lds_extra = 64;   // the waves' landing flags (kFlagBar)
    constexpr int kRows = 16 * X * kW;
    const int nqb = (a.N + kRows - 1) / kRows;
    const long long nwg = (long long)a.BH * nqb;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const long long cap = device_cus();
    const unsigned grid = nwg > cap ? (unsigned)cap : (unsigned)nwg;
    auto kern = fa_fwd_rp16_kernel<T, D, X, kOutF32, kFold, kDma, kCausal, false, kWv, kKeySplit>;
    constexpr int lds_all = (kInLaunch ? lds_tail : lds_bytes) + lds_extra;
    const hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds_all);
    if (attr != hipSuccess) return attr;
    FA_LAUNCH(kern, dim3(grid), dim3(64 * kW * kKeySplit), lds_all, a.stream,
              static_cast<const uint16_t*>(a.Q), static_cast<const uint16_t*>(a.K), static_cast<const uint16_t*>(a.V), a.O, a.N, nqb,
              host_scale_log2e(a.scale), (unsigned)nwg);
    if (launch_status() != hipSuccess) return launch_status();
    if constexpr (!kDma && 16 * X * (D / 64) >= 64 && !kInLaunch) {
        // full-width waves, one per SIMD: the redo kernel for the row blocks whose optimistic passes failed (see kScan): half-width waves,
        // running-max pass only; with nothing marked it ends after one look at the marker words
        constexpr int kW2 = 8, X2 = X * kW / (2 * kW2), kRows2 = 16 * X2 * kW2;
        constexpr int lds2 = (pair_tiles(D, X2, false) ? 8 : 4) * 2 * kBlockN * D * 2 + 4 * (1 + 64 * kW2);   // (half this kernel's row block, on eight waves)
        const int nqb2 = (a.N + kRows2 - 1) / kRows2;
        const long long nwg2 = (long long)a.BH * nqb2;
        if (nwg2 > 0x7FFFFFFFll) return hipErrorInvalidValue;
        const unsigned grid2 = nwg2 > cap ? (unsigned)cap : (unsigned)nwg2;
        auto kern2 = fa_fwd_rp16_kernel<T, D, X2, kOutF32, false, false, kCausal, true>;
        const hipError_t attr2 = ensure_dyn_lds(reinterpret_cast<const void*>(kern2), lds2);
        if (attr2 != hipSuccess) return attr2;
        static_assert(2 * kRows2 == kRows, "the redo kernel's row block is half of this kernel's");
        FA_LAUNCH(kern2, dim3(grid2), dim3(64 * kW2), lds2, a.stream,
                  static_cast<const uint16_t*>(a.Q), static_cast<const uint16_t*>(a.K), static_cast<const uint16_t*>(a.V), a.O, a.N, nqb2,
                  host_scale_log2e(a.scale), (unsigned)nwg2);
    }
    return launch_status();
}

// One (D, X, staging, mask) family of the pipeline: its (input type, output type, folded-first) instantiations.  The families
// are explicitly instantiated in translation units of their own (fa_fwd_rp16_{d64,d64n,d64ks,d128,d128w,c,cw}.hip) so that they
// compile side by side; fa_dispatch.hpp declares the template for fa_fwd_rp16.hip.
template <int D, int X, bool kDma, bool kCausal, int kWv, int kKeySplit>
hipError_t rp16_family(const FwdArgs& a, bool fold)
{
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        using T = decltype(t);
        constexpr bool kOutF32 = decltype(f32)::value;
        // (the LDS-DMA path cannot convert bf16 K on the way: exact passes only)
        if constexpr (!(kDma && std::is_same<T, BF16>::value)) {
            if (fold) return launch_rp16<T, D, X, kOutF32, true, kDma, kCausal, kWv, kKeySplit>(a);
        }
        return launch_rp16<T, D, X, kOutF32, false, kDma, kCausal, kWv, kKeySplit>(a);
    });
}

}  // namespace fa
