// fa_fwd_split_kernel.hpp -- device code of the split-KV stream: one kernel template for fa_forward_splitkv (fa_fwd_split.hip) and
// for every KV-cache decode entry, and the merge kernel behind a split.  The plain instantiations take no trailing argument; a
// KV-cache instantiation (kCache) takes ONE pack, a CacheArgs inside the wrappers of the parts it has.  A wrapper derives from what
// it wraps and adds its bit to kParts, and everything a part adds to the kernel sits behind `if constexpr` of its flag:
//
//   part (pack type)       what it adds                                             guard      note under profiles/
//   CacheArgs              key counts read on the device, causal tail, lse          kCache     kvcache_decode.txt
//   PagedArgs              K/V rows from pages of a pool, through a block table     kPaged     kvcache_paged.txt
//   Fp8Args<>              one-byte e4m3fn K/V, widened into LDS; per-head scales   kFp8       kvcache_fp8.txt
//   WindowArgs<>           a lower key limit per row, a first tile per sequence     kWindow    kvcache_window.txt
//   LogitArgs<>            soft-capped scores, one sink logit per query head        kLogits    kvcache_logits.txt
//   RaggedArgs<>           a query row count per sequence                           kRagged    kvcache_ragged.txt
//   PackedArgs<>           token-packed Q, O and lse, row counts from cu_q          kPacked    kvcache_decode_varlen.txt
//   TreeArgs<>             a 64-bit ancestor word per row for the causal triangle   kTree      kvcache_tree.txt
//   RoutedArgs<>           a sequence above max_q rows has no live row here         kRouted    kvcache_attend_varlen.txt
//
// The wrappers nest in one order -- [Paged] < [Fp8] < Window < Logit < Ragged < Packed < {Tree | Routed} -- and the packs the library
// instantiates, with the translation unit that owns each, are named in fa_fwd_kvdecode.hpp (PackFor) and DESIGN.md 7.21.  What each
// part does in the kernel is told above the kernel.  Design notes: head of fa_fwd_split.hip, DESIGN.md 7.1.
#pragma once
#include "fa_tile.hpp"

#include <type_traits>

namespace fa {

#ifndef FA_SPLIT_ROTATE
#define FA_SPLIT_ROTATE 1
#endif
#ifndef FA_SPLIT_NT
#define FA_SPLIT_NT 1   // K/V are read exactly once: non-temporal loads (5.97 -> 6.75 TB/s at B8 H16 Nq1 Nk32768 d128)
#endif
namespace split {
constexpr int kW = 4;                 // waves per workgroup
constexpr int kRows = 32 * kW;        // query rows per workgroup
}  // namespace split
constexpr float kLn2 = 0.6931471805599453f;

// One bit per part of a pack: a pack's kParts is its base's with its own bit set, and the kernel's k* flags are tests of it.
namespace kvpart {
constexpr unsigned kPaged = 1u, kFp8 = 2u, kWindow = 4u, kLogits = 8u, kRagged = 16u, kPacked = 32u, kTree = 64u, kRouted = 128u;
}

// What the KV-cache instantiations (kCache) take as their trailing argument; the plain split kernels have no such argument.
struct CacheArgs {
    static constexpr unsigned kParts = 0u;
    const int* seqlens;   // [B] key counts on the device, or nullptr: every sequence holds Nk keys
    float* lse;           // [BH][Nq] natural-log sum of exponentials, or nullptr
    int Hkv;              // K/V heads per batch entry: bh / Hkv indexes seqlens
    int Nq1;              // query rows per query head (the Nq rows of a K/V head are G folded heads of Nq1 rows)
    int causal;           // row i of its head sees the keys [0, L - Nq1 + 1 + i)
};

// What the paged instantiations take instead: the CacheArgs plus where a key's row lives.  K/V are pools [num_pages, Hkv, page, D];
// key j of sequence b is row j % page of page table[b * max_pages + j / page].
struct PagedArgs : CacheArgs {
    static constexpr unsigned kParts = CacheArgs::kParts | kvpart::kPaged;
    const int* table;     // [B][max_pages] page numbers on the device
    int max_pages;        // row pitch of the table; the capacity Nk is max_pages << lg_page
    int num_pages;        // pages in the pool: a live entry outside [0, num_pages) reads as a page of zeros
    int lg_page;          // log2 of the page size in keys (>= 4)
};

// What the fp8 instantiations take: the CacheArgs or the PagedArgs plus the dequantisation scales.  K/V elements are then ONE byte
// (OCP e4m3fn) and are widened to T while a tile is written to LDS; the kernel's K/V pointers address bytes.
template <typename Base> struct Fp8Args : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kFp8;
    const float* k_scale;   // [Hkv] on the device, or nullptr (1.0): the logits are scale * k_scale[hkv] * q.k8
    const float* v_scale;   // [Hkv] on the device, or nullptr (1.0): the output is v_scale[hkv] * softmax.v8
};

// What the sliding-window instantiations take: any of the packs above plus the window.  Row i of a head sees the keys
// [max(0, L - Nq1 + 1 + i - window), c_i) with c_i the limit of the wrapped pack (L, or the causal one).  The wrapper derives from
// what it wraps, so the wrapped pack's fields and parts are its own.
template <typename Base> struct WindowArgs : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kWindow;
    int window;           // >= 1 (0, "no window", never reaches the kernel: the host calls the wrapped entry)
};

// What the soft-cap / attention-sink instantiations take (fa_kvcache_decode): a WindowArgs pack plus the two options on the logits.
// The cap comes in log2 units, as the scores do once they are multiplied by the folded factor c; the sinks are one natural-log
// logit per QUERY head and never enter the tile loop (they join in the one-pass epilogue and in the merge, SinkLse below).
template <typename Base> struct LogitArgs : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kLogits;
    const float* sinks;   // [Hkv * G] on the device, or nullptr: none
    float cap2;           // softcap * log2(e); 0: no cap (the tile loop then runs the wrapped pack's arithmetic)
    float cap_rk;         // 2 / softcap: 2^(x * cap_rk) = e^(2 x / cap2) for a score x in log2 units
};

// What the per-sequence query count instantiations take (fa_kvcache_decode with seqlens_q): a LogitArgs pack plus the counts.  The
// CacheArgs' Nq1 is then the PADDED row count per query head; sequence b has n_b = min(max(seqlens_q[b], 0), Nq1) live rows per
// head, and n_b takes the place of Nq1 in every limit.
template <typename Base> struct RaggedArgs : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kRagged;
    const int* seqlens_q;   // [B] on the device, not null (without it the host runs the wrapped pack's kernels)
};

// What the token-packed instantiations take (fa_kvcache_decode_varlen): a RaggedArgs pack plus where the rows live.  Q and O are
// packed (total_q, Hkv*G, d) tensors read and written through their strides, lse is [Hkv*G, total_q], and sequence b owns the tokens
// [s_b, e_b) that cu_q gives under fa_forward_varlen's clamps; n_b = min(e_b - s_b, Nq1) takes the place of the seqlens_q count (the
// wrapped pack's seqlens_q is null and never read).  Strides in elements; every byte offset inside one (sequence, K/V head) view --
// rows [0, n_b) of the G heads of the group -- fits 32 bits (checked on the host).
template <typename Base> struct PackedArgs : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kPacked;
    const int* cu_q;        // [B + 1] on the device, not null
    int total_q;
    long long q_st, q_sh, o_st, o_sh;
};
// What the tree-mask instantiations take (fa_kvcache_decode_varlen_ex with a mask): a PackedArgs pack plus one 64-bit word per token
// row.  Bit j of token s_b + i's word: row i sees the step's own token j, the key at base_b + j with base_b = L_b - n_b; the keys below
// base_b are visible to every row.  The words take the place of the causal triangle (the host refuses causal != 1 and max_q > 64).
template <typename Base> struct TreeArgs : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kTree;
    const unsigned long long* tree_mask;   // [total_q] on the device, 8-byte aligned, not null
};
// What the routed instantiations take (the SHORT half of fa_kvcache_attend_varlen): a PackedArgs pack and nothing more -- the type alone
// says that a sequence with more than Nq1 rows has NO live row here (routed_rows) where the wrapped pack cuts it to its first Nq1: the
// tiled kernel owns such a sequence.  Its workgroups then take the n_b = 0 path and return before any table entry, K/V or Q row is read.
template <typename Base> struct RoutedArgs : Base {
    static constexpr unsigned kParts = Base::kParts | kvpart::kRouted;
};
// The kernel's one view of its trailing argument: the pack itself, or an empty struct for the plain instantiations.  Every field is
// read inside an `if constexpr` of its part's flag, so a pack without the part (and the empty struct) is never asked for it.  The merge
// kernel reads its Lse argument the same way.
struct NoPack {};
__device__ __forceinline__ NoPack pack_of() { return {}; }
template <typename A> __device__ __forceinline__ const A& pack_of(const A& a) { return a; }
// what a kPacked kernel keeps about its (sequence, K/V head) view -- all of it wave-uniform but the lane's offsets and (hd, i), which
// live in the prologue (qoff) or in the epilogue (the rest) only
struct PackedView {
    int s;                            // the sequence's first token
    __amdgpu_buffer_rsrc_t rq, ro;    // the views of Q and O
    unsigned qend, qoff, ooff;        // Q: the view's size (a dead lane's offset) and the lane's offset; O: the lane's offset
    unsigned hd, i;                   // the lane's head within the group and its row
    bool live;
};
// [s, s + n) of sequence b among the total_q token rows: fa_forward_varlen's clamps, cut to at most max_q rows (wave-uniform)
__device__ __forceinline__ void packed_rows(const int* __restrict__ cu, unsigned b, int total, int max_q, int& s, unsigned& n)
{
    s = min(max(cu[b], 0), total);
    n = (unsigned)min(min(max(cu[b + 1], s), total) - s, max_q);
}
// ... under RoutedArgs / RoutedLse: all of the sequence's rows if they are at most max_q, else none (wave-uniform)
__device__ __forceinline__ void routed_rows(const int* __restrict__ cu, unsigned b, int total, int max_q, int& s, unsigned& n)
{
    s = min(max(cu[b], 0), total);
    const int span = min(max(cu[b + 1], s), total) - s;
    n = span <= max_q ? (unsigned)span : 0u;
}
// the (sequence, K/V head) view of a packed tensor: rows [0, n) of the G heads from `h0` on; `bytes` is what a lane past the live
// rows uses as its offset (the first one past the view: loads read 0, stores are dropped)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t packed_rsrc(const void* ptr, int s, unsigned n, unsigned h0, unsigned G, long long st,
                                                              long long sh, int d, unsigned es, unsigned& bytes)
{
    const long long first = (long long)s * st + (long long)h0 * sh;
    bytes = n > 0 ? (unsigned)((unsigned long long)((long long)(n - 1) * st + (long long)(G - 1) * sh + d) * es) : 0u;
    return make_rsrc(static_cast<const char*>(ptr) + first * (long long)es, bytes);
}

// A wave-uniform float into a scalar register.  gfx950 has no scalar float arithmetic, so a value computed from kernel arguments
// lives in a VGPR unless it is read back; the d = 64 kernels sit at their 128 VGPRs and spill for every such value they keep.
__device__ __forceinline__ float to_sgpr(float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

// One sink joins a row's running (m, l), both in log2 units: the new reference is max(m, a2), `l` comes back as the sum under it
// and the return value is the factor the row's accumulators take.  m = -inf (no key) and a2 = -inf (no sink for the head) take the
// weight 0, not 2^(-inf + inf); with a2 = -inf the factor is 2^0 = 1 and (m, l) keep their bits.
__device__ __forceinline__ float sink_join(float a2, float& m, float& l)
{
    const float m_new = fmaxf(m, a2);
    const float w_keys = m == -INFINITY ? 0.0f : fast_exp2(m - m_new);
    const float w_sink = a2 == -INFINITY ? 0.0f : fast_exp2(a2 - m_new);
    l = l * w_keys + w_sink;
    m = m_new;
    return w_keys;
}

// Two e4m3fn bytes of w (kHi: bytes 2 and 3) as one packed pair of T.  Every e4m3fn value is a normal number of fp16 and of bf16,
// so the conversion is exact, and the NaN codes 0x7F / 0xFF stay NaN.  One v_cvt_scalef32_pk_{f16,bf16}_fp8 with a scale of 1.
// FA_FP8_VIA_F32 takes the way through fp32 (v_cvt_pk_f32_fp8, then the pack of the type), which is exact for the same reason.
#ifndef FA_FP8_VIA_F32
#define FA_FP8_VIA_F32 0
#endif
template <typename T, bool kHi> __device__ __forceinline__ unsigned fp8x2_widen(unsigned w) {
#if FA_FP8_VIA_F32
    const f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, kHi);
    return T::pack2(f[0], f[1]);
#else
    if constexpr (T::id == 0) return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, kHi));
    else return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, kHi));
#endif
}
// 16 e4m3fn bytes (one load) -> the two 16-byte LDS chunks of 8 elements of T they become
template <typename T> __device__ __forceinline__ void fp8x16_widen(u32x4 raw, u32x4& lo, u32x4& hi) {
    lo = u32x4{fp8x2_widen<T, false>(raw[0]), fp8x2_widen<T, true>(raw[0]), fp8x2_widen<T, false>(raw[1]), fp8x2_widen<T, true>(raw[1])};
    hi = u32x4{fp8x2_widen<T, false>(raw[2]), fp8x2_widen<T, true>(raw[2]), fp8x2_widen<T, false>(raw[3]), fp8x2_widen<T, true>(raw[3])};
}

// kPartial: write (O^T unnormalised, m, l) to the workspace instead of the normalised output.
// kCache: the key count L of the head's sequence is read on the device (Nk is then the capacity, the stride of a K/V head) and the
// split's chunk follows from L; every row has its own key limit; a row or a split without a key is neutral (m = -inf, l = 0, O = 0).
// With kCache false all of that compiles out and the kernel has the plain argument list (`cache` is empty).
// kPaged (kCache with a PagedArgs in the pack): a tile's rows come from pages.  The 16-byte loads one wave issues for one p cover
// 8 consecutive rows at D = 64 and 4 at D = 128, aligned to as many, so they lie inside ONE page of >= 16 keys: the page number is
// wave-uniform and goes into a scalar buffer descriptor per (wave, p), which ends at the page's last row below key1 (rows past it
// read 0 as the end of the contiguous descriptor does).  The page numbers of the tile after next are fetched while the current
// tile computes, so no tile but a split's first waits for the table.  Splits, tile order, masks and arithmetic are the kCache
// ones: on the same keys the result is bit-equal to the contiguous entry's.
// kFp8 (kCache with an Fp8Args in the pack): a K/V row is D bytes.  One 16-byte load carries 16 elements, the two adjacent LDS
// chunks 2c and 2c + 1 of a row, so a thread issues half the loads per tile (1 at D = 64, 2 at D = 128, each for K and for V),
// keeps the raw bytes across the tile's arithmetic and widens them in stage_write(): the LDS image, and everything that reads it,
// is the 16-bit kernels'.  One wave's loads for one p cover 16 rows at D = 64 and 8 at D = 128, aligned to as many -- still inside
// one page of >= 16 keys, so the paged scheme carries over with byte counts per one-byte element.  k_scale joins scale_log2e
// (the FLT_MIN clamp comes AFTER the product: +-FLT_MIN * 0.5 must not meet a masked -inf as 0); v_scale joins 1 / l in the
// one-pass kernel and the accumulators before the workspace store in the partial one, so the merge kernel is the 16-bit one.
// With scales of 1 the result is bit-equal to the 16-bit kernels' on the widened cache.
// kWindow (kCache with a WindowArgs around the pack): every row also has a LOWER key limit lo.  No row of the sequence sees a key
// below start_b (row 0's lower limit), so the splits deal out the tiles from start_t = start_b rounded down to a tile -- tiles stay
// at absolute multiples of kBlockN, which the paged scheme needs -- and nothing below start_t is touched.  The rows of the first
// tile below start_b are loaded (a page wholly below start_b is not: it gets a descriptor of zero records, and its table entry is
// not read) but reach LDS as zeros: masking the score is not enough for V, because a weight of 0 times a NaN is a NaN in the PV
// MFMA.  Scores of keys below a row's lo become -inf in the tiles that start below the last row's lower limit; a tile that is
// fully masked for a row is what m_ref = -inf already handles.
// kLogits (kWindow with a LogitArgs around the pack): two options on the logits.  Soft-cap: before the masks every score x = s c (log2
// units) becomes cap2 tanh(x / cap2), with tanh(y) = 1 - 2 / (1 + e^(2y)) on v_exp_f32 and v_rcp_f32, which saturates at both ends
// without a branch; the scores are then final, so the factor the vote and the weights multiply them by is 1 (`cs`).  The masks come
// AFTER the cap: tanh(-inf) = -1 would turn a masked key into the finite logit -cap2.  cap2 == 0 skips all of it by a wave-uniform
// branch, and the tile loop is the windowed kernel's.  Sinks: one extra key per row with the head's logit and a zero V row, joined to
// (m, l) by sink_join() in the one-pass epilogue here and in the merge kernel -- NEVER by a partial kernel: a row's sink counts once,
// however many splits its keys were dealt to.
// kRagged (kLogits with a RaggedArgs around the pack): sequence b has n_b <= Nq1 live rows per query head, read on the device, and
// n_b replaces Nq1 in start_b, in the causal limit and in the lower limit.  The G * n_b live rows of a K/V head are PACKED into the
// leading row blocks: packed row r' is row r' % n_b of head r' / n_b, and Q is loaded from (O and lse stored to) that row's padded
// address.  A lane past the live rows gets a row past the descriptors (its Q reads as zeros -- the caller's Q row is never loaded --
// and it stores nothing) and the limits of the last live row, so that it votes for a new reference maximum only in a tile in which
// that live row votes too: a dead row cannot move a live row's bits.  (With n_b = Nq1 no row is dead, and a lane past Nq keeps the
// limits the wrapped kernel gives it, so that the bits are the wrapped kernel's in every shape.)  The dead rows' zeros and -inf are written by the workgroup
// whose block holds their PADDED index (one-pass kernels; behind a split the merge writes them), and a workgroup whose block holds
// no live row returns before any table entry or K/V row is read -- with n_b = 0 that is every workgroup of the sequence.  The
// partial kernels store workspace rows by packed index.  Nothing of this lives in a VGPR across the tile loop: the row's limit
// takes the register the wrapped kernel keeps for it, and the one-pass epilogue derives the padded row again.
// The wrapped kernels' own expressions are left textually alone, with the ragged ones beside them: naming "rows per head" once for
// both changed the schedule of the windowed units (profiles/kvcache_ragged.txt).
// kPacked (kRagged with a PackedArgs around the pack): the rows of sequence b are the tokens [s_b, s_b + n_b) of packed (total_q,
// Hkv*G, d) tensors, n_b = min(e_b - s_b, Nq1) from the clamped cu_q pair.  Everything between the Q load and the O store is the
// ragged kernel's, the lane's packed row -> (head hd, row i) map with its limits for a lane past the live rows included, so the bits
// are the ragged kernel's on the padded copy of the same rows.  Q and O go through ONE scalar descriptor per (sequence, K/V head):
// it starts at token s_b of head hkv*G and spans the n_b rows of the G heads, a row's offset is i * stride_t + hd * stride_h, and a
// lane past the live rows uses the view's size as its offset (loads read 0, stores are dropped).  No dead row is written, by the
// one-pass kernels or by the merge (PackedLse): a token that is no live row keeps its O row and its lse entries.  lse goes to
// lse[hq * total_q + s_b + i] by a guarded store.  As under kRagged nothing new lives in a VGPR across the tile loop: the Q offset
// dies with the Q load, and the epilogue derives (hd, i) and the O offset from the thread id again (profiles/kvcache_decode_varlen.txt).
// kTree (kPacked with a TreeArgs around the pack): the causal triangle over the step's own n_b tokens becomes one 64-bit word per
// row.  With base = L - n_b (may be negative) the keys below base are visible to every row, key base + j to row i iff bit j of
// m_i = (word & low n_b bits) | 1 << i is set, and the row's lower limit is base + popcount(m_i) - window: its depth in its own
// branch where the triangle has its index.  Only the masking block of the tile loop differs, and only in the tiles that reach past
// max(base, 0) -- at most two per sequence, in whichever split they fall -- or start below the last lower limit.  The lane's word is
// loaded INSIDE that block, through a descriptor over the sequence's n_b words, from the row index that row_end already holds; a
// lane past the live rows loads nothing (its offset is the descriptor's size) and takes the triangle's word of that index, so it
// votes where the causal kernel's dead lane votes.  Nothing of the mask lives in a VGPR outside the block.  With
// the word (2 << i) - 1 every score takes the decision the kPacked causal kernel takes: the bits are that kernel's.
// kRouted (kPacked with a RoutedArgs around the pack): the one difference is the row count -- n_b = e_b - s_b when that
// is at most Nq1 and 0 otherwise -- taken where the packed kernel takes its own, so a sequence of up to Nq1 rows returns the packed
// kernel's bits and a longer one is an idle slot.  The decision is wave-uniform and is gone before the Q load.
// Why a parameter pack for one optional argument, and not a shared __device__ body behind two __global__ kernels: the plain
// instantiations must keep the parent's code.  Behind a wrapper the d = 128 plain kernels came out with another register
// allocation (204/205 -> 202/203 VGPRs, another schedule); with the pack their gfx950 assembly is the parent's, instruction for
// instruction (profiles/kvcache_decode.txt).  Do not simplify this without repeating that comparison.  The same holds for `Lse...`
// of the merge kernel below.
template <typename T, int D, bool kOutF32, bool kPartial, bool kCache = false, typename... Cache>
__global__ __launch_bounds__(64 * split::kW, D == 64 ? 4 : 2)
void fa_fwd_split_kernel(const uint16_t* __restrict__ Qg, const uint16_t* __restrict__ Kg,
                         const uint16_t* __restrict__ Vg, void* __restrict__ Og, float* __restrict__ ws,
                         int Nq, int Nk, int nqb, int S, int chunk, float scale_log2e, Cache... cache)
{
    static_assert(sizeof...(Cache) == (kCache ? 1 : 0), "the KV-cache instantiations take one CacheArgs or PagedArgs, the plain ones nothing");
    using G = TileGeom<D>;
    [[maybe_unused]] const CacheArgs ca = {cache...};
    [[maybe_unused]] const auto pa = pack_of(cache...);   // the whole pack; a part's fields are read under its flag only
    constexpr unsigned kParts = (0u | ... | Cache::kParts);
    constexpr bool kPaged = (kParts & kvpart::kPaged) != 0, kFp8 = (kParts & kvpart::kFp8) != 0, kWindow = (kParts & kvpart::kWindow) != 0;
    constexpr bool kLogits = (kParts & kvpart::kLogits) != 0, kRagged = (kParts & kvpart::kRagged) != 0;
    constexpr bool kPacked = (kParts & kvpart::kPacked) != 0, kTree = (kParts & kvpart::kTree) != 0, kRouted = (kParts & kvpart::kRouted) != 0;
    constexpr unsigned kKvRowBytes = kFp8 ? D : G::kRowBytes;      // bytes of one K or V row in memory
    constexpr unsigned kLdChunks = kFp8 ? D / 16 : G::kChunks;     // 16-byte loads per row
    using namespace split;
    constexpr int W = kW;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // block -> (head, query block, split): the splits of one (head, query block) are consecutive
    const unsigned sp = blockIdx.x % (unsigned)S;
    const unsigned rest = blockIdx.x / (unsigned)S;
    // kRouted: the query block is the SLOW index.  With Nq1 = T a one-token sequence has live rows in its block 0 alone, and with the
    // blocks of a head adjacent (bh * nqb + qb) the live workgroups sit at block ids that are multiples of nqb: for nqb = 4 on two of
    // the eight XCDs (block id % 8), with the other six idle (measured: 812 against 322 us at 256 x 1 tokens, T = 128, d = 64).
    // Block-major, the live workgroups are the first BH * S ids and spread over all of them.  Which workgroup computes what is
    // unchanged, and so are the bits.
    [[maybe_unused]] const unsigned nbh = kRouted ? gridDim.x / ((unsigned)S * (unsigned)nqb) : 1u;
    const unsigned bh = kRouted ? rest % nbh : rest / (unsigned)nqb, qb = kRouted ? rest / nbh : rest % (unsigned)nqb;

    const unsigned tid  = threadIdx.x;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u;
    const unsigned r = lane & 31u, h = lane >> 5;

    unsigned nkeys = (unsigned)Nk;   // keys of this head
    if constexpr (kCache) {
        // the clamp keeps a bad length inside the cache; the tiles of THIS sequence are dealt out to the S splits
        if (ca.seqlens) nkeys = (unsigned)min(max(ca.seqlens[bh / (unsigned)ca.Hkv], 0), Nk);
        if constexpr (!kWindow) chunk = (int)(((nkeys + kBlockN - 1) / kBlockN + (unsigned)S - 1) / (unsigned)S) * kBlockN;
    }
    // kRagged: the sequence's live rows per query head and per K/V head (wave-uniform).  The one-pass kernels write the dead rows
    // of this block's padded share -- two threads per row, half a row each -- and a block without a live packed row ends here.
    // kPacked: the count comes from the sequence's clamped cu_q pair, whose first token pv.s is where its rows start; no dead row
    // is written
    [[maybe_unused]] unsigned n_q = 0, live = 0;
    [[maybe_unused]] std::conditional_t<kPacked, PackedView, NoPack> pv;
    if constexpr (kRagged) {
        if constexpr (kRouted) routed_rows(pa.cu_q, bh / (unsigned)ca.Hkv, pa.total_q, ca.Nq1, pv.s, n_q);
        else if constexpr (kPacked) packed_rows(pa.cu_q, bh / (unsigned)ca.Hkv, pa.total_q, ca.Nq1, pv.s, n_q);
        else n_q = (unsigned)min(max(pa.seqlens_q[bh / (unsigned)ca.Hkv], 0), ca.Nq1);
        live = ((unsigned)Nq / (unsigned)ca.Nq1) * n_q;
        if constexpr (!kPartial && !kPacked) {
            const unsigned pr = qb * (unsigned)kRows + (tid >> 1);
            if (pr < (unsigned)Nq && pr % (unsigned)ca.Nq1 >= n_q) {
                constexpr unsigned es = kOutF32 ? 4u : 2u, kHalf = (unsigned)D * es / 2u;
                const __amdgpu_buffer_rsrc_t rz =
                    make_rsrc(reinterpret_cast<char*>(Og) + (size_t)bh * Nq * D * es, (unsigned)((size_t)Nq * D * es));
#pragma unroll
                for (unsigned o = 0; o < kHalf; o += 16u)
                    buf_store16(rz, pr * (unsigned)D * es + (tid & 1u) * kHalf + o, u32x4{0u, 0u, 0u, 0u});
                if (ca.lse && !(tid & 1u))
                    buf_store4(make_rsrc(ca.lse + (size_t)bh * Nq, (unsigned)Nq * 4u), pr * 4u, __float_as_uint(-INFINITY));
            }
        }
        if (qb * (unsigned)kRows >= live) return;   // workgroup-uniform; n_q >= 1 from here on
    }
    // kWindow: the first key any row of the sequence sees, the tile it lies in, and the tiles from there dealt out to the splits
    [[maybe_unused]] unsigned start_b = 0, start_t = 0;
    if constexpr (kWindow) {
        if constexpr (kRagged) start_b = (unsigned)max((int)nkeys - (int)n_q + 1 - pa.window, 0);
        else start_b = (unsigned)max((int)nkeys - ca.Nq1 + 1 - pa.window, 0);
        start_t = start_b & ~(unsigned)(kBlockN - 1);
        chunk = (int)(((nkeys - start_t + kBlockN - 1) / kBlockN + (unsigned)S - 1) / (unsigned)S) * kBlockN;
    }
    const unsigned key0 = (kWindow ? start_t : 0u) + sp * (unsigned)chunk;   // multiple of kBlockN
    const unsigned key1 = min(nkeys, key0 + (unsigned)chunk);         // exclusive
    // kPacked: Q is the (sequence, K/V head) view of the packed tensor -- the sequence's n_b token rows over the G heads of the group
    // (rq itself is then unused; it keeps its line so that the wrapped kernels' text stays as it was)
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(Qg + (size_t)bh * Nq * D, (unsigned)((size_t)Nq * D * 2));
    if constexpr (kPacked) {
        const unsigned grp = (unsigned)Nq / (unsigned)ca.Nq1;
        pv.rq = packed_rsrc(Qg, pv.s, n_q, (bh % (unsigned)ca.Hkv) * grp, grp, pa.q_st, pa.q_sh, D, 2u, pv.qend);
    }
    // K/V descriptors end at this split's last key: rows beyond it read 0 and are masked below
    // element offset -> address: the fp8 instantiations get byte pointers in Kg / Vg
    [[maybe_unused]] auto kv_at = [](const uint16_t* base, size_t elems) -> const void* {
        if constexpr (kFp8) return reinterpret_cast<const uint8_t*>(base) + elems;
        else return base + elems;
    };
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(kv_at(Kg, (size_t)bh * Nk * D), key1 * kKvRowBytes);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(kv_at(Vg, (size_t)bh * Nk * D), key1 * kKvRowBytes);

    constexpr int kLoadsW = (kBlockN * kLdChunks) / (64 * W);
    const unsigned q_row = qb * (unsigned)kRows + wave * 32u + r;   // kRagged: the PACKED row
    const bool has_rows = qb * (unsigned)kRows + wave * 32u < (kRagged ? live : (unsigned)Nq);   // wave-uniform
    // kRagged: the lane's packed row -> its padded row, where Q, O and lse live (a lane past the live rows: a row past every
    // descriptor), and its index within its head, which for such a lane is the last live row's -- except with n_b = Nq1, where no
    // row is dead and a lane past Nq keeps the index q_row % Nq1 the wrapped kernel gives it: its votes then fall in the same tiles,
    // which is what makes full counts return the wrapped kernel's bits in every shape.  Else io_row is q_row.
    // kPacked: the same map; Q is then loaded from row i of head hd of the view, and a lane past the live rows from past its end.
    [[maybe_unused]] unsigned rag_row1 = 0, rag_io = 0;
    if constexpr (kRagged) {
        const unsigned last = n_q == (unsigned)ca.Nq1 ? ~0u : live - 1u;   // wave-uniform
        const unsigned pc = min(q_row, last), hd = pc / n_q;
        rag_row1 = pc - hd * n_q;
        rag_io = q_row < live ? hd * (unsigned)ca.Nq1 + rag_row1 : (unsigned)Nq;
        if constexpr (kPacked) pv.qoff = q_row < live ? (rag_row1 * (unsigned)pa.q_st + hd * (unsigned)pa.q_sh) * 2u : pv.qend;
    }
    const unsigned io_row = kRagged ? rag_io : q_row;

    // first key a row does NOT see, and the smallest such limit of any row (tiles that end at or below it need no mask)
    [[maybe_unused]] unsigned lim = key1, lim_lo = key1;
    if constexpr (kCache) {
        if (ca.causal) {
            if constexpr (kRagged) {
                const int first = (int)nkeys - (int)n_q + 1;
                lim = min((unsigned)max(first + (int)rag_row1, 0), key1);
                lim_lo = min((unsigned)max(first, 0), key1);
            } else {
                const int first = (int)nkeys - ca.Nq1 + 1;   // limit of row 0 of a head; may be <= 0
                lim = min((unsigned)max(first + (int)(q_row % (unsigned)ca.Nq1), 0), key1);
                lim_lo = min((unsigned)max(first, 0), key1);
            }
        }
    }
    // kWindow: the row's causal limit before any clamp -- both of its limits follow from it in the few tiles that mask, so the row
    // keeps ONE register for them, as the kCache kernels do (at D = 64 a second one spills) -- and the largest lower limit of any
    // row: tiles that start at or past it need no lower mask
    [[maybe_unused]] int row_end = 0;
    [[maybe_unused]] unsigned lo_hi = 0;
    if constexpr (kWindow) {
        if constexpr (kRagged) row_end = (int)nkeys - (int)n_q + 1 + (int)rag_row1;
        else row_end = (int)nkeys - ca.Nq1 + 1 + (int)(q_row % (unsigned)ca.Nq1);
        lo_hi = (unsigned)max((int)nkeys - pa.window, 0);
    }

    // kCache: a scale of 0 must not turn a masked -inf into 0 * -inf.  Redundant behind host_scale_log2e() (fa_dispatch.hpp), which
    // hands every kernel +-FLT_MIN in place of 0: that host rule is what makes scale 0 safe, here and in the plain instantiations.
    // kFp8: the head's k_scale is part of the factor, and the clamp applies to the product; v_scale is used at the end
    [[maybe_unused]] float k_scale = 1.0f, v_scale = 1.0f;
    if constexpr (kFp8) {
        const unsigned hkv = bh % (unsigned)ca.Hkv;
        if (pa.k_scale) k_scale = pa.k_scale[hkv];
        if (pa.v_scale) v_scale = pa.v_scale[hkv];
    }
    const float c = kFp8 ? fmaxf(fabsf(scale_log2e * k_scale), 1.17549435e-38f)
                         : kCache ? fmaxf(fabsf(scale_log2e), 1.17549435e-38f) : fabsf(scale_log2e);
    const unsigned q_flip = scale_log2e < 0.0f ? 0x80008000u : 0u;
    // what a score is multiplied by on its way into the vote and the exponent: c, or 1 once the soft-cap has made the scores final
    // kLogits: that factor and the cap's two constants in scalar registers (to_sgpr), so that the kernel keeps no more VGPRs through
    // the tile loop than the windowed one: c itself is then dead after this point
    [[maybe_unused]] float cs = c, cap_k1 = 0.0f, cap_n2 = 0.0f;
    if constexpr (kLogits) {
        cs = to_sgpr(pa.cap2 > 0.0f ? 1.0f : c);
        cap_k1 = to_sgpr(c * pa.cap_rk);
        cap_n2 = to_sgpr(-2.0f * pa.cap2);
    }
    u32x4 qf[G::kKSteps];
#pragma unroll
    for (int s = 0; s < G::kKSteps; ++s) {
        u32x4 raw = buf_load16(rq, io_row * G::kRowBytes + (16u * s + 8u * h) * 2u);
        if constexpr (kPacked) raw = buf_load16(pv.rq, pv.qoff + (16u * s + 8u * h) * 2u);   // the first load is then dead
#pragma unroll
        for (int w = 0; w < 4; ++w) raw[w] ^= q_flip;
        qf[s] = raw;
    }

    unsigned g_off[kLoadsW], k_lds[kLoadsW], v_lds[kLoadsW];
#pragma unroll
    for (int p = 0; p < kLoadsW; ++p) {
        const unsigned idx = tid + p * 64u * W;
        const unsigned row = idx / kLdChunks, ch = idx % kLdChunks;
        g_off[p] = row * kKvRowBytes + ch * 16u;
        // kFp8: the load holds the LDS chunks 2 ch and 2 ch + 1; the second one's offset is the first's with bit 4 flipped, in
        // the K image (the swizzle XORs the chunk index) and in the V image (chunk & 3 is even)
        k_lds[p] = G::k_off(row, kFp8 ? 2u * ch : ch);
        v_lds[p] = G::kTileBytes + G::v_off(row, kFp8 ? 2u * ch : ch);
    }
    u32x4 kst[kLoadsW], vst[kLoadsW];
    // kPaged: the page numbers of the tile that is staged next, one per (wave, p), in scalar registers.  fetch_pages() reads
    // them for a tile; the entry index is clamped to the split's last live page, so no entry at or past ceil(L / page) is read
    // (a (wave, p) whose rows all lie at or past key1 gets a descriptor of zero records whatever the number says).
    [[maybe_unused]] int pg[kLoadsW];
    [[maybe_unused]] auto fetch_pages = [&](unsigned kv0) {
        if constexpr (kPaged) {
            const int* tbl = pa.table + (size_t)(bh / (unsigned)ca.Hkv) * (unsigned)pa.max_pages;
            const unsigned last = (key1 - 1u) >> pa.lg_page;   // only called with key1 > key0 >= 0
#pragma unroll
            for (int p = 0; p < kLoadsW; ++p) {
                const unsigned wrow = (wave * 64u + p * 64u * W) / kLdChunks;   // first row of the tile this wave loads with p
                unsigned e = min((kv0 + wrow) >> pa.lg_page, last);
                // kWindow: nor is an entry below start_b's page read (last is at or past it: key1 > start_b)
                if constexpr (kWindow) e = max(e, start_b >> pa.lg_page);
                pg[p] = __builtin_amdgcn_readfirstlane(tbl[e]);
            }
        }
    };
    auto stage_load = [&](unsigned kv0) {
#pragma unroll
        for (int p = 0; p < kLoadsW; ++p) {
            if constexpr (kPaged) {
                const unsigned page = 1u << pa.lg_page;
                const unsigned wrow = (wave * 64u + p * 64u * W) / kLdChunks;
                const unsigned first = (kv0 + wrow) & ~(page - 1u);             // first key of the page
                bool ok = (unsigned)pg[p] < (unsigned)pa.num_pages && first < key1;
                if constexpr (kWindow) ok = ok && first + page > start_b;   // a page wholly below the window: pg[p] is another page's
                // the page's rows below key1; a bad page number or a page past the split's end: no record, every load reads 0
                const unsigned bytes = ok ? min(page, key1 - first) * kKvRowBytes : 0u;
                // 64-bit: pools beyond 4 GiB are normal; only the offset inside one page-head block is 32 bit
                const size_t blk = (((size_t)(ok ? pg[p] : 0) * (unsigned)ca.Hkv + bh % (unsigned)ca.Hkv) << pa.lg_page) * D;
                const __amdgpu_buffer_rsrc_t pk = make_rsrc(kv_at(Kg, blk), bytes), pv = make_rsrc(kv_at(Vg, blk), bytes);
                const unsigned off = (kv0 * kKvRowBytes + g_off[p]) & (page * kKvRowBytes - 1u);
                kst[p] = buf_load16_nt(pk, off);
                vst[p] = buf_load16_nt(pv, off);
                continue;
            }
#if FA_SPLIT_NT
            kst[p] = buf_load16_nt(rk, kv0 * kKvRowBytes + g_off[p]);
            vst[p] = buf_load16_nt(rv, kv0 * kKvRowBytes + g_off[p]);
#else
            kst[p] = buf_load16(rk, kv0 * kKvRowBytes + g_off[p]);
            vst[p] = buf_load16(rv, kv0 * kKvRowBytes + g_off[p]);
#endif
        }
    };
    // kv0: the tile stage_load() was last called for
    auto stage_write = [&](unsigned buf, [[maybe_unused]] unsigned kv0) {
        if constexpr (kWindow) {
            if (kv0 < start_b) {   // workgroup-uniform, one tile per sequence: rows below the window go to LDS as zeros
#pragma unroll
                for (int p = 0; p < kLoadsW; ++p)
                    if (kv0 + (tid + p * 64u * W) / kLdChunks < start_b) kst[p] = vst[p] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int p = 0; p < kLoadsW; ++p) {
            if constexpr (kFp8) {
                u32x4 lo, hi;
                fp8x16_widen<T>(kst[p], lo, hi);
                lds_write16(smem, buf * G::kBufBytes + k_lds[p], lo);
                lds_write16(smem, buf * G::kBufBytes + (k_lds[p] ^ 16u), hi);
                fp8x16_widen<T>(vst[p], lo, hi);
                lds_write16(smem, buf * G::kBufBytes + v_lds[p], lo);
                lds_write16(smem, buf * G::kBufBytes + (v_lds[p] ^ 16u), hi);
                continue;
            }
            lds_write16(smem, buf * G::kBufBytes + k_lds[p], kst[p]);
            lds_write16(smem, buf * G::kBufBytes + v_lds[p], vst[p]);
        }
    };

    const unsigned k_rd_row = r * G::kRowBytes;
    const unsigned k_rd_swz = G::k_swz(r);
    const unsigned i16 = lane & 15u, vq = i16 >> 2, vp = i16 & 3u, vg = (lane >> 4) & 1u;
    unsigned v_rd[2];
#pragma unroll
    for (int par = 0; par < 2; ++par)
        v_rd[par] = G::kTileBytes + h * G::kDBlocks * 256u + ((vq ^ par) << 6) + vg * 32u + vp * 8u;

    f32x16 o[G::kDBlocks];
    f32x16 zero16;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero16[i] = 0.0f;
#pragma unroll
    for (int db = 0; db < G::kDBlocks; ++db) o[db] = zero16;
    float m_ref = kCache ? -INFINITY : 0.0f, l_part = 0.0f;

    // >= 1 by construction of S; kCache: 0 for a split that lies past the sequence's last key, which touches no K/V
    const int ntiles = (kCache && key0 >= nkeys) ? 0 : (int)((key1 - key0 + kBlockN - 1) / kBlockN);
    // Tiles are visited in a rotated order that differs per (head, split): the chunks of one head start a
    // power-of-two stride apart, and workgroups marching through them in lockstep would keep hitting the
    // same few HBM channels.  The streaming softmax does not care about the order.
    const unsigned rot = FA_SPLIT_ROTATE ? (sp * 5u + bh * 3u) % (unsigned)(kCache ? max(ntiles, 1) : ntiles) : 0u;
    auto tile_of = [&](int t) { const unsigned ti = (unsigned)t + rot; return ti >= (unsigned)ntiles ? ti - (unsigned)ntiles : ti; };
    if (!kCache || ntiles > 0) {   // workgroup-uniform
        if constexpr (kPaged) fetch_pages(key0 + tile_of(0) * kBlockN);
        stage_load(key0 + tile_of(0) * kBlockN);
        if constexpr (kPaged) fetch_pages(key0 + tile_of(min(1, ntiles - 1)) * kBlockN);
        stage_write(0, key0 + tile_of(0) * kBlockN);
        __syncthreads();
    }

    for (int t = 0; t < ntiles; ++t) {
        const unsigned cur = t & 1u;
        const char* kbuf = smem + cur * G::kBufBytes;
        const unsigned kv0 = key0 + tile_of(t) * kBlockN;
        if (t + 1 < ntiles) stage_load(key0 + tile_of(t + 1) * kBlockN);
        // the table read of the tile after next (a last tile re-reads its own entries) overlaps this tile's arithmetic
        if constexpr (kPaged) fetch_pages(key0 + tile_of(min(t + 2, ntiles - 1)) * kBlockN);

        // a wave whose 32 rows all lie past Nq (the usual case for a handful of query rows) only stages
        if (has_rows) {
        f32x16 s[2];
#pragma unroll
        for (int ks = 0; ks < G::kKSteps; ++ks)   // consecutive MFMAs alternate accumulators
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const u32x4 kf = lds_read16(kbuf, kb * 32u * G::kRowBytes + k_rd_row + (((2u * ks + h) ^ k_rd_swz) << 4));
                s[kb] = T::mfma32(kf, qf[ks], ks == 0 ? zero16 : s[kb]);
            }
        if constexpr (kLogits) {
            if (pa.cap2 > 0.0f) {   // wave-uniform; before the masks, so a masked key stays at -inf
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        s[kb][i] = __builtin_fmaf(cap_n2, __builtin_amdgcn_rcpf(1.0f + fast_exp2(s[kb][i] * cap_k1)), pa.cap2);
            }
        }
        if constexpr (kWindow) {
            // kTree: the tiles that hold one of the step's own tokens (keys from max(base, 0) on), the split's end or a row's lower
            // limit.  The lane's row index comes back from row_end, its word from memory, and both die with the block; the thread id
            // and row_end go through an empty asm so that "is my row live", the word's offset and the row's bit are derived here and
            // not kept in registers from the prologue (hoisted, they are five VGPRs across the loop, which the d = 64 kernels spill)
            if constexpr (kTree) {
                const int base = (int)nkeys - (int)n_q;   // wave-uniform
                if (kv0 + kBlockN > min((unsigned)max(base, 0), key1) || kv0 < lo_hi) {
                    unsigned t = tid;
                    int re = row_end;   // through the asm too: what follows from the row index is made here, not hoisted out of the loop
                    asm volatile("" : "+v"(t), "+v"(re));
                    const unsigned ri = (unsigned)(re - base - 1);   // < n_q for every lane
                    const bool lv = qb * (unsigned)kRows + (t >> 6) * 32u + (t & 31u) < live;
                    const u32x2 w = buf_load8(make_rsrc(pa.tree_mask + pv.s, n_q * 8u), lv ? ri * 8u : n_q * 8u);
                    unsigned long long m = ((unsigned long long)w[1] << 32) | w[0];
                    m = lv ? ((m & (~0ull >> (64u - n_q))) | (1ull << ri)) : ((2ull << ri) - 1ull);
                    // The tile's 64 keys as one word per lane, bit o for key kv0 + o, made in place in the two registers of m so that the
                    // block needs little more than the windowed one's (the d = 64 kernels have no register to spare).  The row's lower
                    // limit first, the only other per-lane value
                    const unsigned lo = (unsigned)max(base + (int)__builtin_popcountll(m) - pa.window, 0);
                    // ... the step's tokens the row sees, all keys below base, none from key1 on: d, and with it every shift and
                    // constant here, is wave-uniform (key1 > kv0: the tile exists)
                    const int d = (int)kv0 - base;
                    const unsigned upto = min(key1 - kv0, 64u);
                    const unsigned long long ends = upto < 64u ? (1ull << upto) - 1ull : ~0ull;
                    if (d >= 0) m = d < 64 ? m >> d : 0ull;
                    else m = d > -64 ? (m << -d) | ((1ull << -d) - 1ull) : ~0ull;
                    m &= ends;
                    // ... and none below lo
                    const unsigned below = lo > kv0 ? min(lo - kv0, 64u) : 0u;
                    m = below < 64u ? (m >> below) << below : 0ull;
                    m >>= (t >> 3) & 4u;   // the lane's keys start at kv0 + 4 h; h from t: see above
                    const unsigned vis2[2] = {(unsigned)m, (unsigned)(m >> 32)};
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            if (!(vis2[kb] & (1u << ((i & 3) + 8 * (i >> 2))))) s[kb][i] = -INFINITY;
                }
            } else
            // keys outside [lo, hi) -> -inf: hi is `lim` above, lo the row's lower limit; one unsigned compare per score
            if (kv0 + kBlockN > lim_lo || kv0 < lo_hi) {
                const unsigned lo = (unsigned)max(row_end - pa.window, 0);
                const unsigned hi = ca.causal ? min((unsigned)max(row_end, 0), key1) : key1;
                const unsigned seen = hi > lo ? hi - lo : 0u;   // a split that ends below lo: nothing
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const unsigned key = kv0 + (unsigned)(kb * 32 + (i & 3) + 8 * (i >> 2)) + 4u * h;
                        if (key - lo >= seen) s[kb][i] = -INFINITY;
                    }
            }
        } else if (kv0 + kBlockN > (kCache ? lim_lo : key1)) {   // keys past the split's end (kCache: past the row's limit) -> -inf (p = 0)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned key = kv0 + (unsigned)(kb * 32 + (i & 3) + 8 * (i >> 2)) + 4u * h;
                    if (key >= (kCache ? lim : key1)) s[kb][i] = -INFINITY;
                }
        }

        float tmax = -INFINITY;
#pragma unroll
        for (int e = 0; e < 32; e += 2) tmax = max3(tmax, s[e >> 4][e & 15], s[(e + 1) >> 4][(e + 1) & 15]);
        tmax *= kLogits ? cs : c;
        // kCache: a tile can be fully masked for a row, in any position of the rotated order, so m_ref starts at -inf and stays
        // there until the row meets a key.  The vote is written without a difference (-inf - -inf), and a row whose m_ref is
        // -inf takes alpha = 0 instead of 2^(-inf + inf); a first live key always wins the vote (tmax > -inf).
        if (kCache ? __any(tmax > m_ref + kThr) : (t == 0 || __any(tmax - m_ref > kThr))) {
            const float mx = fmaxf(tmax, swap_halves(tmax));
            const float m_new = (!kCache && t == 0) ? mx : fmaxf(mx, m_ref);
            const float alpha = (kCache ? m_ref == -INFINITY : t == 0) ? 0.0f : fast_exp2(m_ref - m_new);
            m_ref = m_new;
#pragma unroll
            for (int db = 0; db < G::kDBlocks; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
            l_part *= alpha;
        }

        u32x4 pk[4];
        float ls0 = 0.0f, ls1 = 0.0f;
        const float neg_m = (kCache && m_ref == -INFINITY) ? 0.0f : -m_ref;   // every s of such a row is -inf: p = 2^(-inf + 0) = 0
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int kb = q4 >> 1, b8 = (q4 & 1) * 8;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float p0 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w], kLogits ? cs : c, neg_m));
                const float p1 = fast_exp2(__builtin_fmaf(s[kb][b8 + 2 * w + 1], kLogits ? cs : c, neg_m));
                pk[q4][w] = T::pack2(p0, p1);
                if (w & 1) ls1 = T::sum2(pk[q4][w], ls1);   // sums of the ROUNDED weights (fa_common.hpp)
                else ls0 = T::sum2(pk[q4][w], ls0);
            }
        }
        l_part += ls0 + ls1;

#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int db = 0; db < G::kDBlocks; ++db) {
                u32x4 vf;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const u32x2 half = lds_read_tr8(kbuf, v_rd[db & 1] + ((4u * ks + 2u * jj) * G::kDBlocks + db) * 256u);
                    vf[2 * jj] = half[0];
                    vf[2 * jj + 1] = half[1];
                }
                o[db] = T::mfma32(vf, pk[ks], o[db]);
            }
        }   // has_rows

        if (t + 1 < ntiles) stage_write(cur ^ 1u, key0 + tile_of(t + 1) * kBlockN);
        __syncthreads();
    }

    float l = l_part + swap_halves(l_part);
    if constexpr (kPartial) {
        // workspace row (bh, sp, q_row): D floats of O^T (unnormalised), then m, then l
        const size_t rows = (size_t)Nq;
        const unsigned rs = (unsigned)(D + 2) * 4u;
        if constexpr (kFp8) {   // v_scale goes into the partial, so the merge kernel needs no scale
#pragma unroll
            for (int db = 0; db < G::kDBlocks; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[db][i] *= v_scale;
        }
        const __amdgpu_buffer_rsrc_t rw =
            make_rsrc(ws + ((size_t)bh * S + sp) * rows * (D + 2), (unsigned)(rows * rs));
        // kRagged: q_row is the PACKED row; the merge maps padded rows to it
#pragma unroll
        for (int db = 0; db < G::kDBlocks; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned col = db * 32u + 8u * g + 4u * h;
                // scalar copies first: __builtin_bit_cast applied to an ext-vector ELEMENT reads element 0
                const float a = o[db][4 * g], b = o[db][4 * g + 1], cc = o[db][4 * g + 2], d = o[db][4 * g + 3];
                // rows are (D+2)*4 bytes: 8-byte aligned, not 16 -> two 8-byte stores
                buf_store8(rw, q_row * rs + col * 4u, u32x2{__float_as_uint(a), __float_as_uint(b)});
                buf_store8(rw, q_row * rs + col * 4u + 8u, u32x2{__float_as_uint(cc), __float_as_uint(d)});
            }
        if (h == 0)
            buf_store8(rw, q_row * rs + (unsigned)D * 4u, u32x2{__float_as_uint(m_ref), __float_as_uint(l)});
    } else {
        // kRagged: the padded row once more, from the packed one and the two counts taken through an empty asm: kept from the
        // prologue it stays in a VGPR across the tile loop, and so does q_row once the prologue has divided it (the wrapped kernels
        // re-derive q_row from the thread id), which the d = 64 paged kernels spill; the counts themselves are scalar
        // kPacked: the same derivation also gives the row's head and index in the view, where O and lse go; o_row stays the padded
        // row, which names the head whose sink the row joins
        [[maybe_unused]] unsigned o_row = io_row;
        if constexpr (kRagged) {
            unsigned nq = n_q, lv = live, t = tid;
            asm volatile("" : "+s"(nq), "+s"(lv), "+v"(t));
            const unsigned pk = qb * (unsigned)kRows + (t >> 6) * 32u + (t & 31u);   // q_row, from the thread id again
            const unsigned pc = min(pk, lv - 1u), hd = pc / nq;
            o_row = pk < lv ? hd * (unsigned)ca.Nq1 + (pc - hd * nq) : (unsigned)Nq;
            if constexpr (kPacked) {
                pv.hd = hd;
                pv.i = pc - hd * nq;
                pv.live = pk < lv;
            }
        }
        // kLogits: the sink joins here, once per row; rows past Nq read the sink of the head's last row and store nothing
        [[maybe_unused]] float w_keys = 1.0f;
        if constexpr (kLogits) {
            if (pa.sinks) {
                // the two divisors go through an empty asm so that these divisions share nothing with `bh % ca.Hkv` and `q_row %
                // ca.Nq1` of the prologue: shared, two reciprocals stay in VGPRs across the tile loop, which the d = 64 kernels
                // spill (profiles/kvcache_logits.txt); recomputed here they cost a few instructions once per workgroup
                unsigned nq1 = (unsigned)ca.Nq1, nhkv = (unsigned)ca.Hkv;
                asm volatile("" : "+s"(nq1), "+s"(nhkv));
                const unsigned hq = (bh % nhkv) * ((unsigned)Nq / nq1) + min(o_row, (unsigned)Nq - 1u) / nq1;
                w_keys = sink_join(pa.sinks[hq] * kLog2e, m_ref, l);
            }
        }
        float inv = (kCache && l == 0.0f) ? 0.0f : 1.0f / l;   // a row without a key: O = 0
        if constexpr (kLogits) inv *= w_keys;
        if constexpr (kFp8) inv *= v_scale;
        if constexpr (kPacked) {
            // lse is [Hkv*G, total_q]: the live rows alone store, each to its own token's entry
            if (ca.lse && h == 0 && pv.live)
                ca.lse[((size_t)(bh % (unsigned)ca.Hkv) * ((unsigned)Nq / (unsigned)ca.Nq1) + pv.hd) * (size_t)pa.total_q + (size_t)pv.s + pv.i] =
                    l == 0.0f ? -INFINITY : (m_ref + __log2f(l)) * kLn2;
        } else if constexpr (kCache) {
            if (ca.lse && h == 0)   // m_ref is in log2 units; rows past Nq fall outside the descriptor
                buf_store4(make_rsrc(ca.lse + (size_t)bh * Nq, (unsigned)Nq * 4u), o_row * 4u,
                           __float_as_uint(l == 0.0f ? -INFINITY : (m_ref + __log2f(l)) * kLn2));
        }
        constexpr unsigned es = kOutF32 ? 4u : 2u;
        // kPacked: O is the view Q has, through O's strides; a lane past the live rows stores past its end
        const __amdgpu_buffer_rsrc_t ro =
            make_rsrc(reinterpret_cast<char*>(Og) + (size_t)bh * Nq * D * es, (unsigned)((size_t)Nq * D * es));
        if constexpr (kPacked) {
            const unsigned grp = (unsigned)Nq / (unsigned)ca.Nq1;
            unsigned oend;
            pv.ro = packed_rsrc(Og, pv.s, n_q, (bh % (unsigned)ca.Hkv) * grp, grp, pa.o_st, pa.o_sh, D, es, oend);
            pv.ooff = pv.live ? (pv.i * (unsigned)pa.o_st + pv.hd * (unsigned)pa.o_sh) * es : oend;
        }
#pragma unroll
        for (int db = 0; db < G::kDBlocks; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned col = db * 32u + 8u * g + 4u * h;
                const float a = o[db][4 * g] * inv, b = o[db][4 * g + 1] * inv;
                const float cc = o[db][4 * g + 2] * inv, d = o[db][4 * g + 3] * inv;
                if constexpr (kOutF32) {
                    const f32x4 v = {a, b, cc, d};
                    if constexpr (kPacked) buf_store16(pv.ro, pv.ooff + col * 4u, __builtin_bit_cast(u32x4, v));
                    else buf_store16(ro, (o_row * D + col) * 4u, __builtin_bit_cast(u32x4, v));
                } else {
                    if constexpr (kPacked) buf_store8(pv.ro, pv.ooff + col * 2u, u32x2{T::pack2(a, b), T::pack2(cc, d)});
                    else buf_store8(ro, (o_row * D + col) * 2u, u32x2{T::pack2(a, b), T::pack2(cc, d)});
                }
            }
    }
}

// One wave per (bh, row).  Lane = (slice, 4 output columns): the D/4 column groups times 64/(D/4) slices of
// the split axis, so that the S partials of a row are read by parallel lanes with independent loads instead
// of one lane walking them (a serial walk costs ~0.25 us per partial: 64 us at S = 128).
// kCache: a partial with m = -inf is neutral (weight 0, not 2^(-inf + inf)), a row of neutral partials gives O = 0, and the
// trailing float* argument (may be nullptr) receives ln(sum of exponentials) = (M + log2 L) ln 2.
// Four structs can take the float*'s place (the kernel reads the one it got through pack_of(), and its lse pointer through lse_of()).
// SinkLse: the row's head has an attention sink, which joins (M, L) here, once per row.
struct SinkLse {
    float* lse;           // as the float* of the kCache instantiations
    const float* sinks;   // [Hkv * G] on the device, not null
    int Hkv, Nq1;         // K/V heads per batch entry and rows per query head: row `row` of K/V head bh belongs to query head
};                        // (bh % Hkv) * (Nq / Nq1) + row / Nq1
// RaggedLse in the place of the float*: the merge behind the RaggedArgs partial kernels.  Output row `row` (padded) of K/V head bh is
// row i = row % Nq1 of its query head; with n_b = min(max(seqlens_q[bh / Hkv], 0), Nq1) it is dead for i >= n_b -- the wave writes
// zeros and -inf and reads no partial -- and else its partials are workspace row (row / Nq1) * n_b + i.  Sinks (may be null here)
// join the live rows as under SinkLse.
struct RaggedLse {
    float* lse;
    const float* sinks;       // [Hkv * G] on the device, or nullptr
    const int* seqlens_q;     // [B] on the device, not null
    int Hkv, Nq1;
};
// PackedLse in the place of the float*: the merge behind the PackedArgs partial kernels.  The grid is RaggedLse's, one wave per padded
// row; row i = row % Nq1 of head hd = row / Nq1 is live for i < n_b (packed_rows), reads workspace row hd * n_b + i and joins the
// sink as under RaggedLse; it stores O to token s_b + i of query head hkv*G + hd through the strides and lse into [Hkv*G, total_q].
// A wave with i >= n_b returns without writing anything.
struct PackedLse {
    float* lse;
    const float* sinks;       // [Hkv * G] on the device, or nullptr
    const int* cu_q;          // [B + 1] on the device, not null
    int Hkv, Nq1, total_q;
    long long o_st, o_sh;     // elements
};
// RoutedLse: PackedLse behind the RoutedArgs partial kernels -- the row count is routed_rows', so the waves of a sequence with more
// than Nq1 rows return without writing, as those of an idle slot do.
struct RoutedLse : PackedLse {};
// the lse pointer of whatever came in the float*'s place (the plain instantiations: none)
__device__ __forceinline__ float* lse_of() { return nullptr; }
__device__ __forceinline__ float* lse_of(float* p) { return p; }
template <typename L> __device__ __forceinline__ float* lse_of(const L& s) { return s.lse; }
// a live row's token and query head, and the first element of its O row (the overload for the other Lse types is never run: it
// stands in the dead arm of a ?: on a constant)
struct PackedRow { size_t tok, hq; };
template <typename L> __device__ __forceinline__ size_t packed_elem(const L&, const NoPack&) { return 0; }
__device__ __forceinline__ size_t packed_elem(const PackedLse& s, const PackedRow& r) { return r.tok * (size_t)s.o_st + r.hq * (size_t)s.o_sh; }
template <typename T, bool kOutF32, bool kCache = false, typename... Lse>
__global__ __launch_bounds__(64)
void fa_split_combine_kernel(const float* __restrict__ ws, void* __restrict__ Og, int BH, int Nq, int D, int S, Lse... lse_arg)
{
    static_assert(sizeof...(Lse) == (kCache ? 1 : 0), "the KV-cache instantiations take the lse pointer, the plain ones nothing");
    [[maybe_unused]] float* const lse = lse_of(lse_arg...);
    [[maybe_unused]] const auto la = pack_of(lse_arg...);   // the Lse value; a type's fields are read under its flag only
    constexpr bool kSink = (std::is_same_v<Lse, SinkLse> || ...);
    constexpr bool kRaggedM = (std::is_same_v<Lse, RaggedLse> || ...);
    constexpr bool kRoutedM = (std::is_same_v<Lse, RoutedLse> || ...);
    constexpr bool kPackedM = (std::is_same_v<Lse, PackedLse> || ...) || kRoutedM;
    const int cols4 = D / 4;             // 16 or 32
    const int nsl = 64 / cols4;          // 4 or 2 slices of the split axis
    const unsigned lane = threadIdx.x;
    const int c4 = (int)lane % cols4, sl = (int)lane / cols4;
    const long long rowi = blockIdx.x;   // bh * Nq + row
    const int row = (int)(rowi % Nq);
    const int bh = (int)(rowi / Nq);
    const size_t stride_s = (size_t)Nq * (D + 2);
    int ws_row = row;                    // the row's partials in the workspace
    if constexpr (kRaggedM) {
        const int n_q = min(max(la.seqlens_q[bh / la.Hkv], 0), la.Nq1), hd = row / la.Nq1, i = row - hd * la.Nq1;
        if (i >= n_q) {   // wave-uniform: a dead row
            if (sl != 0) return;
            if (lse && lane == 0) lse[rowi] = -INFINITY;
            const size_t off = ((size_t)bh * Nq + row) * D + 4 * c4;
            if constexpr (kOutF32) {
                float* o = static_cast<float*>(Og) + off;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = 0.0f;
            } else {
                unsigned* o = reinterpret_cast<unsigned*>(static_cast<uint16_t*>(Og) + off);
                o[0] = o[1] = 0u;
            }
            return;
        }
        ws_row = hd * n_q + i;
    }
    // kPackedM: the row's token and query head, where O and lse go
    [[maybe_unused]] std::conditional_t<kPackedM, PackedRow, NoPack> pm;
    if constexpr (kPackedM) {
        int s;
        unsigned n_q;
        if constexpr (kRoutedM) routed_rows(la.cu_q, (unsigned)(bh / la.Hkv), la.total_q, la.Nq1, s, n_q);
        else packed_rows(la.cu_q, (unsigned)(bh / la.Hkv), la.total_q, la.Nq1, s, n_q);
        const int hd = row / la.Nq1, i = row - hd * la.Nq1;
        if (i >= (int)n_q) return;   // wave-uniform: no live row, nothing is written
        ws_row = hd * (int)n_q + i;
        pm.tok = (size_t)s + (size_t)i;
        pm.hq = (size_t)(bh % la.Hkv) * (size_t)(Nq / la.Nq1) + (size_t)hd;
    }
    const float* base = ws + (size_t)bh * S * stride_s + (size_t)ws_row * (D + 2);
    // global reference max: every lane takes splits lane, lane+64, ...
    float M = -INFINITY;
    for (int s = (int)lane; s < S; s += 64) M = fmaxf(M, base[(size_t)s * stride_s + D]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    // kSink: the sink takes part in the reference maximum (a sink far above the keys' logits must not overflow the sum)
    [[maybe_unused]] float a2 = -INFINITY;
    if constexpr (kSink) {
        a2 = la.sinks[(bh % la.Hkv) * (Nq / la.Nq1) + row / la.Nq1] * kLog2e;
        M = fmaxf(M, a2);
    }
    if constexpr (kRaggedM) {
        if (la.sinks) a2 = la.sinks[(bh % la.Hkv) * (Nq / la.Nq1) + row / la.Nq1] * kLog2e;
        M = fmaxf(M, a2);
    }
    if constexpr (kPackedM) {
        if (la.sinks) a2 = la.sinks[pm.hq] * kLog2e;
        M = fmaxf(M, a2);
    }
    float L = 0.0f, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int s = sl; s < S; s += nsl) {
        const float* p = base + (size_t)s * stride_s;
        const float w = (kCache && p[D] == -INFINITY) ? 0.0f : fast_exp2(p[D] - M);
        L += p[D + 1] * w;
        // workspace rows are (D+2)*4 bytes: 8-byte aligned, so two 8-byte loads
        const float2 v0 = *reinterpret_cast<const float2*>(p + 4 * c4), v1 = *reinterpret_cast<const float2*>(p + 4 * c4 + 2);
        acc[0] += v0.x * w;
        acc[1] += v0.y * w;
        acc[2] += v1.x * w;
        acc[3] += v1.y * w;
    }
    // sum the slices: lanes that differ only in `sl` are cols4, 2*cols4, ... apart
    for (int o = cols4; o < 64; o <<= 1) {
        L += __shfl_xor(L, o, 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
    }
    if (sl != 0) return;
    if constexpr (kSink || kRaggedM || kPackedM) L += a2 == -INFINITY ? 0.0f : fast_exp2(a2 - M);   // after the slices are summed: once per row
    const float inv = (kCache && L == 0.0f) ? 0.0f : 1.0f / L;
    if constexpr (kPackedM) {
        if (lse && lane == 0) lse[pm.hq * (size_t)la.total_q + pm.tok] = L == 0.0f ? -INFINITY : (M + __log2f(L)) * kLn2;
    } else if constexpr (kCache) {
        if (lse && lane == 0) lse[rowi] = L == 0.0f ? -INFINITY : (M + __log2f(L)) * kLn2;
    }
    const size_t off = kPackedM ? packed_elem(la, pm) + 4 * c4 : ((size_t)bh * Nq + row) * D + 4 * c4;
    if constexpr (kOutF32) {
        float* o = static_cast<float*>(Og) + off;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = acc[i] * inv;
    } else {
        unsigned* o = reinterpret_cast<unsigned*>(static_cast<uint16_t*>(Og) + off);
        o[0] = T::pack2(acc[0] * inv, acc[1] * inv);
        o[1] = T::pack2(acc[2] * inv, acc[3] * inv);
    }
}

}  // namespace fa
