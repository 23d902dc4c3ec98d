// fa_fwd_kvdecode.hpp -- the host path every KV-cache decode entry shares: the pack of a (level, fp8, paged) cell, the pack builder,
// the launcher and the type switch.  The rule: level L wraps the pack of the level below it around the base the cache gives --
// CacheArgs or PagedArgs, inside an Fp8Args for an e4m3fn cache -- with kTree and kRouted both around kPacked's (PackFor).  That is
// 7 levels x {16-bit, fp8} x {contiguous, paged} = 28 packs, each behind one kvdecode_unit<level, fp8, paged>.  Private to the fifteen
// fa_fwd_kv*.hip units: this header instantiates kernels, so a unit instantiates only the cells it owns and no other unit's code
// moves (which unit owns which cell: DESIGN.md 7.21).
#pragma once
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

namespace fa {

template <KvLevel kLevel, typename Base> struct PackAt;
template <typename Base> struct PackAt<KvLevel::kPlain, Base> { using type = Base; };
template <typename Base> struct PackAt<KvLevel::kWindow, Base> { using type = WindowArgs<Base>; };   // around the base: kPlain has no window
template <typename Base> struct PackAt<KvLevel::kLogits, Base> { using type = LogitArgs<typename PackAt<KvLevel::kWindow, Base>::type>; };
template <typename Base> struct PackAt<KvLevel::kRagged, Base> { using type = RaggedArgs<typename PackAt<KvLevel::kLogits, Base>::type>; };
template <typename Base> struct PackAt<KvLevel::kPacked, Base> { using type = PackedArgs<typename PackAt<KvLevel::kRagged, Base>::type>; };
template <typename Base> struct PackAt<KvLevel::kTree, Base> { using type = TreeArgs<typename PackAt<KvLevel::kPacked, Base>::type>; };
template <typename Base> struct PackAt<KvLevel::kRouted, Base> { using type = RoutedArgs<typename PackAt<KvLevel::kPacked, Base>::type>; };
template <bool kPaged> using PagedOr = std::conditional_t<kPaged, PagedArgs, CacheArgs>;
template <KvLevel kLevel, bool kFp8, bool kPaged>
using PackFor = typename PackAt<kLevel, std::conditional_t<kFp8, Fp8Args<PagedOr<kPaged>>, PagedOr<kPaged>>>::type;

// The kernel's trailing argument for checked arguments: each part is filled where the pack has it.  The log-sum-exp pointer is left
// to the launcher.
template <typename Pack>
static Pack kvdecode_pack(const KvDecodeArgs& d, int lg_page)
{
    const KvCacheArgs& a = d.p.c;
    Pack pack;
    static_cast<CacheArgs&>(pack) = {a.seqlens, nullptr, a.Hkv, a.Nq, a.causal};
    if constexpr ((Pack::kParts & kvpart::kPaged) != 0) {
        pack.table = d.p.table;
        pack.max_pages = d.p.max_pages;
        pack.num_pages = d.p.num_pages;
        pack.lg_page = lg_page;
    }
    if constexpr ((Pack::kParts & kvpart::kFp8) != 0) {
        pack.k_scale = d.k_scale;
        pack.v_scale = d.v_scale;
    }
    if constexpr ((Pack::kParts & kvpart::kWindow) != 0) pack.window = d.window;
    if constexpr ((Pack::kParts & kvpart::kLogits) != 0) {
        pack.sinks = d.sinks;
        pack.cap2 = d.softcap * kLog2e;
        pack.cap_rk = d.softcap > 0.0f ? 2.0f / d.softcap : 0.0f;
    }
    if constexpr ((Pack::kParts & kvpart::kRagged) != 0) pack.seqlens_q = d.seqlens_q;
    if constexpr ((Pack::kParts & kvpart::kPacked) != 0) {   // the counts come from cu_q: seqlens_q stays null
        pack.cu_q = d.packed->cu_q;
        pack.total_q = d.packed->total_q;
        pack.q_st = d.packed->q_st;
        pack.q_sh = d.packed->q_sh;
        pack.o_st = d.packed->o_st;
        pack.o_sh = d.packed->o_sh;
    }
    if constexpr ((Pack::kParts & kvpart::kTree) != 0) pack.tree_mask = d.packed->tree_mask;
    return pack;
}

// The longest key range a sequence of a checked call can stream: the capacity, or window_span_cap() under a window -- which is the
// capacity again for a window that covers it, so window 0 and the capacity that stands in for it from kLogits up agree.
static inline int kvdecode_span(const KvDecodeArgs& d)
{
    return d.window == 0 ? d.p.c.Ncap : window_span_cap(d.p.c.Nq, d.p.c.Ncap, d.window);
}

// BH = B * Hkv K/V heads of Ncap rows, rows = G * Nq folded query rows per K/V head.  Split count, grid and workspace follow from
// the span and from the shape alone: nothing here reads lengths, table or scales, so a captured launch stays valid when any of them
// changes in place.
template <typename T, int D, bool kOutF32, typename Pack>
static hipError_t launch_kvdecode(const KvDecodeArgs& d, Pack pack)
{
    using G = TileGeom<D>;
    const KvCacheArgs& a = d.p.c;
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq, span = kvdecode_span(d);
    const int S = split_count(BH, rows, span);
    const int nqb = (rows + split::kRows - 1) / split::kRows;
    const long long nwg = (long long)BH * nqb * S;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!a.ws || a.ws_bytes < split_workspace_bytes(BH, rows, span, D))) return hipErrorInvalidValue;
    // the kernel's K/V parameters are typed for the 16-bit caches; the fp8 instantiations address them as bytes
    const uint16_t *q = static_cast<const uint16_t*>(a.Q), *k = static_cast<const uint16_t*>(a.K), *v = static_cast<const uint16_t*>(a.V);
    hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, false, true, Pack>), G::kLdsBytes);
    if (attr == hipSuccess) attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, true, true, Pack>), G::kLdsBytes);
    if (attr != hipSuccess) return attr;
    // the one-pass kernel stores the log-sum-exp itself; behind a split the merge does
    pack.lse = S == 1 ? a.lse : nullptr;
    // a window that covers the capacity is "every key" for every length: the clamp keeps the kernel's int arithmetic in range
    if constexpr ((Pack::kParts & kvpart::kWindow) != 0)
        if (pack.window > a.Ncap) pack.window = a.Ncap;
    if (S == 1) {
        FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, false, true, Pack>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                           a.stream, q, k, v, a.O, static_cast<float*>(nullptr), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pack);
        return launch_status();
    }
    FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, true, true, Pack>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                       a.stream, q, k, v, a.O, static_cast<float*>(a.ws), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pack);
    const hipError_t e = launch_status();
    return e != hipSuccess ? e : kvdecode_combine(d, S);   // the merge of the level, fa_fwd_kvcache.hip
}

// d has passed its entry's checks and the router: the capacity is filled in, the window is the level's, lg_page is the paged check's.
template <KvLevel kLevel, bool kFp8, bool kPaged>
hipError_t kvdecode_unit(const KvDecodeArgs& d, int lg_page)
{
    using Pack = PackFor<kLevel, kFp8, kPaged>;
    const KvCacheArgs& a = d.p.c;
    const Pack pack = kvdecode_pack<Pack>(d, lg_page);
    if (a.D == 64)
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            return launch_kvdecode<decltype(t), 64, decltype(f32)::value>(d, pack);
        });
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        return launch_kvdecode<decltype(t), 128, decltype(f32)::value>(d, pack);
    });
}

}  // namespace fa
