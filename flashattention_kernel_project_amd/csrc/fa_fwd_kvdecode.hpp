// fa_fwd_kvdecode.hpp -- the host path the eight KV-cache decode entries share: the pack builder, the launcher and the type switch,
// templates over the pack (CacheArgs, PagedArgs, Fp8Args<...>, WindowArgs<...>, LogitArgs<...>, RaggedArgs<...>, PackedArgs<...>, TreeArgs<...>) the kernel
// takes.  Private to the fifteen translation units that each own the kernels of their packs (fa_fwd_kvcache.hip, _kvpaged, _kvfp8, _kvwindow,
// _kvwindow_fp8, _kvlogits, _kvlogits_fp8, _kvragged, _kvragged_fp8, _kvpacked, _kvpacked_fp8, _kvtree, _kvtree_fp8, _kvrouted, _kvrouted_fp8): it instantiates
// kernels, so a unit names only its own packs and no other unit's code moves.
#pragma once
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

namespace fa {

// The kernel's trailing argument for checked arguments (kvdecode_dispatch): each part is filled where the pack has it.  The
// log-sum-exp pointer is left to the launcher.
template <typename Pack>
static Pack kvdecode_pack(const KvDecodeArgs& d, int lg_page)
{
    const KvCacheArgs& a = d.p.c;
    Pack pack;
    static_cast<CacheArgs&>(pack) = {a.seqlens, nullptr, a.Hkv, a.Nq, a.causal};
    if constexpr (std::is_base_of_v<PagedArgs, Pack>) {
        pack.table = d.p.table;
        pack.max_pages = d.p.max_pages;
        pack.num_pages = d.p.num_pages;
        pack.lg_page = lg_page;
    }
    if constexpr (IsFp8Args<Pack>::value) {
        pack.k_scale = d.k_scale;
        pack.v_scale = d.v_scale;
    }
    if constexpr (IsWindowArgs<Pack>::value) pack.window = d.window;
    if constexpr (IsLogitArgs<Pack>::value) {
        pack.sinks = d.sinks;
        pack.cap2 = d.softcap * kLog2e;
        pack.cap_rk = d.softcap > 0.0f ? 2.0f / d.softcap : 0.0f;
    }
    if constexpr (IsRaggedArgs<Pack>::value) pack.seqlens_q = d.seqlens_q;
    if constexpr (IsPackedArgs<Pack>::value) {   // the counts come from cu_q: seqlens_q stays null
        pack.cu_q = d.packed->cu_q;
        pack.total_q = d.packed->total_q;
        pack.q_st = d.packed->q_st;
        pack.q_sh = d.packed->q_sh;
        pack.o_st = d.packed->o_st;
        pack.o_sh = d.packed->o_sh;
    }
    if constexpr (IsTreeArgs<Pack>::value) pack.tree_mask = d.packed->tree_mask;
    return pack;
}

// BH = B * Hkv K/V heads of Ncap rows, rows = G * Nq folded query rows per K/V head.  span: the longest key range a sequence can
// stream -- the capacity, or window_span_cap() under a window.  Split count, grid and workspace follow from it and from the shape
// alone: nothing here reads lengths, table or scales, so a captured launch stays valid when any of them changes in place.
template <typename T, int D, bool kOutF32, typename Pack>
static hipError_t launch_kvdecode(const KvCacheArgs& a, Pack pack, int span)
{
    using G = TileGeom<D>;
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq;
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
    if constexpr (IsWindowArgs<Pack>::value)
        if (pack.window > a.Ncap) pack.window = a.Ncap;
    if (S == 1) {
        FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, false, true, Pack>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                           a.stream, q, k, v, a.O, static_cast<float*>(nullptr), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pack);
        return launch_status();
    }
    FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, true, true, Pack>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                       a.stream, q, k, v, a.O, static_cast<float*>(a.ws), rows, a.Ncap, nqb, S, 0, host_scale_log2e(a.scale), pack);
    hipError_t e = launch_status();
    if (e != hipSuccess) return e;
    // routed rows: the packed merge with the routed row count (a sequence above max_q rows has no live row)
    if constexpr (IsRoutedArgs<Pack>::value)
        return kvrouted_combine(a.ws, a.O, a.lse, pack.sinks, {pack.cu_q, pack.total_q, pack.q_st, pack.q_sh, pack.o_st, pack.o_sh, nullptr}, BH, rows,
                                a.Hkv, a.Nq, D, S, a.in_dtype, a.out_dtype, a.stream);
    // token-packed rows: the merge stores the live rows to their tokens through O's strides and writes nothing else
    else if constexpr (IsPackedArgs<Pack>::value)
        return kvpacked_combine(a.ws, a.O, a.lse, pack.sinks, {pack.cu_q, pack.total_q, pack.q_st, pack.q_sh, pack.o_st, pack.o_sh, nullptr}, BH, rows,
                                a.Hkv, a.Nq, D, S, a.in_dtype, a.out_dtype, a.stream);
    // per-sequence query counts: the merge maps padded rows to the packed workspace rows, writes the dead rows and joins the sinks
    else if constexpr (IsRaggedArgs<Pack>::value)
        return kvragged_combine(a.ws, a.O, a.lse, pack.sinks, pack.seqlens_q, BH, rows, a.Hkv, a.Nq, D, S, a.in_dtype, a.out_dtype, a.stream);
    // the partial kernels leave the sinks alone: the merge joins them, once per row
    else if constexpr (IsLogitArgs<Pack>::value)
        if (pack.sinks) return kvlogits_combine(a.ws, a.O, a.lse, pack.sinks, BH, rows, a.Hkv, a.Nq, D, S, a.in_dtype, a.out_dtype, a.stream);
    return kvcache_combine(a.ws, a.O, a.lse, BH, rows, D, S, a.in_dtype, a.out_dtype, a.stream);
}

// What a unit's hand-over function calls, once per pack it owns: d has passed kvdecode_dispatch's checks (the capacity is filled
// in, lg_page is the paged check's).
template <typename Pack>
static hipError_t dispatch_kvdecode(const KvDecodeArgs& d, int lg_page)
{
    const KvCacheArgs& a = d.p.c;
    const Pack pack = kvdecode_pack<Pack>(d, lg_page);
    int span = a.Ncap;
    if constexpr (IsWindowArgs<Pack>::value) span = window_span_cap(a.Nq, a.Ncap, d.window);
    if (a.D == 64)
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            return launch_kvdecode<decltype(t), 64, decltype(f32)::value>(a, pack, span);
        });
    return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
        return launch_kvdecode<decltype(t), 128, decltype(f32)::value>(a, pack, span);
    });
}

}  // namespace fa
