// fa_fwd_kvcache.hip -- decode against a pre-allocated KV cache (fa_forward_kvcache): the split-KV stream of fa_fwd_split.hip with
// the key count of each sequence read on the device, a causal mask aligned to the end of the cache and a log-sum-exp output.
// DESIGN.md section 7 has the reasoning.  Owns the plain 16-bit contiguous kernels.  Also here, once for all decode entries: the
// argument checks, the entry kvdecode_dispatch, the router from a checked call to its kernels and every merge kernel.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

size_t kvcache_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D)
{
    if (B <= 0 || Hkv <= 0 || G <= 0 || Nq <= 0 || Ncap <= 0 || (D != 64 && D != 128)) return 0;
    if ((long long)B * Hkv > 0x7FFFFFFFll || (long long)G * Nq > 0x7FFFFFFFll) return 0;
    return split_workspace_bytes(B * Hkv, G * Nq, Ncap, D);
}

// What every KV-cache entry rejects before the device is touched (the fp8 entries too: their one-byte elements keep the 16-bit
// bound on the byte offsets).
hipError_t kvcache_check(const KvCacheArgs& a)
{
    if (!a.Q || !a.K || !a.V || !a.O) return hipErrorInvalidValue;
    if (a.B <= 0 || a.Hkv <= 0 || a.G <= 0 || a.Nq <= 0 || a.Ncap <= 0 || (a.D != 64 && a.D != 128)) return hipErrorInvalidValue;
    if (a.causal != 0 && a.causal != 1) return hipErrorInvalidValue;
    if (a.in_dtype != 0 && a.in_dtype != 1) return hipErrorInvalidValue;
    if (a.out_dtype != 0 && a.out_dtype != 1) return hipErrorInvalidValue;
    if ((long long)a.B * a.Hkv > 0x7FFFFFFFll || (long long)a.G * a.Nq > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const int rows = a.G * a.Nq;
    // per-head byte offsets are 32 bit: the checks of split_dispatch, on the folded rows and the capacity
    if (((unsigned long long)rows + split::kRows) * (unsigned)(a.D + 2) * 4ull >= (1ull << 32)) return hipErrorInvalidValue;
    if (((unsigned long long)a.Ncap + kBlockN) * (unsigned)a.D * 2ull >= (1ull << 32)) return hipErrorInvalidValue;
    return hipSuccess;
}

// The one entry behind the eight fa_forward_kvcache* functions and fa_kvcache_decode: the checks, once, then the lowest level that
// has what the call asks for.
hipError_t kvdecode_dispatch(const KvDecodeArgs& d)
{
    if (d.window < 0) return hipErrorInvalidValue;
    if (!(d.softcap >= 0.0f) || __builtin_isinf(d.softcap)) return hipErrorInvalidValue;   // negative, NaN or inf
    KvDecodeArgs q = d;   // ... with the capacity, from the paged check
    int lg_page = 0;
    const hipError_t bad = d.paged ? kvpaged_check(d.p, q.p, lg_page) : kvcache_check(d.p.c);
    if (bad != hipSuccess) return bad;
    q.level = d.seqlens_q                      ? KvLevel::kRagged
              : d.sinks || d.softcap != 0.0f ? KvLevel::kLogits
              : d.window != 0                 ? KvLevel::kWindow
                                              : KvLevel::kPlain;
    return kvdecode_route(q, lg_page);
}

// The router below names all 28 cells with kvdecode_unit's definition in sight; each is instantiated in the unit that owns its
// kernels and nowhere by use, so implicit instantiation is switched off for all of them, and this unit's own cell follows.
#define FA_KVDECODE_EXTERN(level)                                                                       \
    extern template hipError_t kvdecode_unit<KvLevel::level, false, false>(const KvDecodeArgs&, int); \
    extern template hipError_t kvdecode_unit<KvLevel::level, false, true>(const KvDecodeArgs&, int);  \
    extern template hipError_t kvdecode_unit<KvLevel::level, true, false>(const KvDecodeArgs&, int);  \
    extern template hipError_t kvdecode_unit<KvLevel::level, true, true>(const KvDecodeArgs&, int);
FA_KVDECODE_EXTERN(kPlain)
FA_KVDECODE_EXTERN(kWindow)
FA_KVDECODE_EXTERN(kLogits)
FA_KVDECODE_EXTERN(kRagged)
FA_KVDECODE_EXTERN(kPacked)
FA_KVDECODE_EXTERN(kTree)
FA_KVDECODE_EXTERN(kRouted)
#undef FA_KVDECODE_EXTERN
template hipError_t kvdecode_unit<KvLevel::kPlain, false, false>(const KvDecodeArgs&, int);

template <KvLevel kLevel>
static hipError_t route_cache(const KvDecodeArgs& d, int lg_page)
{
    if (d.fp8) return d.paged ? kvdecode_unit<kLevel, true, true>(d, lg_page) : kvdecode_unit<kLevel, true, false>(d, lg_page);
    return d.paged ? kvdecode_unit<kLevel, false, true>(d, lg_page) : kvdecode_unit<kLevel, false, false>(d, lg_page);
}

// Checked arguments (level, fp8, paged) -> the instantiation: the one list of the 28 packs.  The packs from kLogits up wrap a
// WindowArgs whatever the call's window, so window 0 runs there as window = Ncap: include/fa_mi355.h guarantees that to be the
// un-windowed result bit for bit, and kvdecode_span() gives it the same split count.
hipError_t kvdecode_route(const KvDecodeArgs& checked, int lg_page)
{
    KvDecodeArgs d = checked;
    if (d.level >= KvLevel::kLogits && d.window == 0) d.window = d.p.c.Ncap;
    switch (d.level) {
    case KvLevel::kPlain: return route_cache<KvLevel::kPlain>(d, lg_page);
    case KvLevel::kWindow: return route_cache<KvLevel::kWindow>(d, lg_page);
    case KvLevel::kLogits: return route_cache<KvLevel::kLogits>(d, lg_page);
    case KvLevel::kRagged: return route_cache<KvLevel::kRagged>(d, lg_page);
    case KvLevel::kPacked: return route_cache<KvLevel::kPacked>(d, lg_page);
    case KvLevel::kTree: return route_cache<KvLevel::kTree>(d, lg_page);
    case KvLevel::kRouted: return route_cache<KvLevel::kRouted>(d, lg_page);
    }
    return hipErrorInvalidValue;
}

// The merge behind a split, for every level: one wave per output row (the padded rows where the counts are the device's), and the
// Lse value that tells the kernel what a row is -- float*: rows as they are; SinkLse: a sink joins each row; RaggedLse: seqlens_q says
// which rows are live, the dead ones are written as zeros; PackedLse: live rows go to their tokens, nothing else is written;
// RoutedLse: the same with the routed row count.  The merge kernels are instantiated in this translation unit only.
hipError_t kvdecode_combine(const KvDecodeArgs& d, int S)
{
    const KvCacheArgs& a = d.p.c;
    const int BH = a.B * a.Hkv, rows = a.G * a.Nq;
    const long long out_rows = (long long)BH * rows;
    if (out_rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    auto launch = [&](auto lse) {
        return with_types(a.in_dtype, a.out_dtype, [&](auto t, auto f32) {
            FA_LAUNCH((fa_split_combine_kernel<decltype(t), decltype(f32)::value, true, decltype(lse)>), dim3((unsigned)out_rows), dim3(64), 0,
                      a.stream, static_cast<const float*>(a.ws), a.O, BH, rows, a.D, S, lse);
            return launch_status();
        });
    };
    if (d.level >= KvLevel::kPacked) {
        const PackedLse packed = {a.lse, d.sinks, d.packed->cu_q, a.Hkv, a.Nq, d.packed->total_q, d.packed->o_st, d.packed->o_sh};
        return d.level == KvLevel::kRouted ? launch(RoutedLse{packed}) : launch(packed);
    }
    if (d.level == KvLevel::kRagged) return launch(RaggedLse{a.lse, d.sinks, d.seqlens_q, a.Hkv, a.Nq});
    if (d.level == KvLevel::kLogits && d.sinks) return launch(SinkLse{a.lse, d.sinks, a.Hkv, a.Nq});
    return launch(a.lse);
}

}  // namespace fa
