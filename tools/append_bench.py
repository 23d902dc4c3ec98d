#!/usr/bin/env python3
"""KV-cache append (fa_kvcache_append and its paged / fp8 forms) against the way the same job is done with torch alone.

    python tools/append_bench.py                       # B8 Hkv16 d128, Ncap 32768 at length 8192, Nnew 1 and 4096, the four layouts
    python tools/append_bench.py --alt-lib PATH        # a second build of the library as a third contender (e.g. -DFA_APPEND_NT_LOAD=0 or 2)
    python tools/append_bench.py --rope --G 1 4        # the rotary append (rotary_cos=, q=) against torch rotation ops + the plain entry

Method of tools/decode_bench.py --fp8: the contenders of one (layout, Nnew) run in one process, interleaved round by round, 5 rounds of
50 launches each between two device events; a line gives the median of the rounds and their range.  The torch baselines:
  contiguous   cache[:, :, L:L+Nnew] = new   -- torch's best case: the lengths are equal, so one slice assignment serves the batch
  paged        pool[page, :, row] = new      -- one index_put_ through precomputed (page, row) slot tensors [B, Nnew]
  fp8          quantize_kv_fp8(new, scale) first, then the same
The baselines know the length on the host; the library entry reads it on the device.  Before the timing the results of the two are
compared byte for byte.  For Nnew >= 1024 a line also gives GB/s over the bytes read plus the bytes written.
The verdict of a pair: the entry is "not slower" when its median is at most the baseline's median plus the baseline's round-to-round
spread (max - min of its rounds).
--rope adds Q [B, Hkv*G, Nnew, d] and fp32 tables (rot_dim = d, half-split) and times three contenders per (layout, G, Nnew):
  rope         fa_kvcache_append*(..., q=, rotary_cos=, rotary_sin=): K and Q rotated inside the append's launch
  torch+entry  what a caller does without it: positions from the device-side lengths, a gather of the table rows, the rotation of q and
               k_new with element-wise fp32 torch ops and a rounding to 16 bit, then the plain fa_kvcache_append* entry
  plain        the plain entry alone on the same shape (no rotation): context for what the extra bytes cost
Their results are compared first: equal bytes for a 16-bit cache and for Q; for an fp8 cache the composition rounds K to 16 bit before
the quantisation, so some codes differ and their number is printed.  The verdict is the one above, with torch+entry as the baseline.
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=16, help="K/V heads")
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--Ncap", type=int, default=32768)
    ap.add_argument("--len", type=int, default=8192, dest="L", help="keys every sequence holds before the append")
    ap.add_argument("--Nnew", type=int, nargs="+", default=[1, 4096])
    ap.add_argument("--page", type=int, default=16)
    ap.add_argument("--layouts", nargs="+", default=["contiguous", "paged", "fp8", "paged_fp8"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alt-lib", default=None, help="another build of libfa_mi355.so, timed as a third contender")
    ap.add_argument("--rope", action="store_true", help="time the rotary append against torch rotation ops + the plain entry")
    ap.add_argument("--G", type=int, nargs="+", default=[1, 4], help="query heads per K/V head (--rope)")
    ap.add_argument("--max-pos", type=int, default=None, help="rows of the cos / sin tables (--rope; default Ncap)")
    args = ap.parse_args()
    if args.rope:
        return rope_main(args)

    import torch
    import flashattention_kernel_project_amd as fa

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    B, H, d, Ncap, L, ps = args.B, args.H, args.d, args.Ncap, args.L, args.page
    dev = "cuda"
    alt = None
    if args.alt_lib:
        fa.lib()   # the shared HIP runtime first
        alt = ctypes.CDLL(args.alt_lib)
    print(f"{fa.version()}; B{B} Hkv{H} d{d} Ncap{Ncap} length {L}, pages of {ps}; median of {args.rounds} rounds of {args.iters} launches")
    g = torch.Generator(device="cpu").manual_seed(0)
    max_pages = Ncap // ps
    perm = torch.randperm(B * max_pages, generator=g).to(dev)
    table = perm.view(B, max_pages).to(torch.int32).contiguous()
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    k_scale = torch.rand(H, device=dev) * 0.02 + 0.005   # amax / 448 of N(0, 1) data is about 0.01
    v_scale = torch.rand(H, device=dev) * 0.02 + 0.005

    for layout in args.layouts:
        paged, fp8 = "paged" in layout, "fp8" in layout
        cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
        shape = (B * max_pages, H, ps, d) if paged else (B, H, Ncap, d)
        # caches of the entry, of the baseline and of the alternative build: zero-filled, so that they can be compared afterwards
        caches = {name: [torch.zeros(shape, dtype=torch.uint8 if fp8 else cdt, device=dev).view(cdt) for _ in range(2)]
                  for name in ["entry", "torch"] + (["alt"] if alt else [])}
        for Nnew in args.Nnew:
            kn = torch.randn(B, H, Nnew, d, device=dev).to(torch.bfloat16)
            vn = torch.randn(B, H, Nnew, d, device=dev).to(torch.bfloat16)
            pos = torch.arange(L, L + Nnew, device=dev)
            page = table.long()[:, (pos // ps)]            # [B, Nnew]
            row = (pos % ps).expand(B, Nnew)

            def entry(kc, vc):
                if paged and fp8:
                    fa.fa_kvcache_append_paged_fp8(kn, vn, kc, vc, table, k_scale, v_scale, cache_seqlens=lens)
                elif paged:
                    fa.fa_kvcache_append_paged(kn, vn, kc, vc, table, cache_seqlens=lens)
                elif fp8:
                    fa.fa_kvcache_append_fp8(kn, vn, kc, vc, k_scale, v_scale, cache_seqlens=lens)
                else:
                    fa.fa_kvcache_append(kn, vn, kc, vc, cache_seqlens=lens)

            def baseline(kc, vc):
                for new, cache, scale in ((kn, kc, k_scale), (vn, vc, v_scale)):
                    if fp8:
                        new = fa.quantize_kv_fp8(new, scale)[0].view(torch.uint8)
                        cache = cache.view(torch.uint8)
                    if paged:
                        cache[page, :, row] = new.permute(0, 2, 1, 3)
                    else:
                        cache[:, :, L:L + Nnew] = new

            def alt_call(kc, vc):
                vp = ctypes.c_void_p
                head = [vp(t.data_ptr()) for t in (kn, vn, kc, vc)] + [vp(lens.data_ptr()), None]
                sc = [vp(k_scale.data_ptr()), vp(v_scale.data_ptr())] if fp8 else []
                stream = vp(torch.cuda.current_stream().cuda_stream)
                if paged:
                    fn = alt.fa_kvcache_append_paged_fp8 if fp8 else alt.fa_kvcache_append_paged
                    code = fn(*head, vp(table.data_ptr()), *sc, B, H, Nnew, shape[0], ps, max_pages, d, 1, stream)
                else:
                    fn = alt.fa_kvcache_append_fp8 if fp8 else alt.fa_kvcache_append
                    code = fn(*head, *sc, B, H, Nnew, Ncap, d, 1, stream)
                assert code == 0, code

            calls = {"entry": entry, "torch": baseline}
            if alt:
                calls["alt"] = alt_call
            for name, fn in calls.items():
                for _ in range(3):
                    fn(*caches[name])
            torch.cuda.synchronize()
            raw = {name: [c.view(torch.uint8) for c in caches[name]] for name in calls}
            for name in calls:   # 16-bit: a copy, equal or wrong.  fp8: torch's GPU division and conversion are not the contract
                diff = sum(int((a != b).sum()) for a, b in zip(raw[name], raw["torch"]))   # (the CPU recipe is; tests hold it)
                assert fp8 or diff == 0, f"{layout} Nnew={Nnew}: {name} and torch wrote different caches"
                if diff:
                    print(f"{layout:10s} Nnew {Nnew:5d} [{name:5s}]: {diff} bytes differ from torch's GPU quantisation")
            assert int(torch.count_nonzero(raw["entry"][0])) > 0
            times = {name: [] for name in calls}
            for _ in range(args.rounds):   # the contenders alternate inside every round: drift hits all alike
                for name, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fn(*caches[name])
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / args.iters)
            med = {name: statistics.median(t) for name, t in times.items()}
            moved = 2.0 * B * H * Nnew * d * (2 + (1 if fp8 else 2))   # K and V: 16-bit rows read, rows written
            for name in calls:
                rate = f", {moved / med[name] / 1e6:.0f} GB/s over {moved / 1e6:.0f} MB read + written (decode streams 6300-6900 GB/s)" \
                    if Nnew >= 1024 else ""
                print(f"{layout:10s} Nnew {Nnew:5d} [{name:5s}]: median {med[name] * 1e3:8.1f} us "
                      f"(rounds {min(times[name]) * 1e3:.1f}-{max(times[name]) * 1e3:.1f}){rate}")
            spread = max(times["torch"]) - min(times["torch"])
            ok = med["entry"] <= med["torch"] + spread
            print(f"{layout:10s} Nnew {Nnew:5d}: entry / torch = {med['entry'] / med['torch']:.3f}; torch's rounds spread over "
                  f"{spread * 1e3:.1f} us: {'not slower' if ok else 'SLOWER beyond the spread'}")
            del kn, vn
        del caches
        torch.cuda.empty_cache()


def timed_rounds(calls, rounds, iters):
    """{name: fn} -> {name: [ms per launch of each round]}; the contenders alternate inside every round: drift hits all alike"""
    import torch
    times = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    return times


def rope_main(args):
    import torch
    import flashattention_kernel_project_amd as fa

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    B, H, d, Ncap, L, ps = args.B, args.H, args.d, args.Ncap, args.L, args.page
    dev, half = "cuda", args.d // 2
    max_pos = args.max_pos or Ncap
    layouts = [l for l in args.layouts if l in ("contiguous", "paged_fp8")] if args.layouts == ["contiguous", "paged", "fp8", "paged_fp8"] \
        else args.layouts
    print(f"{fa.version()}; rope: B{B} Hkv{H} d{d} rot_dim {d} half-split, Ncap{Ncap} length {L}, pages of {ps}, table of {max_pos} rows; "
          f"median of {args.rounds} rounds of {args.iters} launches")
    g = torch.Generator(device="cpu").manual_seed(0)
    max_pages = Ncap // ps
    table = torch.randperm(B * max_pages, generator=g).to(dev).view(B, max_pages).to(torch.int32).contiguous()
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    k_scale = torch.rand(H, device=dev) * 0.02 + 0.005
    v_scale = torch.rand(H, device=dev) * 0.02 + 0.005
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, d, 2, dtype=torch.float64) / d))[None]
    cos, sin = ang.cos().float().to(dev).contiguous(), ang.sin().float().to(dev).contiguous()

    for layout in layouts:
        paged, fp8 = "paged" in layout, "fp8" in layout
        cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
        shape = (B * max_pages, H, ps, d) if paged else (B, H, Ncap, d)
        fn = {(False, False): fa.fa_kvcache_append, (True, False): fa.fa_kvcache_append_paged, (False, True): fa.fa_kvcache_append_fp8,
              (True, True): fa.fa_kvcache_append_paged_fp8}[paged, fp8]
        extra = ((table,) if paged else ()) + ((k_scale, v_scale) if fp8 else ())
        caches = {name: [torch.zeros(shape, dtype=torch.uint8 if fp8 else cdt, device=dev).view(cdt) for _ in range(2)]
                  for name in ("rope", "torch+entry", "plain")}
        for G in args.G:
            for Nnew in args.Nnew:
                kn = torch.randn(B, H, Nnew, d, device=dev).to(torch.bfloat16)
                vn = torch.randn(B, H, Nnew, d, device=dev).to(torch.bfloat16)
                q0 = torch.randn(B, H * G, Nnew, d, device=dev).to(torch.bfloat16)
                qs = {name: q0.clone() for name in ("rope", "torch+entry")}
                q_out = torch.empty_like(q0)
                steps = torch.arange(Nnew, device=dev)

                def rotate(x, c, s):
                    xf = x.float()
                    x1, x2 = xf[..., :half], xf[..., half:]
                    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)

                def fused():
                    fn(kn, vn, *caches["rope"], *extra, cache_seqlens=lens, q=qs["rope"], q_out=q_out, rotary_cos=cos, rotary_sin=sin)

                def composition():
                    pos = (lens.long()[:, None] + steps[None]).clamp(max=max_pos - 1)   # from the device-side lengths
                    c, s = cos[pos][:, None], sin[pos][:, None]                         # [B, 1, Nnew, half]
                    composition.q = rotate(qs["torch+entry"], c, s)
                    fn(rotate(kn, c, s), vn, *caches["torch+entry"], *extra, cache_seqlens=lens)

                def plain():
                    fn(kn, vn, *caches["plain"], *extra, cache_seqlens=lens)

                calls = {"rope": fused, "torch+entry": composition, "plain": plain}
                for pair in caches.values():   # rows of an earlier (G, Nnew) would count in the comparison below
                    for c in pair:
                        c.view(torch.uint8).zero_()
                for f in calls.values():
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                tag = f"{layout:10s} G{G} Nnew {Nnew:5d}"
                if not torch.equal(q_out.view(torch.int16), composition.q.view(torch.int16)):
                    print(f"{tag}: Q DIFFERS from torch's rotation")
                raw = {name: [c.view(torch.uint8) for c in caches[name]] for name in calls}
                diff = int((raw["rope"][0] != raw["torch+entry"][0]).sum())
                if not torch.equal(raw["rope"][1], raw["torch+entry"][1]) or (diff and not fp8):
                    print(f"{tag}: the caches DIFFER from the composition's")
                assert int(torch.count_nonzero(raw["rope"][0])) > 0
                if diff:
                    print(f"{tag}: {diff} of {B * H * Nnew * d} K codes differ from the composition's (its 16-bit rounding before the "
                          "quantisation)")
                times = timed_rounds(calls, args.rounds, args.iters)
                med = {name: statistics.median(t) for name, t in times.items()}
                kv = 2.0 * B * H * Nnew * d * (2 + (1 if fp8 else 2))            # K and V: 16-bit rows read, rows written
                moved = {"rope": kv + 4.0 * B * H * G * Nnew * d, "plain": kv}   # Q: read and written, 16 bit
                for name in calls:
                    rate = f", {moved[name] / med[name] / 1e6:.0f} GB/s over {moved[name] / 1e6:.0f} MB read + written" \
                        if Nnew >= 1024 and name in moved else ""
                    print(f"{tag} [{name:11s}]: median {med[name] * 1e3:8.1f} us "
                          f"(rounds {min(times[name]) * 1e3:.1f}-{max(times[name]) * 1e3:.1f}){rate}")
                spread = max(times["torch+entry"]) - min(times["torch+entry"])
                ok = med["rope"] <= med["torch+entry"] + spread
                print(f"{tag}: rope / torch+entry = {med['rope'] / med['torch+entry']:.3f}, rope / plain = "
                      f"{med['rope'] / med['plain']:.3f}; torch+entry's rounds spread over {spread * 1e3:.1f} us: "
                      f"{'not slower' if ok else 'SLOWER beyond the spread'}")
                del kn, vn, q0, qs, q_out
                composition.q = None
                torch.cuda.empty_cache()
        del caches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
