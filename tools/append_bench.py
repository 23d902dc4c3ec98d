#!/usr/bin/env python3
"""KV-cache append (fa_kvcache_append and its paged / fp8 forms) against the way the same job is done with torch alone.

    python tools/append_bench.py                       # B8 Hkv16 d128, Ncap 32768 at length 8192, Nnew 1 and 4096, the four layouts
    python tools/append_bench.py --alt-lib PATH        # a second build of the library as a third contender (e.g. -DFA_APPEND_NT_LOAD=0 or 2)

Method of tools/decode_bench.py --fp8: the contenders of one (layout, Nnew) run in one process, interleaved round by round, 5 rounds of
50 launches each between two device events; a line gives the median of the rounds and their range.  The torch baselines:
  contiguous   cache[:, :, L:L+Nnew] = new   -- torch's best case: the lengths are equal, so one slice assignment serves the batch
  paged        pool[page, :, row] = new      -- one index_put_ through precomputed (page, row) slot tensors [B, Nnew]
  fp8          quantize_kv_fp8(new, scale) first, then the same
The baselines know the length on the host; the library entry reads it on the device.  Before the timing the results of the two are
compared byte for byte.  For Nnew >= 1024 a line also gives GB/s over the bytes read plus the bytes written.
The verdict of a pair: the entry is "not slower" when its median is at most the baseline's median plus the baseline's round-to-round
spread (max - min of its rounds).
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
    args = ap.parse_args()

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


if __name__ == "__main__":
    main()
