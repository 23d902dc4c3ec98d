#!/usr/bin/env python3
"""Few-query forward over a long K/V (fa_forward_splitkv): time, and GB/s against the bytes K and V
occupy (the path is HBM-bound: every K and V byte is read once).

    python tools/decode_bench.py --B 8 --H 16 --Nq 1 --Nk 32768 --d 128
    python tools/decode_bench.py --kvcache --fill 0.25          # fa_forward_kvcache: a 32768-row cache holding 8192 keys per sequence
    python tools/decode_bench.py --paged 16 --fill 0.25         # fa_forward_kvcache_paged: the same cache in shuffled pages of 16 keys
    python tools/decode_bench.py --kvcache --fp8 [--paged 16]   # the fp8 entry against the 16-bit entry on the same shape
    python tools/decode_bench.py --kvcache --window 4096 [--paged 64] [--fp8]   # a sliding window against two yardsticks

--kvcache times fa_forward_kvcache against a cache of --Nk rows in which every sequence holds --fill x Nk keys (the lengths live
in a device tensor); GB/s then counts the K and V bytes of the keys held, not of the capacity.  --causal adds the mask.
--paged PAGE_SIZE (implies --kvcache) scatters that cache into a pool [B * Nk / PAGE_SIZE, H, PAGE_SIZE, d] through a seeded random
permutation of the pages and times fa_forward_kvcache_paged with the block table of that permutation.
--fp8 (with --kvcache or --paged) quantises the cache with quantize_kv_fp8 and times fa_forward_kvcache[_paged]_fp8 AND the 16-bit
entry on the same shape in the same process, interleaved round by round; each line counts the bytes its cache actually holds, and
the last line gives the ratio of the medians next to the round-to-round spread of the 16-bit timings.
--window W (with --kvcache, --paged or --fp8; --Nq 1) times three calls of ONE entry form (the fp8 one with --fp8, else the 16-bit one;
paged with --paged), interleaved round by round in one process: "window", the windowed entry on the cache; "full", the unwindowed
entry on the same cache; and "short", the unwindowed entry on a cache of capacity W + 64 filled to W keys -- by the split rule the
same keys per sequence, the same split count and the same bytes as "window" when the fill leaves (L - W) a multiple of 64.  The last
lines give window / short next to the spread of the "short" rounds, and window / full.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scatter_pages(torch, k, v, page_size, seed=0):
    """Caches [B, H, Nk, d] -> (K pool, V pool [B * Nk / page_size, H, page_size, d], block table [B, Nk / page_size] int32): logical
    page p of sequence b becomes physical page perm[b * max_pages + p] of a seeded random permutation."""
    B, H, Nk, d = k.shape
    max_pages = Nk // page_size
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(B * max_pages, generator=g).to(k.device)
    pools = []
    for x in (k, v):
        raw = x.view(torch.uint8) if x.element_size() == 1 else x   # an fp8 cache is moved as bytes
        pages = raw.view(B, H, max_pages, page_size, d).permute(0, 2, 1, 3, 4).reshape(B * max_pages, H, page_size, d)
        pool = torch.empty_like(pages)
        pool[perm] = pages
        pools.append(pool.view(x.dtype))
    return pools[0], pools[1], perm.view(B, max_pages).to(torch.int32).contiguous()


def bench_window(args, torch, fa, q, k, v):
    """--window: "window", "full" and "short" of one entry form, alternating inside every round"""
    B, H, Nk, d, W, ps = args.B, args.H, args.Nk, args.d, args.window, args.paged
    held = min(max(int(round(args.fill * Nk)), 0), Nk)
    seen = min(W, held)
    ncap_s = W + 64
    lens, lens_s = (torch.full((B,), n, dtype=torch.int32, device="cuda") for n in (held, seen))
    # the short cache holds the keys the window sees, at its front
    ks_, vs_ = (torch.zeros(B, H, ncap_s, d, dtype=x.dtype, device="cuda") for x in (k, v))
    ks_[:, :, :seen], vs_[:, :, :seen] = k[:, :, held - seen:held], v[:, :, held - seen:held]
    scales = ()
    if args.fp8:
        (k, sk), (v, sv) = fa.quantize_kv_fp8(k), fa.quantize_kv_fp8(v)
        (ks_, _), (vs_, _) = fa.quantize_kv_fp8(ks_, scale=sk), fa.quantize_kv_fp8(vs_, scale=sv)
        scales = (sk, sv)
    if ps:
        k, v, table = scatter_pages(torch, k, v, ps, seed=0)
        ks_, vs_, table_s = scatter_pages(torch, ks_, vs_, ps, seed=1)
        entry = fa.fa_forward_kvcache_paged_fp8 if args.fp8 else fa.fa_forward_kvcache_paged
        need = {"window": fa.kvcache_paged_window_workspace_bytes(B, H, 1, 1, Nk // ps, ps, d, W),
                "full": fa.kvcache_paged_workspace_bytes(B, H, 1, 1, Nk // ps, ps, d),
                "short": fa.kvcache_paged_workspace_bytes(B, H, 1, 1, ncap_s // ps, ps, d)}
        big, small = (k, v, table), (ks_, vs_, table_s)
    else:
        entry = fa.fa_forward_kvcache_fp8 if args.fp8 else fa.fa_forward_kvcache
        need = {"window": fa.kvcache_window_workspace_bytes(B, H, 1, 1, Nk, d, W), "full": fa.kvcache_workspace_bytes(B, H, 1, 1, Nk, d),
                "short": fa.kvcache_workspace_bytes(B, H, 1, 1, ncap_s, d)}
        big, small = (k, v), (ks_, vs_)
    ws = torch.empty(max(max(need.values()), 1), dtype=torch.uint8, device="cuda")
    calls = {"window": lambda: entry(q, *big, *scales, lens, causal=args.causal, workspace=ws, window=W),
             "full": lambda: entry(q, *big, *scales, lens, causal=args.causal, workspace=ws),
             "short": lambda: entry(q, *small, *scales, lens_s, causal=args.causal, workspace=ws)}
    got = {name: fn().float() for name, fn in calls.items()}
    torch.cuda.synchronize()
    same = torch.equal(got["window"], got["short"]) if (held - seen) % 64 == 0 else None
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    elem = 1 if args.fp8 else 2
    form = ("fp8" if args.fp8 else "16-bit") + (f" paged {ps}" if ps else "") + (" causal" if args.causal else "")
    med = {}
    for name in calls:
        med[name] = statistics.median(times[name])
        keys = held if name == "full" else seen
        kv_bytes = 2.0 * B * H * keys * d * elem
        print(f"B{B} H{H} Nq1 Nk{Nk} d{d} {form} window {W}, {held} keys held [{name}]: workspace {need[name]} B, median "
              f"{med[name] * 1e3:.1f} us (rounds {min(times[name]) * 1e3:.1f}-{max(times[name]) * 1e3:.1f}), K+V {kv_bytes / 1e6:.1f} MB -> "
              f"{kv_bytes / med[name] / 1e6:.0f} GB/s")
    spread = (max(times["short"]) - min(times["short"])) / med["short"]
    ratio = med["window"] / med["short"]
    print(f"window / short = {ratio:.3f}; the short rounds spread over {spread * 100:.1f} %: bound 1 + spread + 5 % = {1 + spread + 0.05:.3f} "
          f"-> {'within' if ratio <= 1 + spread + 0.05 else 'MISSED'}" + ("" if same is None else f"; results bit-equal: {same}"))
    print(f"window / full = {med['window'] / med['full']:.3f} (keys seen / keys held = {seen / max(held, 1):.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--Nq", type=int, default=1)
    ap.add_argument("--Nk", type=int, default=32768)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kvcache", action="store_true", help="fa_forward_kvcache with per-sequence lengths instead of fa_forward_splitkv")
    ap.add_argument("--fill", type=float, default=1.0, help="with --kvcache: every sequence holds FILL * Nk keys")
    ap.add_argument("--causal", action="store_true", help="with --kvcache: the causal mask aligned to the end of the cache")
    ap.add_argument("--paged", type=int, default=0, metavar="PAGE_SIZE",
                    help="fa_forward_kvcache_paged on the cache scattered into shuffled pages of PAGE_SIZE keys (implies --kvcache)")
    ap.add_argument("--fp8", action="store_true",
                    help="with --kvcache / --paged: also time the fp8 entry on the quantised cache, interleaved with the 16-bit one")
    ap.add_argument("--window", type=int, default=0, metavar="W",
                    help="with --kvcache / --paged / --fp8: time the windowed entry against the unwindowed one and a cache of W + 64 rows")
    args = ap.parse_args()
    if args.paged:
        args.kvcache = True
        if args.paged < 16 or args.paged & (args.paged - 1) or args.Nk % args.paged:
            ap.error("--paged needs a power of two >= 16 that divides --Nk")
    import torch
    import flashattention_kernel_project_amd as fa
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(args.B, args.H, args.Nq, args.d, generator=g, device="cuda").half()
    k, v = (torch.randn(args.B, args.H, args.Nk, args.d, generator=g, device="cuda").half() for _ in range(2))
    if not args.kvcache and (args.fill != 1.0 or args.causal or args.fp8):
        ap.error("--fill, --causal and --fp8 need --kvcache")
    if args.window and (not args.kvcache or args.window < 1 or args.Nq != 1 or (args.window + 64) % max(args.paged, 1)):
        ap.error("--window needs --kvcache or --paged, W >= 1, --Nq 1 and, with --paged, a page size that divides W + 64")
    if args.window:
        return bench_window(args, torch, fa, q, k, v)
    calls = {}   # name -> (call, bytes per K/V element)
    if args.kvcache:
        held = min(max(int(round(args.fill * args.Nk)), 0), args.Nk)
        lens = torch.full((args.B,), held, dtype=torch.int32, device="cuda")
        need = fa.kvcache_workspace_bytes(args.B, args.H, 1, args.Nq, args.Nk, args.d)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")

        if args.fp8:
            (k8, ks), (v8, vs) = fa.quantize_kv_fp8(k), fa.quantize_kv_fp8(v)
            if args.paged:
                k8, v8, _ = scatter_pages(torch, k8, v8, args.paged, seed=0)   # the same permutation as the 16-bit pools below
        if args.paged:
            k, v, table = scatter_pages(torch, k, v, args.paged, seed=0)
            need = fa.kvcache_paged_workspace_bytes(args.B, args.H, 1, args.Nq, args.Nk // args.paged, args.paged, args.d)

            def call():
                fa.fa_forward_kvcache_paged(q, k, v, table, lens, causal=args.causal, workspace=ws)

            def call8():
                fa.fa_forward_kvcache_paged_fp8(q, k8, v8, table, ks, vs, lens, causal=args.causal, workspace=ws)
        else:
            def call():
                fa.fa_forward_kvcache(q, k, v, lens, causal=args.causal, workspace=ws)

            def call8():
                fa.fa_forward_kvcache_fp8(q, k8, v8, ks, vs, lens, causal=args.causal, workspace=ws)
    else:
        held = args.Nk
        need = fa.splitkv_workspace_bytes(args.B, args.H, args.Nq, args.Nk, args.d)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")

        def call():
            fa.fa_forward_splitkv(q, k, v, workspace=ws)
    calls["16-bit"] = (call, 2)
    if args.fp8:
        calls["fp8"] = (call8, 1)
    for fn, _ in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(args.rounds):   # the entries alternate inside every round: drift hits both alike
        for name, (fn, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    tag = f" kvcache fill {args.fill:g} ({held} keys){' causal' if args.causal else ''}" if args.kvcache else ""
    if args.paged:
        tag += f" paged {args.paged}"
    med = {}
    for name, (_, elem) in calls.items():
        med[name] = statistics.median(times[name])
        kv_bytes = 2.0 * args.B * args.H * held * args.d * elem
        which = f" [{name}]" if args.fp8 else ""
        print(f"B{args.B} H{args.H} Nq{args.Nq} Nk{args.Nk} d{args.d}{tag}{which}: workspace {need} B, median {med[name] * 1e3:.1f} us "
              f"(rounds {min(times[name]) * 1e3:.1f}-{max(times[name]) * 1e3:.1f}), "
              f"K+V {kv_bytes / 1e6:.1f} MB -> {kv_bytes / med[name] / 1e6:.0f} GB/s ({kv_bytes / med[name] / 1e6 / 8000 * 100:.1f} % of 8 TB/s)")
    if args.fp8:
        spread = max(times["16-bit"]) - min(times["16-bit"])
        gain = med["16-bit"] - med["fp8"]
        print(f"fp8 / 16-bit = {med['fp8'] / med['16-bit']:.3f} (ideal 0.5); fp8 is {gain * 1e3:.1f} us faster, the 16-bit rounds spread "
              f"over {spread * 1e3:.1f} us: {'faster beyond the spread' if gain > spread else 'NOT faster beyond the spread'}")

if __name__ == "__main__":
    main()
