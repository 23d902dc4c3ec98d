#!/usr/bin/env python3
"""What attention sinks and a soft-cap cost on KV-cache decode (profiles/kvcache_logits.txt): the four variants of one call --
(a) neither option (the existing kernels), (b) sinks, (c) soft-cap, (d) both -- timed alternately in one process, so that what
else the machine does falls on all of them alike.
    python tools/logits_bench.py [--B 8 --Hkv 16 --G 1 --Nq 1 --Nk 32768 --d 128] [--window W] [--fp8] [--rounds 7 --iters 40]
One line per variant: the median over the rounds of the time per call (device events around `iters` calls), the spread of the
rounds (min .. max), and the ratio of the medians to (a) with the spread of the per-round ratios.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--Hkv", type=int, default=16)
    ap.add_argument("--G", type=int, default=1)
    ap.add_argument("--Nq", type=int, default=1)
    ap.add_argument("--Nk", type=int, default=32768)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--softcap", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "logits_bench needs a GPU"
    torch.manual_seed(0)
    B, Hkv, G, Nq, Nk, d = args.B, args.Hkv, args.G, args.Nq, args.Nk, args.d
    q = torch.randn(B, Hkv * G, Nq, d, device="cuda", dtype=torch.float16)
    k = torch.randn(B, Hkv, Nk, d, device="cuda", dtype=torch.float16)
    v = torch.randn(B, Hkv, Nk, d, device="cuda", dtype=torch.float16)
    lens = torch.full((B,), Nk, dtype=torch.int32, device="cuda")
    sinks = torch.linspace(0.0, 4.0, Hkv * G, device="cuda", dtype=torch.float32)
    need = fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Nk, d, args.window)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    kw = dict(cache_seqlens=lens, causal=True, workspace=ws, window=args.window)
    if args.fp8:
        k8, ks = fa.quantize_kv_fp8(k)
        v8, vs = fa.quantize_kv_fp8(v)
        call = lambda **o: fa.fa_forward_kvcache_fp8(q, k8, v8, ks, vs, **kw, **o)
    else:
        call = lambda **o: fa.fa_forward_kvcache(q, k, v, **kw, **o)
    variants = (("a neither", {}), ("b sinks", dict(sinks=sinks)), ("c softcap", dict(softcap=args.softcap)),
                ("d both", dict(sinks=sinks, softcap=args.softcap)))
    for _, o in variants:   # warm-up: code objects, the LDS attribute
        for _ in range(5):
            call(**o)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, o in variants:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                call(**o)
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
    kv_bytes = 2 * B * Hkv * (min(args.window + Nq - 1, Nk) if args.window else Nk) * d * (1 if args.fp8 else 2)
    print(f"B{B} Hkv{Hkv} G{G} Nq{Nq} Nk{Nk} d{d} window={args.window} {'fp8' if args.fp8 else 'fp16'} softcap={args.softcap} "
          f"S={need // max(B * Hkv * G * Nq * (d + 2) * 4, 1) or 1} rounds={args.rounds} iters={args.iters}")
    base = times["a neither"]
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        ratios = [x / y for x, y in zip(t, base)]
        print(f"  {name:10s} {med:8.2f} us/call ({min(t):.2f} .. {max(t):.2f})  {kv_bytes / med / 1e6:6.2f} TB/s of K/V  "
              f"ratio to (a) {med / statistics.median(base):.3f} (per round {min(ratios):.3f} .. {max(ratios):.3f})")


if __name__ == "__main__":
    main()
