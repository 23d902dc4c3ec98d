#!/usr/bin/env python3
"""The varlen prefill against an fp8 KV cache (fa_forward_varlen_kvcache_fp8) next to the kernel it derives from and the only route an
fp8 cache had before it (profiles/varlen_cache_fp8.txt).  B sequences each feed a chunk of Lq query rows that attends, causally, to a
cached prefix of P keys plus the chunk itself (Lk = P + Lq); Hkv K/V heads, G query heads per K/V head, fp16 queries, 16-bit output.
For the contiguous cache and for page pools behind a shuffled block table, three variants, timed alternately in one process so that
what else the machine does falls on all of them alike:
  (8)  fa_forward_varlen_kvcache_fp8    on the e4m3fn cache, with k_scale and v_scale vectors (of ones, so that the bits can be compared)
  (16) fa_forward_varlen_kvcache        on a 16-bit cache that holds the same keys (the widened codes): the kernel (8) derives from
  (w)  cache.to(fp16) + (16)            the whole fp8 cache, or both pools, widened by torch before the call: the route without the entry
    python tools/varlen_cache_fp8_bench.py [--groups chunk512 one2048] [--d 128 64] [--pages 16] [--rounds 7 --iters 20]
One line per variant: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds
(min .. max), the TFLOP/s that makes of the VISIBLE (unmasked) query-key pairs, 4 d flops each, and the ratios of the medians to (16)
and to (w) of the same layout.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = {   # name: [(B, Lq, prefix)]
    "chunk512": [(16, 512, 0), (16, 512, 4096), (16, 512, 32768)],
    "one2048": [(1, 2048, 8192)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", nargs="+", default=["chunk512", "one2048"])
    ap.add_argument("--d", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--pages", type=int, nargs="+", default=[16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "varlen_cache_fp8_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, G = args.Hkv, args.G
    Hq = Hkv * G
    f16, e4 = torch.float16, torch.float8_e4m3fn

    def run(title, variants, flops):
        for _, _, call in variants:   # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, _, call in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        print(title)
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, layout, _ in variants:
            t = times[name]
            m16 = med[f"(16) fa_forward_varlen_kvcache, {layout}"]
            mw = med[f"(w) cache.to(fp16) + (16), {layout}"]
            print(f"  {name:52s} {med[name]:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  {flops / med[name] / 1e6:7.1f} TFLOP/s visible"
                  f"  to (16) {med[name] / m16:.3f}  to (w) {med[name] / mw:.3f}")

    for d in args.d:
        for group in args.groups:
            for B, Lq, P in GROUPS[group]:
                Lk = P + Lq
                total_q = B * Lq
                q = torch.randn(total_q, Hq, d, device="cuda", dtype=f16)
                k8 = torch.randn(B, Hkv, Lk, d, device="cuda", dtype=f16).to(e4)    # the contiguous fp8 cache, Ncap = Lk
                v8 = torch.randn(B, Hkv, Lk, d, device="cuda", dtype=f16).to(e4)
                k16, v16 = k8.to(f16), v8.to(f16)                                      # the same keys in a 16-bit cache
                ones = torch.ones(Hkv, device="cuda")
                cu_q = torch.arange(0, total_q + 1, Lq, dtype=torch.int32, device="cuda")
                lens = torch.full((B,), Lk, dtype=torch.int32, device="cuda")
                out = torch.empty_like(q)
                flops = 4.0 * d * Hq * B * sum(P + i + 1 for i in range(Lq))
                layouts = {"contiguous": (k8, v8, k16, v16, None)}
                for ps in args.pages:
                    assert Lk % ps == 0, "the groups keep Lk a multiple of the page sizes"
                    mp = Lk // ps
                    perm = torch.randperm(B * mp, device="cuda")
                    pools = []
                    for cache in (k8, v8):
                        pool = torch.empty(B * mp, Hkv, ps, d, device="cuda", dtype=e4)
                        pool[perm] = cache.reshape(B, Hkv, mp, ps, d).permute(0, 2, 1, 3, 4).reshape(B * mp, Hkv, ps, d)
                        pools.append(pool)
                    layouts[f"pages of {ps}"] = (pools[0], pools[1], pools[0].to(f16), pools[1].to(f16), perm.reshape(B, mp).to(torch.int32))
                variants = []
                for layout, (a8, b8, a16, b16, table) in layouts.items():
                    kw = dict(block_table=table, causal=True, out=out)
                    variants += [
                        (f"(8) fa_forward_varlen_kvcache_fp8, {layout}", layout,
                         lambda a8=a8, b8=b8, kw=kw: fa.fa_forward_varlen_kvcache_fp8(q, a8, b8, cu_q, lens, k_scale=ones, v_scale=ones, **kw)),
                        (f"(16) fa_forward_varlen_kvcache, {layout}", layout,
                         lambda a16=a16, b16=b16, kw=kw: fa.fa_forward_varlen_kvcache(q, a16, b16, cu_q, lens, **kw)),
                        (f"(w) cache.to(fp16) + (16), {layout}", layout,
                         lambda a8=a8, b8=b8, kw=kw: fa.fa_forward_varlen_kvcache(q, a8.to(f16), b8.to(f16), cu_q, lens, **kw))]
                # the routes compute the same thing, bit for bit: the widening is exact and the scales are ones
                ref = None
                for name, _, call in variants:
                    out.zero_()
                    call()
                    torch.cuda.synchronize()
                    ref = out.clone() if ref is None else ref
                    assert torch.equal(out, ref), name
                print("    all variants return the same bits")
                head = (f"{group}: B{B} x {Lq} rows over a prefix of {P} keys (Lk {Lk}) Hkv{Hkv} G{G} d{d} fp16 causal, 16-bit out, "
                        f"rounds={args.rounds} iters={args.iters}")
                run(head, variants, flops)
                del q, k8, v8, k16, v16, out, ref, layouts, variants
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
