#!/usr/bin/env python3
"""The varlen prefill against the KV cache (fa_forward_varlen_kvcache) next to the routes the library had before it
(profiles/varlen_cache.txt).  B sequences each feed a chunk of Lq query rows that attends, causally, to a cached prefix of P keys plus
the chunk itself (Lk = P + Lq); Hkv K/V heads, G query heads per K/V head, fp16, 16-bit output.  Each group's variants are timed
alternately in one process, so that what else the machine does falls on all of them alike:
  (a) fa_forward_varlen, packed        the same keys already packed (total_k, Hkv, d): the kernel alone
  fa_forward_varlen_kvcache            on the contiguous cache [B,Hkv,Ncap,d], and on page pools with pages of 16 and of 128 keys behind a
                                       shuffled block table
  (b) gather + fa_forward_varlen       the pages of every sequence gathered into a packed copy by index_select (one pass: the pool
                                       viewed [num_pages, page, Hkv, d]), K and V, then (a): the only route without the entry
  (c) fa_forward_kvcache_paged         the ragged paged decode entry with seqlens_q on q [B,Hq,Lq,d]: a split-KV streaming kernel
    python tools/varlen_cache_bench.py [--groups chunk512 one2048 tiny16 crossover] [--rounds 7 --iters 10]
One line per variant: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds
(min .. max), the TFLOP/s that makes of the VISIBLE (unmasked) query-key pairs, 4 d flops each, and the ratios of the medians to (a)
and to (b).  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = {   # name: [(B, Lq, prefix)]
    "chunk512": [(16, 512, 0), (16, 512, 4096), (16, 512, 32768)],
    "one2048": [(1, 2048, 8192)],
    "tiny16": [(8, 16, 32768 - 16)],                                 # 32768 keys, the chunk included: whole pages of 128
    "crossover": [(8, n, 32768 - n) for n in (32, 64, 128, 256)],    # with tiny16 and chunk512: where (c) stops winning
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", nargs="+", default=["chunk512", "one2048", "tiny16", "crossover"])
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--pages", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "varlen_cache_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, G, d = args.Hkv, args.G, args.d
    Hq = Hkv * G
    f16 = torch.float16

    def run(title, variants, flops):
        for _, call in variants:   # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, call in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        print(title)
        med = {name: statistics.median(t) for name, t in times.items()}
        a = med[variants[0][0]]
        b = next((m for name, m in med.items() if name.startswith("(b)")), float("nan"))
        for name, _ in variants:
            t = times[name]
            print(f"  {name:46s} {med[name]:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  {flops / med[name] / 1e6:7.1f} TFLOP/s visible"
                  f"  to (a) {med[name] / a:.3f}  to (b) {med[name] / b:.3f}")

    for group in args.groups:
        for B, Lq, P in GROUPS[group]:
            Lk = P + Lq
            total_q, total_k = B * Lq, B * Lk
            q = torch.randn(total_q, Hq, d, device="cuda", dtype=f16)
            kc = torch.randn(B, Hkv, Lk, d, device="cuda", dtype=f16)            # the contiguous cache, Ncap = Lk
            vc = torch.randn(B, Hkv, Lk, d, device="cuda", dtype=f16)
            k = kc.permute(0, 2, 1, 3).reshape(total_k, Hkv, d).contiguous()       # (a): the same keys packed
            v = vc.permute(0, 2, 1, 3).reshape(total_k, Hkv, d).contiguous()
            cu_q = torch.arange(0, total_q + 1, Lq, dtype=torch.int32, device="cuda")
            cu_k = torch.arange(0, total_k + 1, Lk, dtype=torch.int32, device="cuda")
            lens = torch.full((B,), Lk, dtype=torch.int32, device="cuda")
            out = torch.empty_like(q)
            flops = 4.0 * d * Hq * B * sum(P + i + 1 for i in range(Lq))
            packed = lambda: fa.fa_forward_varlen(q, k, v, cu_q, cu_k, causal=True, out=out)
            variants = [("(a) fa_forward_varlen, packed", packed),
                        ("fa_forward_varlen_kvcache, contiguous", lambda: fa.fa_forward_varlen_kvcache(q, kc, vc, cu_q, lens, causal=True, out=out))]
            packed()
            ref = out.clone()
            pools = {}
            for ps in args.pages:
                assert Lk % ps == 0, "the groups keep Lk a multiple of the page sizes, so that (b) is one gather"
                mp = Lk // ps
                perm = torch.randperm(B * mp, device="cuda")
                table = perm.reshape(B, mp).to(torch.int32)
                kp = torch.empty(B * mp, Hkv, ps, d, device="cuda", dtype=f16)
                vp = torch.empty_like(kp)
                kp[perm] = kc.reshape(B, Hkv, mp, ps, d).permute(0, 2, 1, 3, 4).reshape(B * mp, Hkv, ps, d)
                vp[perm] = vc.reshape(B, Hkv, mp, ps, d).permute(0, 2, 1, 3, 4).reshape(B * mp, Hkv, ps, d)
                pools[ps] = (kp, vp, table, table.reshape(-1).long())
                variants.append((f"fa_forward_varlen_kvcache, pages of {ps}",
                                 lambda ps=ps: fa.fa_forward_varlen_kvcache(q, pools[ps][0], pools[ps][1], cu_q, lens,
                                                                            block_table=pools[ps][2], causal=True, out=out)))

            def gathered(ps):
                kp, vp, _, idx = pools[ps]
                kg = kp.permute(0, 2, 1, 3).index_select(0, idx).reshape(total_k, Hkv, d)
                vg = vp.permute(0, 2, 1, 3).index_select(0, idx).reshape(total_k, Hkv, d)
                return fa.fa_forward_varlen(q, kg, vg, cu_q, cu_k, causal=True, out=out)

            ps_b = max(args.pages)
            variants.append((f"(b) gather pages of {ps_b} + fa_forward_varlen", lambda: gathered(ps_b)))
            # (c): the ragged decode entry on q [B,Hq,Lq,d]; its own output buffer
            qd = q.reshape(B, Lq, Hq, d).permute(0, 2, 1, 3).contiguous()
            nq = torch.full((B,), Lq, dtype=torch.int32, device="cuda")
            decode = lambda: fa.fa_forward_kvcache_paged(qd, pools[ps_b][0], pools[ps_b][1], pools[ps_b][2], lens, causal=True,
                                                         out_dtype=f16, seqlens_q=nq)
            try:
                od = decode()
                torch.cuda.synchronize()
                worst_c = float((od.permute(0, 2, 1, 3).reshape(total_q, Hq, d).float() - ref.float()).abs().max())
                variants.append((f"(c) fa_forward_kvcache_paged seqlens_q, pages of {ps_b}", decode))
            except (ValueError, fa.FaError) as e:
                worst_c = float("nan")
                print(f"    (c) refused at this shape: {e}")
            # the routes compute the same thing: the cache forms bit for bit
            worst = 0.0
            for name, call in variants[1:2 + len(args.pages)]:
                out.zero_()
                call()
                torch.cuda.synchronize()
                assert torch.equal(out, ref), name
            gathered(ps_b)
            torch.cuda.synchronize()
            worst = float((out.float() - ref.float()).abs().max())
            print(f"    the cache forms return (a)'s bits; largest |difference| of (b) to (a) {worst:.3e}, of (c) to (a) {worst_c:.3e}")
            head = (f"{group}: B{B} x {Lq} rows over a prefix of {P} keys (Lk {Lk}) Hkv{Hkv} G{G} d{d} fp16 causal, 16-bit out, "
                    f"rounds={args.rounds} iters={args.iters}")
            run(head, variants, flops)
            del q, kc, vc, k, v, out, ref, pools, qd
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
