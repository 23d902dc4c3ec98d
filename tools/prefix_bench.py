#!/usr/bin/env python3
"""What a shared prefix saves and costs on KV-cache decode (profiles/kvcache_prefix.txt).  For B sequences that share a prefix of P
keys and own a suffix of S keys each, on 16-bit and on fp8 caches, each group's variants timed alternately in one process, so that
what else the machine does falls on all of them alike:
  (a) fa_forward_kvcache_shared_prefix against the route without it: fa_forward_kvcache on caches that each hold prefix + suffix
      (B copies of the prefix), eager through the Python front ends and replayed from a captured graph (no host work at all)
  (b) the three launches and the copy of the composed call one by one: the permute of q, the prefix decode with the batch folded
      into rows, the suffix decode, the merge
  (c) the merge kernel against the same rule written in torch ops (max, exp, sum, weighted sum, log; -inf not handled)
  (d) the prefix length swept down to where the plain call wins (16 bit, captured graphs): the crossover
    python tools/prefix_bench.py [--B 8 32 --Hkv 16 --G 4 --P 32768 --S 512 --d 128] [--rounds 7 --iters 20]
One line per variant: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds
(min .. max), the K/V bytes the variant has to read and the rate that makes of the median, and the ratio of the medians to the
group's first variant with the spread of the per-round ratios.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--Hkv", type=int, default=16)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--P", type=int, default=32768)
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--sweep", type=int, nargs="*", default=[256, 512, 1024, 2048, 4096, 8192])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "prefix_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, G, S, d = args.Hkv, args.G, args.S, args.d
    Hq = Hkv * G
    ints = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")

    def cache(b, n, fp8):
        """[b, Hkv, n, d] random K or V, drawn head by head (an fp32 draw of the whole cache would not fit beside it)"""
        out = torch.empty(b, Hkv, n, d, device="cuda", dtype=torch.float8_e4m3fn if fp8 else torch.float16)
        for i in range(b):
            out[i] = torch.randn(Hkv, n, d, device="cuda", dtype=torch.float16).to(out.dtype)
        return out

    def captured(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        return g.replay

    def run(title, variants):
        for _, call, _ in variants:   # warm-up: code objects, the allocator's blocks
            for _ in range(5):
                call()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, call, _ in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        print(title)
        base = times[variants[0][0]]
        for name, _, nbytes in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            rate = f"{nbytes / 2 ** 20:9.1f} MiB K/V {nbytes / med / 1e6:6.2f} TB/s" if nbytes else " " * 32
            print(f"  {name:38s} {med:9.2f} us/call ({min(t):.2f} .. {max(t):.2f})  {rate}  "
                  f"ratio to the first {med / statistics.median(base):.3f} (per round {min(ratios):.3f} .. {max(ratios):.3f})")
        return {name: statistics.median(t) for name, t in times.items()}

    def setup(B, P, fp8):
        """-> the composed call, the plain call, and their K/V bytes"""
        eb = 1 if fp8 else 2
        q = torch.randn(B, Hq, 1, d, device="cuda", dtype=torch.float16)
        kp, vp = cache(1, P, fp8), cache(1, P, fp8)
        ks, vs = cache(B, S, fp8), cache(B, S, fp8)
        kf, vf = cache(B, P + S, fp8), cache(B, P + S, fp8)
        plen, slen, flen = ints([P]), ints([S] * B), ints([P + S] * B)
        shared = lambda: fa.fa_forward_kvcache_shared_prefix(q, kp, vp, ks, vs, prefix_len=plen, cache_seqlens=slen, causal=True)
        plain_fn = fa.fa_forward_kvcache_fp8 if fp8 else fa.fa_forward_kvcache
        plain = lambda: plain_fn(q, kf, vf, cache_seqlens=flen, causal=True)
        kv = 2 * Hkv * d * eb
        return dict(q=q, kp=kp, vp=vp, ks=ks, vs=vs, plen=plen, slen=slen, shared=shared, plain=plain, shared_bytes=kv * (P + B * S),
                    plain_bytes=kv * B * (P + S), fn=plain_fn)

    for fp8 in (False, True):
        for B in args.B:
            kind = "fp8 e4m3 (q fp16)" if fp8 else "fp16"
            head = f"B{B} Hkv{Hkv} G{G} Nq1 d{d} prefix {args.P} suffix {S} {kind} causal rounds={args.rounds} iters={args.iters}"
            x = setup(B, args.P, fp8)
            run(f"(a) {head}: the shared-prefix call against B copies of the prefix",
                (("plain fa_forward_kvcache, eager", x["plain"], x["plain_bytes"]),
                 ("shared prefix, eager", x["shared"], x["shared_bytes"]),
                 ("plain fa_forward_kvcache, graph", captured(x["plain"]), x["plain_bytes"]),
                 ("shared prefix, graph", captured(x["shared"]), x["shared_bytes"])))
            # (b) the pieces of the composed call, each as the front end issues it
            q, fn = x["q"], x["fn"]
            permute = lambda: q.view(B, Hkv, G, 1, d).permute(1, 0, 2, 3, 4).reshape(1, Hkv * B * G, 1, d).contiguous()
            qp = permute()
            pre = lambda: fn(qp, x["kp"], x["vp"], cache_seqlens=x["plen"], out_dtype=torch.float32, return_lse=True)
            suf = lambda: fn(q, x["ks"], x["vs"], cache_seqlens=x["slen"], causal=True, out_dtype=torch.float32, return_lse=True)
            (o_p, l_p), (o_s, l_s) = pre(), suf()
            # the merge through the public front end needs [B,Hq,Nq,d] parts: the prefix part permuted once, outside the timing
            o_pb = o_p.view(Hkv, B, G, 1, d).permute(1, 0, 2, 3, 4).reshape(B, Hq, 1, d).contiguous()
            l_pb = l_p.view(Hkv, B, G, 1).permute(1, 0, 2, 3).reshape(B, Hq, 1).contiguous()
            merge = lambda: fa.fa_merge_states([o_pb, o_s], [l_pb, l_s])
            eb = 1 if fp8 else 2
            run(f"(b) {head}: the pieces of the composed call, captured graphs",
                (("shared prefix, graph", captured(x["shared"]), x["shared_bytes"]),
                 ("permute copy of q", captured(permute), 0),
                 ("prefix decode, batch folded into rows", captured(pre), 2 * Hkv * d * eb * args.P),
                 ("suffix decode", captured(suf), 2 * Hkv * d * eb * B * S),
                 ("fa_merge_states, 2 parts", captured(merge), 0)))

            def torch_rule():
                lses = torch.stack([l_pb, l_s])
                m = lses.max(0).values
                w = torch.exp(lses - m)
                tot = w.sum(0)
                return (w.unsqueeze(-1) * torch.stack([o_pb, o_s])).sum(0) / tot.unsqueeze(-1), m + torch.log(tot)

            got, ref = merge()[0], torch_rule()[0]
            print(f"    merge kernel against the torch ops on the same parts: max |difference| {float((got - ref).abs().max()):.3e}")
            run(f"(c) {head}: the merge of 2 fp32 parts [{B},{Hq},1,{d}], captured graphs",
                (("fa_merge_states", captured(merge), 0), ("the rule in torch ops", captured(torch_rule), 0)))
            del x, o_p, o_s, o_pb, qp
            torch.cuda.empty_cache()

    # (d) the crossover
    print(f"(d) prefix length swept, suffix {S}, fp16, captured graphs: us/call plain | shared | shared / plain")
    for B in args.B:
        for P in sorted(set(args.sweep + [args.P])):
            x = setup(B, P, False)
            sh, pl = captured(x["shared"]), captured(x["plain"])
            ts, tp = [], []
            for _ in range(args.rounds):
                for call, acc in ((pl, tp), (sh, ts)):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.iters):
                        call()
                    t1.record()
                    torch.cuda.synchronize()
                    acc.append(t0.elapsed_time(t1) * 1e3 / args.iters)
            ratios = [a / b for a, b in zip(ts, tp)]
            print(f"  B{B:<3d} prefix {P:6d}: {statistics.median(tp):9.2f} | {statistics.median(ts):9.2f} | "
                  f"{statistics.median(ts) / statistics.median(tp):.3f} (per round {min(ratios):.3f} .. {max(ratios):.3f})")
            del x, sh, pl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
