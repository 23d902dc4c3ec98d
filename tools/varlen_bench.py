#!/usr/bin/env python3
"""Variable-length packed prefill against the two routes the library had before it (profiles/varlen_prefill.txt).  A causal
self-attention prefill of B prompts of different lengths, Hkv K/V heads, G query heads per K/V head, fp16, 16-bit output; each group's
variants timed alternately in one process, so that what else the machine does falls on all of them alike:
  fa_forward_varlen                one launch on the packed (total, H, d) tensors, K/V not expanded; with and without lse
  (a) padded fa_forward_causal     one call on [B, Hq, Lmax, d], every prompt padded to the longest, K/V expanded G times -- the
                                   expansion (repeat_interleave into a fresh tensor) timed alone, the call alone, and both
  (b) looped fa_forward_causal     one call per prompt on [1, Hq, L_b, d] with expanded K/V (the expansion not included)
The copies that pad the prompts, resp. cut them apart, are made before the timing and are NOT counted against (a) and (b).
    python tools/varlen_bench.py [--d 128 64 --Hkv 8 --G 4] [--batches uniform skewed short] [--rounds 7 --iters 10]
One line per variant: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds
(min .. max), the TFLOP/s that makes of the VISIBLE (unmasked) query-key pairs, 4 d flops each, and the ratio of the medians to the
group's first variant with the spread of the per-round ratios.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lengths(name):
    """the three batches: uniform 16 x 2048; one 8192 plus fifteen between 128 and 1024 (seeded); 256 x 64"""
    if name == "uniform":
        return [2048] * 16
    if name == "short":
        return [64] * 256
    import random
    rng = random.Random(3)
    return [8192] + [rng.randrange(128, 1025) for _ in range(15)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--batches", nargs="+", default=["uniform", "skewed", "short"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "varlen_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, G = args.Hkv, args.G
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
        base = times[variants[0][0]]
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            rate = f"{flops / med / 1e6:7.1f} TFLOP/s visible" if "expand K/V" not in name or "+" in name else " " * 23
            print(f"  {name:44s} {med:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  {rate}  "
                  f"ratio to the first {med / statistics.median(base):.3f} (per round {min(ratios):.3f} .. {max(ratios):.3f})")

    for d in args.d:
        for batch in args.batches:
            lens = lengths(batch)
            B, total, Lmax = len(lens), sum(lens), max(lens)
            cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(B)], dtype=torch.int32, device="cuda")
            q = torch.randn(total, Hq, d, device="cuda", dtype=f16)
            k = torch.randn(total, Hkv, d, device="cuda", dtype=f16)
            v = torch.randn(total, Hkv, d, device="cuda", dtype=f16)
            out = torch.empty_like(q)
            lse = torch.empty(Hq, total, device="cuda", dtype=torch.float32)
            visible = sum(n * (n + 1) // 2 for n in lens)
            flops = 4.0 * d * Hq * visible
            # (a): padded to the longest prompt, [B, H, Lmax, d]; K/V with their Hkv heads, expanded inside the timing
            qp = torch.zeros(B, Hq, Lmax, d, device="cuda", dtype=f16)
            kp = torch.zeros(B, Hkv, Lmax, d, device="cuda", dtype=f16)
            vp = torch.zeros(B, Hkv, Lmax, d, device="cuda", dtype=f16)
            s = 0
            for b, n in enumerate(lens):
                qp[b, :, :n], kp[b, :, :n], vp[b, :, :n] = (t[s:s + n].transpose(0, 1) for t in (q, k, v))
                s += n
            expand = lambda: (kp.repeat_interleave(G, dim=1), vp.repeat_interleave(G, dim=1))
            kx, vx = expand()
            op = torch.empty_like(qp)
            padded = lambda: fa.fa_forward(qp, kx, vx, causal=True, out=op)   # fa_forward_causal, AUTO

            def expand_and_padded():
                a, b_ = expand()
                return fa.fa_forward(qp, a, b_, causal=True, out=op)

            # (b): one call per prompt on its own [1, Hq, L, d] tensors, K/V expanded before the timing
            per = []
            s = 0
            for n in lens:
                qs = q[s:s + n].transpose(0, 1).contiguous()[None]
                ks, vs = (t[s:s + n].transpose(0, 1).repeat_interleave(G, dim=0).contiguous()[None] for t in (k, v))
                per.append((qs, ks, vs, torch.empty_like(qs)))
                s += n

            def looped():
                for qs, ks, vs, os_ in per:
                    fa.fa_forward(qs, ks, vs, causal=True, out=os_)

            varlen = lambda: fa.fa_forward_varlen(q, k, v, cu, causal=True, out=out)
            varlen_lse = lambda: fa.fa_forward_varlen(q, k, v, cu, causal=True, out=out, lse=lse)
            # the three routes compute the same thing
            varlen(), padded(), looped()
            torch.cuda.synchronize()
            s, worst_p, worst_l = 0, 0.0, 0.0
            for b, n in enumerate(lens):
                mine = out[s:s + n].transpose(0, 1).float()
                worst_p = max(worst_p, float((mine - op[b, :, :n].float()).abs().max()))
                worst_l = max(worst_l, float((mine - per[b][3][0].float()).abs().max()))
                s += n
            head = (f"{batch}: B{B} lengths {min(lens)}..{Lmax} total {total} Hkv{Hkv} G{G} d{d} fp16 causal, 16-bit out, "
                    f"rounds={args.rounds} iters={args.iters}")
            print(f"    largest |difference| of fa_forward_varlen to the padded call {worst_p:.3e}, to the looped calls {worst_l:.3e}")
            run(head, (("fa_forward_varlen", varlen), ("fa_forward_varlen with lse", varlen_lse),
                       ("(a) expand K/V G times", expand), ("(a) padded fa_forward_causal", padded),
                       ("(a) expand K/V + padded fa_forward_causal", expand_and_padded),
                       ("(b) looped fa_forward_causal", looped)), flops)
            del q, k, v, out, lse, qp, kp, vp, kx, vx, op, per
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
