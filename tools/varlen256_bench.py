#!/usr/bin/env python3
"""What the d = 256 varlen prefill costs, against the route there was and against this library's d = 128 varlen kernel
(profiles/varlen_d256.txt).  Per (dtype, G, shape) the contenders are timed alternately in one process, so that what else the machine
does falls on all alike:
  d256     fa_forward_varlen_d256 (packed) or fa_forward_varlen_kvcache_d256 (cache), causal, out prepared once
  d256'    the same call once more: the ratio d256' / d256 per round is the run's own A/A spread
  torch    (a) the only route before these entries, per sequence: gather the rows (paged: pool[table]), cut them to the window,
           softmax(mask(cap(scale * q K^T))) V as two 16-bit matmuls over the G heads of a group; the mask is made outside the timing
  d128     (b) a yardstick, not a contender: this library's d = 128 varlen entry on the same bytes seen as 2 * Hkv K/V heads and
           2 * Hq query heads of 128 -- the same matrix FLOPs, twice the exponentials
With --fp8 (profiles/varlen_d256_fp8.txt) the cache shapes are timed on an e4m3fn cache instead (quantize_kv_fp8 of the 16-bit
one, per-head scales):
  fp8      fa_forward_varlen_kvcache_d256_fp8 on the codes
  fp8'     the same call once more: the A/A pair
  d256     fa_forward_varlen_kvcache_d256 on the 16-bit cache of the same keys
  widen    the only route before the entry: cache.to(dtype) of K and V, then that call
    python tools/varlen256_bench.py [--G 2 4] [--types f16 bf16] [--shapes packed chunk0 chunk4096 chunk32768 gemma]
                                    [--forms contig paged] [--rounds 5 --iters 3] [--fp8] [--out FILE]
Shapes: Hkv 8, 16 sequences; "packed" is 16 x 2048 self-attention; "chunkP" is a 512-row chunk per sequence over P cached keys, as a
contiguous cache and on pages of 16; "gemma" is chunk32768 with W = 4096 and softcap 50.  One line per contender: the median over the
rounds of the time per call (device events around `iters` calls), the spread of the rounds, and TFLOP/s over the visible (row, key)
pairs, 4 * 256 flop each and query head.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, PAGE, HKV, B = 256, 16, 8, 16
SHAPES = {"packed": (2048, 0, 0, 0.0), "chunk0": (512, 0, 0, 0.0), "chunk4096": (512, 4096, 0, 0.0), "chunk32768": (512, 32768, 0, 0.0),
          "gemma": (512, 32768, 4096, 50.0)}   # (rows per sequence, cached prefix, window, softcap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--types", nargs="+", default=["f16", "bf16"])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fp8", action="store_true", help="the e4m3fn cache section: the cache shapes alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "varlen256_bench needs a GPU"
    torch.manual_seed(0)
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, flops):
        for _, call in variants:   # warm-up: code objects, torch's algorithm choices
            for _ in range(2):
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
        say(title)
        base = times[variants[0][0]]
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            say(f"  {name:6s} {med:11.1f} us/call ({min(t):.1f} .. {max(t):.1f})  x{med / statistics.median(base):.3f} of {variants[0][0]} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f})  {flops / med * 1e-6:7.1f} TFLOP/s")

    say(f"varlen prefill at d = 256{' on an e4m3fn cache' * args.fp8}, Hkv={HKV}, {B} sequences, causal, rounds={args.rounds} iters={args.iters} page={PAGE} ({fa.version()})")
    for typ in args.types:
        tdt = torch.float16 if typ == "f16" else torch.bfloat16
        for shape in args.shapes:
            Lq, P, W, cap = SHAPES[shape]
            L = P + Lq
            cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * Lq
            lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
            # the visible pairs of one sequence and head, and the additive mask of the torch route (rows x keys it keeps)
            i = torch.arange(Lq, device="cuda")[:, None]
            j = torch.arange(L, device="cuda")[None, :]
            seen = (j <= i + P) & ((j > i + P - W) if W else (j >= 0))
            pairs = int(seen.sum())
            first = max(0, P + 1 - W) if W else 0
            mask = torch.zeros((Lq, L - first), device="cuda", dtype=tdt).masked_fill_(~seen[:, first:], float("-inf"))
            if args.fp8 and shape == "packed":
                continue   # there is no packed e4m3fn source
            for form in (["packed"] if shape == "packed" else args.forms):
                k, v = (torch.randn(B, HKV, L, D, device="cuda", dtype=tdt) for _ in range(2))
                # the same bytes as 2 * Hkv heads of 128: every row of 256 is two rows of 128 of two heads
                as128 = lambda x: x.view(*x.shape[:-1], 2, 128).transpose(-2, -3).reshape(x.shape[0], 2 * HKV, x.shape[2], 128)  # noqa: E731
                table = None
                if form == "packed":    # (total, Hkv, D)
                    k, v = (x.transpose(1, 2).reshape(B * L, HKV, D) for x in (k, v))
                    k128, v128 = (x.view(B * L, 2 * HKV, 128) for x in (k, v))
                elif form == "paged":
                    pages = B * L // PAGE
                    table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, L // PAGE)
                    k, v = (x.view(B, HKV, L // PAGE, PAGE, D).transpose(1, 2).reshape(pages, HKV, PAGE, D) for x in (k, v))
                    k128, v128 = as128(k), as128(v)
                else:
                    k128, v128 = as128(k), as128(v)
                if args.fp8:
                    (k8, ks), (v8, vs) = fa.quantize_kv_fp8(k), fa.quantize_kv_fp8(v)
                for G in args.G:
                    Hq = HKV * G
                    q = torch.randn(B * Lq, Hq, D, device="cuda", dtype=tdt)
                    q128 = q.view(B * Lq, 2 * Hq, 128)
                    out, o128 = torch.empty_like(q), torch.empty_like(q128)

                    def d256(q=q, out=out):
                        if form == "packed":
                            return fa.fa_forward_varlen_d256(q, k, v, cu, causal=True, window=W, softcap=cap, out=out)
                        return fa.fa_forward_varlen_kvcache_d256(q, k, v, cu, lens, block_table=table, causal=True, window=W, softcap=cap, out=out)

                    def d128(q128=q128, o128=o128):
                        if form == "packed":
                            return fa.fa_forward_varlen(q128, k128, v128, cu, causal=True, window=W, softcap=cap, out=o128)
                        return fa.fa_forward_varlen_kvcache(q128, k128, v128, cu, lens, block_table=table, causal=True, window=W, softcap=cap,
                                                            out=o128)

                    def torch_route(q=q, G=G):
                        res = []
                        for b in range(B):
                            if form == "packed":
                                kk, vv = (x[b * L:(b + 1) * L].transpose(0, 1) for x in (k, v))
                            elif form == "paged":   # [max_pages] pages -> [Hkv, L, D]
                                kk, vv = (x[table[b].long()].transpose(0, 1).reshape(HKV, L, D) for x in (k, v))
                            else:
                                kk, vv = k[b], v[b]
                            kk, vv = kk[:, first:], vv[:, first:]
                            qq = q[b * Lq:(b + 1) * Lq].view(Lq, HKV, G, D).permute(1, 2, 0, 3)
                            s = torch.matmul(qq, kk[:, None].transpose(-1, -2)) * D ** -0.5
                            if cap:
                                s = cap * torch.tanh(s / cap)
                            res.append(torch.matmul(torch.softmax(s + mask, dim=-1), vv[:, None]))
                        return res

                    def fp8(q=q, out=out):
                        return fa.fa_forward_varlen_kvcache_d256_fp8(q, k8, v8, cu, lens, block_table=table, k_scale=ks, v_scale=vs,
                                                                     causal=True, window=W, softcap=cap, out=out)

                    def widen(q=q, out=out):
                        return fa.fa_forward_varlen_kvcache_d256(q, k8.to(tdt), v8.to(tdt), cu, lens, block_table=table, causal=True,
                                                                 window=W, softcap=cap, out=out)

                    title = f"{typ} {shape} {form} G{G}: {B} x {Lq} rows over {P} cached keys, W={W} softcap={cap}"
                    if args.fp8:
                        run(title, [("fp8", fp8), ("fp8'", fp8), ("d256", d256), ("widen", widen)], 4.0 * D * pairs * B * Hq)
                        continue
                    run(title,
                        [("d256", d256), ("d256'", d256), ("torch", torch_route), ("d128", d128)], 4.0 * D * pairs * B * Hq)
                del k, v, k128, v128
                if args.fp8:
                    del k8, v8
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
