#!/usr/bin/env python3
"""What fa_kvcache_decode_d256 costs, against the route there was and against this library's d = 128 stream (profiles/kv256_decode.txt).
Per (dtype, cache form, Hkv, G, B, L, options) the contenders are timed alternately in one process, so that what else the machine does
falls on all alike:
  d256     fa_kvcache_decode_d256, one token per sequence, causal, the library's split count (out and workspace prepared once)
  d256'    the same call once more: the ratio d256' / d256 per round is the run's own A/A spread
  torch    (a) the only route before this entry: gather the sequences' rows (paged: pool[table]; contiguous: the cache as it lies),
           cut them to the window, then softmax(cap(scale * q K^T)) V as two 16-bit matmuls over the G heads of a group
  d128     (b) a yardstick for the STREAM only, not a contender: fa_kvcache_decode_varlen, d = 128, on the same cache bytes seen as
           2 * Hkv heads of 128 (the same options), one token per sequence
    python tools/kv256_bench.py [--Hkv 8 4] [--G 2 4 8] [--B 8 64] [--L 4096 32768] [--types f16 bf16] [--forms contig paged]
                                [--opts plain gemma] [--rounds 5 --iters 10] [--out FILE]
One line per contender: the median over the rounds of the time per call (device events around `iters` calls) and the spread of the
rounds, and the K/V rate 2 * B * Hkv * keys * 512 B / t computed from the shape, `keys` being L, or min(L, W) under the window.
"gemma" is W = 4096 with softcap 50.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, PAGE = 256, 16
OPTS = {"plain": (0, 0.0), "gemma": (4096, 50.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Hkv", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--G", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--B", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--L", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--types", nargs="+", default=["f16", "bf16"])
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--opts", nargs="+", default=["plain", "gemma"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "kv256_bench needs a GPU"
    torch.manual_seed(0)
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, nbytes):
        for _, call in variants:   # warm-up: code objects, torch's algorithm choices
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
        say(title)
        base = times[variants[0][0]]
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            say(f"  {name:6s} {med:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  x{med / statistics.median(base):.3f} of {variants[0][0]} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f})  {nbytes / med * 1e-6:6.2f} TB/s of K+V")

    say(f"fa_kvcache_decode_d256, one token per sequence, causal, rounds={args.rounds} iters={args.iters} page={PAGE} ({fa.version()})")
    for typ in args.types:
        tdt = torch.float16 if typ == "f16" else torch.bfloat16
        for form in args.forms:
            for Hkv in args.Hkv:
                for B in args.B:
                    for L in args.L:
                        # one cache per (type, form, Hkv, B, L); the G and option loops reuse it
                        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
                        cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
                        k, v = (torch.randn(B, Hkv, L, D, device="cuda", dtype=tdt) for _ in range(2))
                        table, geo = None, dict(Ncap=L)
                        if form == "paged":
                            pages = B * L // PAGE
                            table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, L // PAGE)
                            k, v = (x.view(B, Hkv, L // PAGE, PAGE, D).transpose(1, 2).reshape(pages, Hkv, PAGE, D) for x in (k, v))
                            geo = dict(max_pages=L // PAGE, page_size=PAGE)
                        # the same bytes as 2 * Hkv heads of 128: every row of 256 is two rows of 128 of two heads
                        k128, v128 = (x.view(*x.shape[:-1], 2, 128).transpose(-2, -3).reshape(x.shape[0], 2 * Hkv, x.shape[2], 128)
                                      for x in (k, v))
                        for G in args.G:
                            Hq = Hkv * G
                            q = torch.randn(B, Hq, D, device="cuda", dtype=tdt)
                            q128 = torch.randn(B, 2 * Hq, 128, device="cuda", dtype=tdt)
                            out, o128 = torch.empty_like(q), torch.empty_like(q128)
                            for opt in args.opts:
                                W, cap = OPTS[opt]
                                ws = torch.empty(max(fa.kvcache_decode_d256_workspace_bytes(B, Hkv, G, 1, window=W, **geo), 1),
                                                 dtype=torch.uint8, device="cuda")
                                ws128 = torch.empty(max(fa.kvcache_decode_varlen_workspace_bytes(B, 2 * Hkv, G, 1, 128, window=W, **geo), 1),
                                                    dtype=torch.uint8, device="cuda")

                                def d256(q=q, out=out, ws=ws, W=W, cap=cap):
                                    return fa.fa_kvcache_decode_d256(q, k, v, cu, 1, cache_seqlens=lens, block_table=table, causal=True, window=W,
                                                                     softcap=cap, out=out, workspace=ws)

                                def d128(q128=q128, o128=o128, ws128=ws128, W=W, cap=cap):
                                    return fa.fa_kvcache_decode_varlen(q128, k128, v128, cu, 1, cache_seqlens=lens, block_table=table, causal=True,
                                                                       window=W, softcap=cap, out=o128, workspace=ws128)

                                def torch_route(q=q, G=G, W=W, cap=cap):
                                    kk, vv = k, v
                                    if table is not None:   # [B, max_pages] pages -> [B, Hkv, L, D]
                                        kk, vv = (x[table.view(-1).long()].view(B, L // PAGE, Hkv, PAGE, D).transpose(1, 2).reshape(B, Hkv, L, D)
                                                  for x in (k, v))
                                    if W and W < L:
                                        kk, vv = kk[:, :, L - W:], vv[:, :, L - W:]
                                    s = torch.matmul(q.view(B, Hkv, G, D), kk.transpose(-1, -2)) * D ** -0.5
                                    if cap:
                                        s = cap * torch.tanh(s / cap)
                                    return torch.matmul(torch.softmax(s, dim=-1), vv)

                                keys = min(L, W) if W else L
                                run(f"{typ} {form} Hkv{Hkv} G{G} B{B} L{L} {opt} (workspace {ws.numel()} B)",
                                    [("d256", d256), ("d256'", d256), ("torch", torch_route), ("d128", d128)], 2.0 * B * Hkv * keys * D * 2)
                        del k, v, k128, v128
                        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
