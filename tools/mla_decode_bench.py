#!/usr/bin/env python3
"""What fa_mla_decode costs, against the route there was and against this library's own key stream (profiles/mla_decode.txt).
Per (dtype, cache form, Hq, B, L) the contenders are timed alternately in one process, so that what else the machine does falls on
all alike:
  mla      fa_mla_decode, one token per sequence, the library's split count (out and workspace prepared once)
  mla'     the same call once more: the ratio mla' / mla per round is the run's own A/A spread
  torch    the only route before this entry: gather the sequences' rows (paged: pool[table]; contiguous: the cache as it lies), then
           softmax(scale * q C^T) C[:, :, :512] as two 16-bit torch.bmm with a softmax between them
  d128     a yardstick for the STREAM only, not a contender: fa_kvcache_decode_varlen, d = 128, on a cache of the same byte count
           (Hkv = 9 heads of L / 4 keys: 9 * 512 B * L / 4 = 1152 B * L per sequence), G = 2, one token per sequence
    python tools/mla_decode_bench.py [--Hq 16 128] [--B 8 64] [--L 4096 32768] [--types f16 bf16] [--forms contig paged]
                                     [--sweep] [--rounds 5 --iters 10] [--out FILE]
One line per contender: the median over the rounds of the time per call (device events around `iters` calls) and the spread of the
rounds; for the MLA calls the cache rate B * L * 1152 B / t and the arithmetic rate 2 * B * Hq * L * (576 + 512) / t, both computed
from the shape.  --sweep adds forced split counts at L = 32768, B = 8.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DQK, DC, PAGE = 576, 512, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Hq", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--B", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--L", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--types", nargs="+", default=["f16", "bf16"])
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "mla_decode_bench needs a GPU"
    torch.manual_seed(0)
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, rates):
        """variants: (name, call); rates(name, us) -> a suffix for the line"""
        for _, call in variants:   # warm-up: code objects, the LDS attribute, torch's algorithm choices
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
            say(f"  {name:8s} {med:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  x{med / statistics.median(base):.3f} of {variants[0][0]} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f}){rates(name, med)}")

    say(f"fa_mla_decode, one token per sequence, causal, rounds={args.rounds} iters={args.iters} page={PAGE} ({fa.version()})")
    for typ in args.types:
        tdt = torch.float16 if typ == "f16" else torch.bfloat16
        for form in args.forms:
            for Hq in args.Hq:
                for B in args.B:
                    for L in args.L:
                        cap = L
                        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
                        cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
                        q = torch.randn(B, Hq, DQK, device="cuda", dtype=tdt)
                        cache = torch.randn(B, cap, DQK, device="cuda", dtype=tdt)
                        table = None
                        if form == "paged":
                            pages = B * cap // PAGE
                            table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, cap // PAGE)
                            cache = cache.view(pages, PAGE, DQK)
                            geo = dict(max_pages=cap // PAGE, page_size=PAGE)
                        else:
                            geo = dict(Ncap=cap)
                        out = torch.empty(B, Hq, DC, device="cuda", dtype=tdt)
                        scale = DQK ** -0.5

                        def mla(S=0, q=q, cache=cache, cu=cu, lens=lens, table=table, out=out, geo=geo, B=B, Hq=Hq):
                            need = fa.mla_decode_workspace_bytes(B, Hq, 1, num_splits=S, **geo)
                            ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
                            return lambda: fa.fa_mla_decode(q, cache, cu, 1, cache_seqlens=lens, block_table=table, causal=True, num_splits=S,
                                                            out=out, workspace=ws)

                        def torch_route(q=q, cache=cache, table=table, B=B, cap=cap, L=L):
                            c = cache[table.view(-1).long()].view(B, cap, DQK) if table is not None else cache
                            c = c[:, :L]
                            p = torch.softmax(torch.bmm(q, c.transpose(1, 2)) * scale, dim=-1)
                            return torch.bmm(p, c[:, :, :DC])

                        # the d = 128 stream on the same number of cache bytes
                        Hkv, G, Nk = 9, 2, L // 4
                        q128 = torch.randn(B, Hkv * G, 128, device="cuda", dtype=tdt)
                        k128, v128 = (torch.randn(B, Hkv, Nk, 128, device="cuda", dtype=tdt) for _ in range(2))
                        l128 = torch.full((B,), Nk, dtype=torch.int32, device="cuda")
                        o128 = torch.empty(B, Hkv * G, 128, device="cuda", dtype=tdt)
                        ws128 = torch.empty(max(fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, 1, 128, Ncap=Nk), 1), dtype=torch.uint8,
                                            device="cuda")

                        def d128():
                            return fa.fa_kvcache_decode_varlen(q128, k128, v128, cu, 1, cache_seqlens=l128, causal=True, out=o128, workspace=ws128)

                        nbytes, flops = B * L * DQK * 2, 2.0 * B * Hq * L * (DQK + DC)

                        def rates(name, us, nbytes=nbytes, flops=flops):
                            if name == "d128":
                                return f"  {nbytes / us * 1e-6:6.2f} TB/s of K+V"
                            return f"  {nbytes / us * 1e-6:6.2f} TB/s cache  {flops / us * 1e-6:7.1f} TFLOP/s"

                        variants = [("mla", mla()), ("mla'", mla()), ("torch", torch_route), ("d128", d128)]
                        if args.sweep and L == 32768 and B == 8:
                            variants += [(f"S={S}", mla(S)) for S in (1, 4, 16, 64, 256)]
                        need = fa.mla_decode_workspace_bytes(B, Hq, 1, **geo)
                        say_title = f"{typ} {form} Hq{Hq} B{B} L{L} (auto workspace {need} B)"
                        run(say_title, variants, rates)
                        del cache, q, k128, v128
                        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
