#!/usr/bin/env python3
"""What fa_mla_decode_sparse costs, against two yardsticks that are not the code under test (profiles/mla_sparse.txt).  Per (cache
form, Hq, tokens, topk, L) the contenders are timed alternately in one process, so that what else the machine does falls on all alike:
  sparse   fa_mla_decode_sparse, one token per sequence, topk distinct random keys of [0, L) per token, the library's split count
           (out and workspace prepared once)
  sparse'  the same call once more: the ratio sparse' / sparse per round is the run's own A/A spread
  dense    yardstick (a): fa_mla_decode on a CONTIGUOUS cache of exactly topk keys per sequence with the same number of splits --
           the same bytes and the same arithmetic without the gather, so sparse / dense is the gather's price
  torch    yardstick (b), the route there was: index_select of the listed rows (paged: through the table) into (tokens, topk, 576),
           then softmax(scale * q C^T) C[:, :, :512] as two 16-bit torch.bmm with a softmax between them
    python tools/mla_sparse_bench.py [--Hq 16 128] [--tokens 8 64] [--topk 512 2048] [--L 8192 65536] [--forms contig paged]
                                     [--type bf16] [--rounds 5 --iters 20] [--out FILE]
One line per contender: the median over the rounds of the time per call (device events around `iters` calls), the spread of the
rounds, the ratio to `sparse`, and for the library's calls the row rate tokens * topk * 1152 B / t computed from the shape.  Needs a
GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DQK, DC, PAGE = 576, 512, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Hq", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--tokens", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--topk", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--L", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--type", default="bf16", choices=["f16", "bf16"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "mla_sparse_bench needs a GPU"
    torch.manual_seed(0)
    sink = open(args.out, "w") if args.out else None
    tdt = torch.float16 if args.type == "f16" else torch.bfloat16
    scale = DQK ** -0.5

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, nbytes):
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
            rate = "" if name == "torch" else f"  {nbytes / med * 1e-6:6.2f} TB/s of rows"
            say(f"  {name:8s} {med:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  x{med / statistics.median(base):.3f} of sparse "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f}){rate}")

    say(f"fa_mla_decode_sparse, {args.type}, one token per sequence, causal, rounds={args.rounds} iters={args.iters} page={PAGE} "
        f"({fa.version()})")
    for form in args.forms:
        for Hq in args.Hq:
            for B in args.tokens:
                for L in args.L:
                    cache = torch.randn(B, L, DQK, device="cuda", dtype=tdt)
                    table, geo = None, dict(Ncap=L)
                    if form == "paged":
                        pages = B * L // PAGE
                        table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, L // PAGE)
                        cache, geo = cache.view(pages, PAGE, DQK), dict(max_pages=L // PAGE, page_size=PAGE)
                    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
                    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
                    q = torch.randn(B, Hq, DQK, device="cuda", dtype=tdt)
                    out = torch.empty(B, Hq, DC, device="cuda", dtype=tdt)
                    for topk in args.topk:
                        idx = torch.stack([torch.randperm(L, device="cuda")[:topk] for _ in range(B)]).to(torch.int32)
                        need = fa.mla_decode_sparse_workspace_bytes(B, Hq, 1, topk, **geo)
                        S = max(1, need // (B * ((Hq + 63) // 64) * 64 * (DC + 4) * 4))   # the library's choice, read off its workspace
                        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")

                        def sparse():
                            return fa.fa_mla_decode_sparse(q, cache, idx, cu, 1, cache_seqlens=lens, block_table=table, causal=True,
                                                           out=out, workspace=ws)

                        small = torch.randn(B, topk, DQK, device="cuda", dtype=tdt)
                        lens_s = torch.full((B,), topk, dtype=torch.int32, device="cuda")
                        ws_d = torch.empty(max(fa.mla_decode_workspace_bytes(B, Hq, 1, Ncap=topk, num_splits=S), 1), dtype=torch.uint8,
                                           device="cuda")

                        def dense():
                            return fa.fa_mla_decode(q, small, cu, 1, cache_seqlens=lens_s, causal=True, num_splits=S, out=out, workspace=ws_d)

                        flat = cache.view(-1, DQK)
                        if table is None:
                            slots = (idx.long() + torch.arange(B, device="cuda")[:, None] * L).view(-1)
                        else:
                            slots = (torch.gather(table.long(), 1, idx.long() // PAGE) * PAGE + idx.long() % PAGE).view(-1)

                        def torch_route():
                            c = flat.index_select(0, slots).view(B, topk, DQK)
                            p = torch.softmax(torch.bmm(q, c.transpose(1, 2)) * scale, dim=-1)
                            return torch.bmm(p, c[:, :, :DC])

                        run(f"{form} Hq{Hq} tokens{B} topk{topk} L{L} (S={S}, workspace {need} B)",
                            [("sparse", sparse), ("sparse'", sparse), ("dense", dense), ("torch", torch_route)], B * topk * DQK * 2)
                    del cache, q
                    torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
