#!/usr/bin/env python3
"""What fa_mla_decode_fp8 costs against the 16-bit entry on the same keys and against the only route there was for an fp8 latent cache,
and what fa_mla_append_fp8 costs against a torch quantise-and-scatter (profiles/mla_decode_fp8.txt).  On the model of
tools/mla_decode_bench.py: per (dtype, cache form, Hq, B, L) the contenders are timed alternately in one process, so that what else
the machine does falls on all alike:
  fp8      fa_mla_decode_fp8 on the cache of codes [.., 576 bytes] with its scale, one token per sequence, the library's split count
  fp8'     the same call once more: the ratio fp8' / fp8 per round is the run's own A/A spread
  16bit    fa_mla_decode on a 16-bit cache holding the same keys (code * c_scale, rounded to the type)
  widen    c8.to(dtype) followed by fa_mla_decode: what a caller with an fp8 latent cache had to do before this entry (the whole cache or
           pool is widened on every call; the scale is left out, which favours this route)
    python tools/mla_decode_fp8_bench.py [--Hq 16 128] [--B 8 64] [--L 4096 32768] [--types f16 bf16] [--forms contig paged]
                                         [--rounds 5 --iters 10] [--no-append] [--out FILE]
One line per contender: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds,
and the cache rate B * L * (576 or 1152) B / t computed from the shape.  Behind the table: every row where fp8 is NOT ahead of 16bit by
more than the run's A/A spread, and every row where it loses to widen.  Then the append: fa_mla_append_fp8 against quantize_mla_fp8 plus
an index_copy_ into the cache.  Needs a GPU."""
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "mla_decode_fp8_bench needs a GPU"
    torch.manual_seed(0)
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, rates):
        """variants: (name, call); rates(name, us) -> a suffix for the line.  -> {name: (median, per-round times)}"""
        for _, call in variants:
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
        return {name: (statistics.median(t), t) for name, t in times.items()}

    say(f"fa_mla_decode_fp8, one token per sequence, causal, rounds={args.rounds} iters={args.iters} page={PAGE} ({fa.version()})")
    c_scale = torch.tensor([6.0 / 448.0], dtype=torch.float32, device="cuda")   # N(0,1) keys: 6 sigma on the top code
    findings = []
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
                        c8 = torch.empty(B, cap, DQK, device="cuda", dtype=torch.float8_e4m3fn)
                        c16 = torch.empty(B, cap, DQK, device="cuda", dtype=tdt)
                        for b in range(B):   # one sequence at a time: the fp32 temporaries stay small
                            codes = fa.quantize_mla_fp8(torch.randn(cap, DQK, device="cuda"), c_scale)[0]
                            c8.view(torch.uint8)[b] = codes.view(torch.uint8)
                            c16[b] = (codes.float() * c_scale).to(tdt)
                        table = None
                        if form == "paged":
                            pages = B * cap // PAGE
                            table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, cap // PAGE)
                            c8, c16 = c8.view(pages, PAGE, DQK), c16.view(pages, PAGE, DQK)
                            geo = dict(max_pages=cap // PAGE, page_size=PAGE)
                        else:
                            geo = dict(Ncap=cap)
                        out = torch.empty(B, Hq, DC, device="cuda", dtype=tdt)
                        need = fa.mla_decode_workspace_bytes(B, Hq, 1, **geo)
                        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
                        kw = dict(cache_seqlens=lens, block_table=table, causal=True, out=out, workspace=ws)

                        def fp8(q=q, c8=c8, cu=cu, kw=kw):
                            return fa.fa_mla_decode_fp8(q, c8, cu, 1, c_scale=c_scale, **kw)

                        def bit16(q=q, c16=c16, cu=cu, kw=kw):
                            return fa.fa_mla_decode(q, c16, cu, 1, **kw)

                        def widen(q=q, c8=c8, cu=cu, kw=kw, tdt=tdt):
                            return fa.fa_mla_decode(q, c8.to(tdt), cu, 1, **kw)

                        n8, n16 = B * L * DQK, B * L * DQK * 2

                        def rates(name, us, n8=n8, n16=n16):
                            if name == "16bit":
                                return f"  {n16 / us * 1e-6:6.2f} TB/s of 16-bit cache"
                            if name == "widen":
                                return f"  {n8 / us * 1e-6:6.2f} TB/s of codes (plus the widened copy written and read)"
                            return f"  {n8 / us * 1e-6:6.2f} TB/s of codes"

                        title = f"{typ} {form} Hq{Hq} B{B} L{L} (auto workspace {need} B)"
                        res = run(title, [("fp8", fp8), ("fp8'", fp8), ("16bit", bit16), ("widen", widen)], rates)
                        aa = [x / y for x, y in zip(res["fp8'"][1], res["fp8"][1])]
                        spread = max(max(aa), 1.0 / min(aa))
                        gain = res["16bit"][0] / res["fp8"][0]
                        if gain <= spread:
                            findings.append(f"NOT ahead of 16bit: {title.split(' (')[0]}: 16bit / fp8 = x{gain:.3f}, A/A spread x{spread:.3f}")
                        if res["widen"][0] <= res["fp8"][0]:
                            findings.append(f"LOSES to widen: {title.split(' (')[0]}: widen / fp8 = x{res['widen'][0] / res['fp8'][0]:.3f}")
                        del c8, c16, q
                        torch.cuda.empty_cache()
    say("")
    say("rows where fa_mla_decode_fp8 is NOT ahead of fa_mla_decode by more than the row's A/A spread, or loses to widen-first:")
    for line in findings or ["  (none)"]:
        say("  " + line.strip())

    if not args.no_append:
        say("")
        say("fa_mla_append_fp8 against quantize_mla_fp8 + index_copy_ (contiguous cache, capacity 4096, lengths 1000)")
        for typ in args.types:
            tdt = torch.float16 if typ == "f16" else torch.bfloat16
            for B, m in ((64, 1), (8, 512)):
                cap, total = 4096, B * m
                cache = torch.zeros(B, cap, DQK, device="cuda", dtype=torch.float8_e4m3fn)
                new = torch.randn(total, DQK, device="cuda", dtype=tdt)
                cu = (torch.arange(B + 1, device="cuda") * m).to(torch.int32)
                lens = torch.full((B,), 1000, dtype=torch.int32, device="cuda")
                rows = (torch.arange(B, device="cuda").repeat_interleave(m) * cap + 1000 + torch.arange(m, device="cuda").repeat(B)).long()
                flat = cache.view(B * cap, DQK).view(torch.uint8)

                def entry(new=new, cache=cache, cu=cu, lens=lens):
                    return fa.fa_mla_append_fp8(new, cache, cu, cache_seqlens=lens, c_scale=c_scale)

                def torch_route(new=new, flat=flat, rows=rows):
                    return flat.index_copy_(0, rows, fa.quantize_mla_fp8(new, c_scale)[0].view(torch.uint8))

                nbytes = total * DQK * 3   # 2 bytes read, 1 written per element

                def rates(name, us, nbytes=nbytes):
                    return f"  {nbytes / us * 1e-6:7.4f} TB/s (read + written)"

                run(f"append {typ} B{B} x {m} tokens", [("entry", entry), ("entry'", entry), ("torch", torch_route)], rates)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
