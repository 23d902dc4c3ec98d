#!/usr/bin/env python3
"""What the token-packed decode entry costs against the routes there were (profiles/kvcache_decode_varlen.txt).  Per (d, cache form,
cache type, shape) five contenders are timed alternately in one process, so that what else the machine does falls on all alike:
  new      fa_kvcache_decode_varlen on the packed Q (out, lse-less, workspace prepared once)
  (a) pad  the route through the padded entry: gather the packed Q into [B,Hq,Nq,d] in torch (host-known lengths, the index prepared
           once), fa_forward_kvcache*(seqlens_q), scatter O back into the packed layout
  (a) pre  fa_forward_varlen_kvcache* on the same packed Q
  (b)      the padded entry alone, on data that already lies padded
  (b')     (b) once more: the ratio (b') / (b) per round is the run's own A/A spread
Workload: Hkv 8, G 4, fp16, causal; shapes: 8 sequences x {1, 16, 128, 256} rows over 32768 keys, 256 x 1 over 4096 keys, one 128-row
chunk beside 15 one-token sequences over 32768 keys.
    python tools/decode_varlen_bench.py [--d 64 128] [--rounds 5 --iters 20] [--forms contig paged] [--types f16 fp8] [--out FILE]
One line per contender: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds,
the ratio of the medians to (b) with the spread of the per-round ratios.  Needs a GPU."""
import argparse
import itertools
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("8x1", [1] * 8, 32768), ("8x16", [16] * 8, 32768), ("8x128", [128] * 8, 32768), ("8x256", [256] * 8, 32768),
          ("256x1", [1] * 256, 4096), ("128+15x1", [128] + [1] * 15, 32768)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--types", nargs="+", default=["f16", "fp8"])
    ap.add_argument("--shapes", nargs="+", default=[s[0] for s in SHAPES])
    ap.add_argument("--page", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    assert torch.cuda.is_available(), "decode_varlen_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, G = args.Hkv, args.G
    Hq = Hkv * G
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants):
        for _, call in variants:   # warm-up: code objects, the LDS attribute
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
        base = times["(b)"]
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            say(f"  {name:8s} {med:9.2f} us/call ({min(t):.2f} .. {max(t):.2f})  ratio to (b) {med / statistics.median(base):.3f} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f})")

    say(f"Hkv{Hkv} G{G} fp16 causal rounds={args.rounds} iters={args.iters} page={args.page}")
    for d in args.d:
        for name, n, Nk in SHAPES:
            if name not in args.shapes:
                continue
            B, Nq, T = len(n), max(n), sum(n)
            lens = torch.full((B,), Nk - 64, dtype=torch.int32, device="cuda")
            cu = torch.tensor([0] + list(itertools.accumulate(n)), dtype=torch.int32, device="cuda")
            nq = torch.tensor(n, dtype=torch.int32, device="cuda")
            q = torch.randn(T, Hq, d, device="cuda", dtype=torch.float16)
            # the gather of the pad route: token of (b, i), 0 for a dead row; the live rows' (b, i) and tokens for the way back
            tok = torch.zeros(B, Nq, dtype=torch.long, device="cuda")
            bi, ii, ti = [], [], []
            for b, (s, m) in enumerate(zip(cu.tolist(), n)):
                tok[b, :m] = torch.arange(s, s + m, device="cuda")
                bi += [b] * m
                ii += list(range(m))
                ti += list(range(s, s + m))
            bi, ii, ti = (torch.tensor(x, dtype=torch.long, device="cuda") for x in (bi, ii, ti))
            qpad = q[tok].permute(0, 2, 1, 3).contiguous()
            for form in args.forms:
                for typ in args.types:
                    fp8 = typ == "fp8"
                    if form == "paged":
                        pages = B * (Nk // args.page)
                        shape = (pages, Hkv, args.page, d)
                        table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, Nk // args.page)
                    else:
                        shape, table = (B, Hkv, Nk, d), None
                    k, v = (torch.randn(shape, device="cuda", dtype=torch.float16) for _ in range(2))
                    if fp8:
                        k, v = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
                    geo = dict(max_pages=Nk // args.page, page_size=args.page) if table is not None else dict(Ncap=Nk)
                    need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, Nq, d, **geo)
                    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
                    S = max(need // (B * Hkv * G * Nq * (d + 2) * 4), 1)
                    out = torch.zeros(T, Hq, d, device="cuda", dtype=torch.float32)
                    new_fn = fa.fa_kvcache_decode_varlen_fp8 if fp8 else fa.fa_kvcache_decode_varlen
                    pre_fn = fa.fa_forward_varlen_kvcache_fp8 if fp8 else fa.fa_forward_varlen_kvcache
                    pad_fn = getattr(fa, "fa_forward_kvcache" + ("_paged" if table is not None else "") + ("_fp8" if fp8 else ""))
                    lead = (k, v, table) if table is not None else (k, v)
                    kw = dict(cache_seqlens=lens, causal=True, workspace=ws, seqlens_q=nq)
                    out2 = torch.zeros(T, Hq, d, device="cuda", dtype=torch.float32)

                    def new():
                        return new_fn(q, k, v, cu, Nq, lens, table, causal=True, out=out, workspace=ws)

                    def pre():
                        return pre_fn(q, k, v, cu, lens, table, causal=True, out=out2)

                    def padded():
                        return pad_fn(qpad, *lead, **kw)

                    def pad_route():
                        o = pad_fn(q[tok].permute(0, 2, 1, 3).contiguous(), *lead, **kw)
                        out2[ti] = o.permute(0, 2, 1, 3)[bi, ii]
                        return out2

                    # the contenders agree before they are timed: the new entry has the padded entry's bits on the live rows
                    a, b = new().clone(), padded().permute(0, 2, 1, 3)[bi, ii]
                    torch.cuda.synchronize()
                    assert torch.equal(a[ti], b), "the new entry and the padded entry differ"
                    run(f"d{d} {form} {typ} {name} over {Nk} keys (B={B} max_q={Nq} total_q={T} S={S})",
                        (("(b)", padded), ("new", new), ("(a) pad", pad_route), ("(a) pre", pre), ("(b')", padded)))
                    del k, v, ws
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
