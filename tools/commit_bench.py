#!/usr/bin/env python3
"""What the commit step of tree speculation costs (profiles/kvcache_commit.txt): fa_kvcache_commit against the two ways a caller has
without it.  Per (d, cache type, cache form, sequences, word case) the contenders are timed alternately in one process, so that what
else the machine does falls on all alike:
  (a)   fa_kvcache_commit at the C ABI, descriptor prepared once, seqlens_out disjoint (copy kernel + lengths kernel)
  (a')  (a) once more: the ratio (a') / (a) per round is the run's own A/A spread
  (t)   torch advanced indexing on the same cache: one gather and one index_put per tensor, index tensors prebuilt on the device (for
        pages: page numbers and in-page rows already looked up), plus the add that updates the lengths.  e4m3fn caches are indexed as
        bytes.  Only the rows that move are indexed: with a prefix word the index tensors are empty.
  (r)   re-appending the accepted path: fa_kvcache_append_varlen of the path's kept k_new, v_new rows (fp16, total = B * a) behind the
        old lengths, descriptor prepared once (on an e4m3fn cache it quantises again).  It rewrites all a rows, moved or not.
Word cases: "prefix" 4 of 8 tokens, the low four bits (nothing moves); "4of8" the path {0,2,5,7}; "8of64" a path of 8 among 64 tokens
that ends at bit 63.
Modes: "eager" times `iters` calls between two device events (the host's enqueue is in the figure where it is the slower side);
"graph" captures the `iters` calls once and times the replay (device time alone: what the step costs inside a captured step).
Workload: Hkv 8, capacity 1024, L_b = 512 for all, pages of 16 with a shuffled table.
    python tools/commit_bench.py [--d 64 128] [--types f16 fp8] [--forms contig paged] [--seqs 8 256] [--modes eager graph]
                                 [--rounds 5 --iters 50] [--out FILE]
One line per contender: the median over the rounds of the time per call, the spread of the rounds, the ratio of the medians to (a) with
the spread of the per-round ratios.  Needs a GPU."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = {"prefix": (8, (0, 1, 2, 3)), "4of8": (8, (0, 2, 5, 7)), "8of64": (64, (0, 5, 11, 23, 30, 41, 52, 63))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--types", nargs="+", default=["f16", "fp8"])
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--seqs", type=int, nargs="+", default=[8, 256])
    ap.add_argument("--cases", nargs="+", default=list(WORDS))
    ap.add_argument("--modes", nargs="+", default=["eager", "graph"])
    ap.add_argument("--Ncap", type=int, default=1024)
    ap.add_argument("--page", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    from flashattention_kernel_project_amd import capi
    assert torch.cuda.is_available(), "commit_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, Ncap, ps = args.Hkv, args.Ncap, args.page
    L0 = Ncap // 2
    lib = fa.lib()
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(call, mode):
        """-> a function that runs `iters` calls and returns the time per call in us"""
        if mode == "graph":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                call(side.cuda_stream)                      # warm-up on the stream that will capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                stream = torch.cuda.current_stream().cuda_stream
                for _ in range(args.iters):
                    call(stream)
            run = graph.replay
        else:
            stream = torch.cuda.current_stream().cuda_stream

            def run():
                for _ in range(args.iters):
                    call(stream)

        def once():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e3 / args.iters
        return once

    def run(title, variants, base, mode):
        runners = [(name, timed(call, mode)) for name, call in variants]
        for _, once in runners:   # warm-up: code objects, clocks
            once()
        times = {name: [] for name, _ in runners}
        for _ in range(args.rounds):
            for name, once in runners:
                times[name].append(once())
        say(title)
        for name, _ in runners:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, times[base])]
            say(f"  {name:5s} {med:9.2f} us/call ({min(t):.2f} .. {max(t):.2f})  ratio to {base} {med / statistics.median(times[base]):.3f} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f})")

    say(f"Hkv{Hkv} Ncap{Ncap} L{L0} page={ps} rounds={args.rounds} iters={args.iters}")
    for d in args.d:
        for typ in args.types:
            fp8 = typ == "fp8"
            for form in args.forms:
                for B in args.seqs:
                    paged = form == "paged"
                    max_pages = Ncap // ps
                    shape = (B * max_pages, Hkv, ps, d) if paged else (B, Hkv, Ncap, d)
                    k, v = (torch.randn(shape, device="cuda", dtype=torch.float16) for _ in range(2))
                    if fp8:
                        k, v = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
                    table = torch.randperm(B * max_pages, device="cuda").to(torch.int32).view(B, max_pages) if paged else None
                    geo = dict(num_pages=shape[0], max_pages=max_pages, page_size=ps, block_table=table.data_ptr()) if paged \
                        else dict(Ncap=Ncap)
                    lens = torch.full((B,), L0, dtype=torch.int32, device="cuda")
                    out = torch.zeros(B, dtype=torch.int32, device="cuda")
                    kv_dtype = capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT
                    for case in args.cases:
                        max_new, bits = WORDS[case]
                        a = len(bits)
                        word = sum(1 << i for i in bits)
                        words = torch.full((B,), word - (1 << 64) if word >> 63 else word, dtype=torch.int64, device="cuda")
                        cd = capi.KvCommitDesc(K=k.data_ptr(), V=v.data_ptr(), seqlens_k=lens.data_ptr(), seqlens_out=out.data_ptr(),
                                               accept_mask=words.data_ptr(), kv_dtype=kv_dtype, dtype=0, B=B, Hkv=Hkv, d=d, max_new=max_new,
                                               **geo)

                        def commit(stream, cd=cd):
                            cd.stream = stream
                            assert lib.fa_kvcache_commit(C.byref(cd)) == 0

                        # (t): the rows that move, as index tensors on the device
                        moves = [(L0 + i, L0 + j) for j, i in enumerate(bits) if i != j]
                        bb = torch.arange(B, device="cuda").repeat_interleave(len(moves))
                        src = torch.tensor([s for s, _ in moves] * B, dtype=torch.int64, device="cuda")
                        dst = torch.tensor([t for _, t in moves] * B, dtype=torch.int64, device="cuda")
                        if paged:
                            i0s, i2s = table[bb, src // ps].long(), src % ps
                            i0d, i2d = table[bb, dst // ps].long(), dst % ps
                        else:
                            i0s, i2s, i0d, i2d = bb, src, bb, dst
                        hh = torch.arange(Hkv, device="cuda")[None, :]
                        kb, vb = (x.view(torch.uint8) if fp8 else x for x in (k, v))
                        s_idx, d_idx = (i0s[:, None], hh, i2s[:, None]), (i0d[:, None], hh, i2d[:, None])

                        def by_torch(stream):
                            kb[d_idx] = kb[s_idx]
                            vb[d_idx] = vb[s_idx]
                            torch.add(lens, a, out=out)

                        # (r): the path's kept rows through the packed append
                        kn, vn = (torch.randn(B * a, Hkv, d, device="cuda", dtype=torch.float16) for _ in range(2))
                        cu = torch.arange(0, B * a + 1, a, dtype=torch.int32, device="cuda")
                        ad = capi.KvAppendVarlenDesc(
                            Knew=kn.data_ptr(), Vnew=vn.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), cu_seqlens_new=cu.data_ptr(),
                            seqlens_k=lens.data_ptr(), seqlens_out=out.data_ptr(), kv_dtype=kv_dtype, B=B, Hkv=Hkv, d=d, total_new=B * a,
                            dtype=0, k_stride_t=kn.stride(0), k_stride_h=kn.stride(1), v_stride_t=vn.stride(0), v_stride_h=vn.stride(1),
                            **geo)

                        def reappend(stream, ad=ad):
                            ad.stream = stream
                            assert lib.fa_kvcache_append_varlen(C.byref(ad)) == 0

                        for mode in args.modes:
                            run(f"d{d} {typ} {form} B{B} {case} ({len(moves)} of {a} rows move) [{mode}]",
                                (("(a)", commit), ("(t)", by_torch), ("(r)", reappend), ("(a')", commit)), "(a)", mode)
                    del k, v
                    torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
