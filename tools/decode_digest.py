#!/usr/bin/env python3
"""Digests of what the KV-cache decode entries compute, for comparing two builds bit for bit.

    python tools/decode_digest.py            # needs a GPU: one line per case, then the graph replays
    python tools/decode_digest.py --splits   # no GPU: the split count of every launch path below, from the sizing functions

Only the package's public functions are called (fa_forward_kvcache, _paged, _fp8, _paged_fp8 and their window argument), on inputs
that are seeded on the CPU, so the same file run in two checkouts prints the same lines exactly when both compute the same bits:
`diff` of the two listings is the check.  A line is one (entry, dtype, output type, d, Nq, causal, capacity); it carries, per
window, the split count S and 12 hex digits of the sha256 of O and of lse over two ragged length sets (one with an empty and a
full sequence).  The shapes are the smallest at which each launch path is taken: B 2, Hkv 2, G 2; capacity 200 is one pass
(S = 1), 1024 is four splits; at 1024 a window of 50 gives one pass, 700 three splits, and 2000 exceeds the capacity (the clamp).
The paged entries use pages of 16 keys behind a shuffled table (capacity 208 for 200).  Then every entry replays one captured
graph twice, the second time after cache_seqlens was rewritten in place.

Last come the entries above the flat ones, one dtype pair (fp16 in, fp32 out) each, on the four cache forms, d 64 / 128 and both
capacities, so that every merge runs one-pass and behind a split: `decode` lines are fa_forward_kvcache* with sinks and a soft-cap,
with a soft-cap alone, and with seqlens_q (with and without sinks; once under window 700); `varlen` lines are
fa_kvcache_decode_varlen[_fp8] on rows (2, 5) cut at max_seqlen_q 3, causal and under a tree mask that is no triangle, each also with
sinks; `attend` lines are fa_kvcache_attend_varlen[_fp8] on the same rows with split_rows 3, so the second sequence runs on the tiled
kernel and all its rows are written, which the varlen lines leave at 0 / -inf.
"""
import argparse
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HKV, G, PAGE = 2, 2, 2, 16
WINDOWS = (0, 50, 700, 2000)
ENTRIES = ("kvcache", "paged", "fp8", "paged_fp8")


def capacity(entry, ncap):
    return -(-ncap // PAGE) * PAGE if "paged" in entry else ncap


def splits(fa, entry, nq, ncap, d, window):
    """The split count of a launch, from the workspace the sizing functions ask for (0 bytes: one pass)."""
    cap = capacity(entry, ncap)
    if "paged" in entry:
        need = fa.kvcache_paged_window_workspace_bytes(B, HKV, G, nq, cap // PAGE, PAGE, d, window)
    else:
        need = fa.kvcache_window_workspace_bytes(B, HKV, G, nq, cap, d, window)
    per_split = B * HKV * G * nq * (d + 2) * 4
    assert need % per_split == 0
    return need // per_split or 1


def digest(tensors):
    import torch
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:12]


def make_cache(torch, fa, entry, dtype, d, ncap, seed):
    """-> (k, v, table or None, scales, capacity): a seeded cache; the paged forms hold the same keys behind a shuffled table"""
    from decode_bench import scatter_pages
    cap = capacity(entry, ncap)
    g = torch.Generator(device="cpu").manual_seed(seed)
    k, v = (torch.randn(B, HKV, cap, d, generator=g).to(dtype).cuda() for _ in range(2))
    scales, table = (), None
    if "fp8" in entry:
        (k, ks), (v, vs) = fa.quantize_kv_fp8(k), fa.quantize_kv_fp8(v)
        scales = (ks * 1.25, vs * 0.75)   # not the scales of the quantisation: they must reach the kernel to matter
    if "paged" in entry:
        k, v, table = scatter_pages(torch, k, v, PAGE, seed=seed)
    return k, v, table, scales, cap


def make_entry(torch, fa, entry, dtype, d, ncap, seed):
    """-> (call(q, lens, **kw), capacity) of one flat entry on a seeded cache"""
    k, v, table, scales, cap = make_cache(torch, fa, entry, dtype, d, ncap, seed)
    if table is not None:
        fn = fa.fa_forward_kvcache_paged_fp8 if scales else fa.fa_forward_kvcache_paged
        return (lambda q, lens, **kw: fn(q, k, v, table, *scales, lens, return_lse=True, **kw)), cap
    fn = fa.fa_forward_kvcache_fp8 if scales else fa.fa_forward_kvcache
    return (lambda q, lens, **kw: fn(q, k, v, *scales, lens, return_lse=True, **kw)), cap


MAX_Q, CU_Q = 3, (0, 2, 7)       # rows (2, 5): the second sequence is cut at MAX_Q by the varlen entry and routed to the tiled kernel by attend
TREE = (1, 3, 1, 3, 5, 0, 0)     # per token row: a chain of two; a root with two children (no triangle); rows past MAX_Q are not read


def make_varlen(torch, fa, entry, d, ncap, seed):
    """-> (varlen(q, lens, **kw), attend(q, lens, **kw), capacity): the packed entries on a seeded fp16 cache, rows as CU_Q says"""
    k, v, table, scales, cap = make_cache(torch, fa, entry, torch.float16, d, ncap, seed)
    cu = torch.tensor(CU_Q, dtype=torch.int32).cuda()
    kw8 = dict(k_scale=scales[0], v_scale=scales[1]) if scales else {}
    dec = fa.fa_kvcache_decode_varlen_fp8 if scales else fa.fa_kvcache_decode_varlen
    att = fa.fa_kvcache_attend_varlen_fp8 if scales else fa.fa_kvcache_attend_varlen
    return ((lambda q, lens, **kw: dec(q, k, v, cu, MAX_Q, lens, table, return_lse=True, out_dtype=torch.float32, **kw8, **kw)),
            (lambda q, lens, **kw: att(q, k, v, cu, lens, table, split_rows=MAX_Q, return_lse=True, out_dtype=torch.float32, **kw8, **kw)),
            cap)


def varlen_splits(fa, entry, ncap, d, window):
    """The split count of a packed launch, from the workspace its sizing function asks for (0 bytes: one pass)."""
    cap = capacity(entry, ncap)
    where = dict(max_pages=cap // PAGE, page_size=PAGE) if "paged" in entry else dict(Ncap=cap)
    need = fa.kvcache_decode_varlen_workspace_bytes(B, HKV, G, MAX_Q, d, window=window, **where)
    per_split = B * HKV * G * MAX_Q * (d + 2) * 4
    assert need % per_split == 0
    return need // per_split or 1


def upper_lines(torch, fa, seed):
    """The `decode`, `varlen` and `attend` lines: (what, run(call, q, lens) per cell) on each cache form, d and capacity."""
    for entry, d, ncap in itertools.product(ENTRIES, (64, 128), (200, 1024)):
        seed += 1
        g = torch.Generator(device="cpu").manual_seed(2000 + seed)
        sinks = (torch.randn(HKV * G, generator=g) * 2).cuda()
        q = torch.randn(B, HKV * G, MAX_Q, d, generator=g).half().cuda()
        qp = torch.randn(CU_Q[-1], HKV * G, d, generator=g).half().cuda()
        counts = torch.tensor((1, 3), dtype=torch.int32).cuda()
        tree = torch.tensor(TREE, dtype=torch.int64).cuda()
        call, cap = make_entry(torch, fa, entry, torch.float16, d, ncap, seed)
        varlen, attend, _ = make_varlen(torch, fa, entry, d, ncap, seed)
        lens = [torch.tensor(x, dtype=torch.int32).cuda() for x in ((0, cap), (cap // 3 + 1, cap - 5))]
        s0, s700 = splits(fa, entry, MAX_Q, ncap, d, 0), splits(fa, entry, MAX_Q, ncap, d, 700)
        v0, v700 = varlen_splits(fa, entry, ncap, d, 0), varlen_splits(fa, entry, ncap, d, 700)
        flat = dict(causal=True, out_dtype=torch.float32)
        rows = (("decode", call, q, ((f"sinks+cap S{s0}", dict(flat, sinks=sinks, softcap=30.0)),
                                     (f"cap S{s0}", dict(flat, softcap=30.0)),
                                     (f"seqlens_q S{s0}", dict(flat, seqlens_q=counts)),
                                     (f"seqlens_q+sinks S{s0}", dict(flat, seqlens_q=counts, sinks=sinks)),
                                     (f"seqlens_q+sinks w700 S{s700}", dict(flat, seqlens_q=counts, sinks=sinks, window=700)))),
                ("varlen", varlen, qp, ((f"causal S{v0}", dict(causal=True)),
                                        (f"causal+sinks w700 S{v700}", dict(causal=True, sinks=sinks, window=700)),
                                        (f"tree S{v0}", dict(causal=True, tree_mask=tree)),
                                        (f"tree+sinks+cap S{v0}", dict(causal=True, tree_mask=tree, sinks=sinks, softcap=30.0)))),
                ("attend", attend, qp, ((f"plain S{v0}", dict()),
                                        (f"sinks w700 S{v700}", dict(sinks=sinks, window=700)),
                                        (f"short half S{v0}", dict(parts=1)))))
        for what, fn, qq, cells in rows:
            out = []
            for label, kw in cells:
                got = [fn(qq, L, **kw) for L in lens]
                out.append(f"{label} O:{digest(o for o, _ in got)} lse:{digest(l for _, l in got)}")
            print(f"{what:6s} {entry:9s} d{d:<3d} Ncap{cap:<4d} | " + " | ".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splits", action="store_true", help="print the split counts of the cases and exit (no GPU)")
    args = ap.parse_args()
    import flashattention_kernel_project_amd as fa
    if args.splits:
        for entry, ncap, nq, d in itertools.product(ENTRIES, (200, 1024), (1, 3), (64, 128)):
            print(f"{entry:9s} Ncap{capacity(entry, ncap):<4d} Nq{nq} d{d:<3d} S by window: "
                  + " ".join(f"w{w}={splits(fa, entry, nq, ncap, d, w)}" for w in WINDOWS))
        for entry, ncap, d in itertools.product(ENTRIES, (200, 1024), (64, 128)):
            print(f"varlen {entry:9s} Ncap{capacity(entry, ncap):<4d} max_q{MAX_Q} d{d:<3d} S by window: "
                  + " ".join(f"w{w}={varlen_splits(fa, entry, ncap, d, w)}" for w in (0, 700)))
        return
    import torch
    seed = 0
    for entry, dtype, d, ncap in itertools.product(ENTRIES, (torch.float16, torch.bfloat16), (64, 128), (200, 1024)):
        seed += 1
        call, cap = make_entry(torch, fa, entry, dtype, d, ncap, seed)
        lens = [torch.tensor(x, dtype=torch.int32).cuda() for x in ((0, cap), (cap // 3 + 1, cap - 5))]
        for nq, out32, causal in itertools.product((1, 3), (True, False), (False, True)):
            g = torch.Generator(device="cpu").manual_seed(1000 + seed)
            q = torch.randn(B, HKV * G, nq, d, generator=g).to(dtype).cuda()
            cells = []
            for w in WINDOWS:
                got = [call(q, L, causal=causal, out_dtype=torch.float32 if out32 else dtype, window=w) for L in lens]
                cells.append(f"w{w} S{splits(fa, entry, nq, ncap, d, w)} O:{digest(o for o, _ in got)} lse:{digest(l for _, l in got)}")
            print(f"{entry:9s} {str(dtype)[6:]:8s} out{'32' if out32 else '16'} d{d:<3d} Nq{nq} causal{int(causal)} Ncap{cap:<4d} | "
                  + " | ".join(cells))
    # one captured graph per entry (window 0: the four base entries, 700: their window forms), replayed before and after the
    # lengths change in place
    for entry, w in itertools.product(ENTRIES, (0, 700)):
        seed += 1
        call, cap = make_entry(torch, fa, entry, torch.float16, 128, 1024, seed)
        g = torch.Generator(device="cpu").manual_seed(1000 + seed)
        q = torch.randn(B, HKV * G, 1, 128, generator=g).half().cuda()
        lens = torch.tensor((300, cap), dtype=torch.int32).cuda()
        ws = torch.empty(max(fa.kvcache_workspace_bytes(B, HKV, G, 1, cap, 128), 1), dtype=torch.uint8).cuda()   # covers any window
        call(q, lens.clone(), causal=True, window=w, workspace=ws)   # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            o, lse = call(q, lens, causal=True, window=w, workspace=ws)
        cells = []
        for now in ((300, cap), (1000, 17)):
            lens.copy_(torch.tensor(now, dtype=torch.int32))
            o.fill_(float("nan")), lse.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            cells.append(f"lengths {now} O:{digest([o])} lse:{digest([lse])}")
        print(f"graph {entry:9s} window {w:<3d} S{splits(fa, entry, 1, 1024, 128, w)} | " + " | ".join(cells))
    upper_lines(torch, fa, seed)


if __name__ == "__main__":
    main()
