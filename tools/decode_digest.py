#!/usr/bin/env python3
"""Digests of what the eight KV-cache decode entries compute, for comparing two builds bit for bit.

    python tools/decode_digest.py            # needs a GPU: one line per case, then the graph replays
    python tools/decode_digest.py --splits   # no GPU: the split count of every launch path below, from the sizing functions

Only the package's public functions are called (fa_forward_kvcache, _paged, _fp8, _paged_fp8 and their window argument), on inputs
that are seeded on the CPU, so the same file run in two checkouts prints the same lines exactly when both compute the same bits:
`diff` of the two listings is the check.  A line is one (entry, dtype, output type, d, Nq, causal, capacity); it carries, per
window, the split count S and 12 hex digits of the sha256 of O and of lse over two ragged length sets (one with an empty and a
full sequence).  The shapes are the smallest at which each launch path is taken: B 2, Hkv 2, G 2; capacity 200 is one pass
(S = 1), 1024 is four splits; at 1024 a window of 50 gives one pass, 700 three splits, and 2000 exceeds the capacity (the clamp).
The paged entries use pages of 16 keys behind a shuffled table (capacity 208 for 200).  Last, every entry replays one captured
graph twice, the second time after cache_seqlens was rewritten in place.
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


def make_entry(torch, fa, entry, dtype, d, ncap, seed):
    """-> (call(q, lens, **kw), capacity) of one entry on a seeded cache; the paged forms see the same keys through a shuffled table"""
    from decode_bench import scatter_pages
    cap = capacity(entry, ncap)
    g = torch.Generator(device="cpu").manual_seed(seed)
    k, v = (torch.randn(B, HKV, cap, d, generator=g).to(dtype).cuda() for _ in range(2))
    scales = ()
    if "fp8" in entry:
        (k, ks), (v, vs) = fa.quantize_kv_fp8(k), fa.quantize_kv_fp8(v)
        scales = (ks * 1.25, vs * 0.75)   # not the scales of the quantisation: they must reach the kernel to matter
    if "paged" in entry:
        k, v, table = scatter_pages(torch, k, v, PAGE, seed=seed)
        fn = fa.fa_forward_kvcache_paged_fp8 if scales else fa.fa_forward_kvcache_paged
        return (lambda q, lens, **kw: fn(q, k, v, table, *scales, lens, return_lse=True, **kw)), cap
    fn = fa.fa_forward_kvcache_fp8 if scales else fa.fa_forward_kvcache
    return (lambda q, lens, **kw: fn(q, k, v, *scales, lens, return_lse=True, **kw)), cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splits", action="store_true", help="print the split counts of the cases and exit (no GPU)")
    args = ap.parse_args()
    import flashattention_kernel_project_amd as fa
    if args.splits:
        for entry, ncap, nq, d in itertools.product(ENTRIES, (200, 1024), (1, 3), (64, 128)):
            print(f"{entry:9s} Ncap{capacity(entry, ncap):<4d} Nq{nq} d{d:<3d} S by window: "
                  + " ".join(f"w{w}={splits(fa, entry, nq, ncap, d, w)}" for w in WINDOWS))
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


if __name__ == "__main__":
    main()
