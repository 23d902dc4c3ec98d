#!/usr/bin/env python3
"""What a query count per sequence costs and saves on the KV-cache step (profiles/kvcache_ragged.txt).  Five groups, each with its
variants timed alternately in one process, so that what else the machine does falls on all of them alike:
  (a) padded Nq = 8, every n_b = 1: the ragged call, the un-ragged Nq = 8 call, the un-ragged Nq = 1 call
  (b) the ragged call with half the slots idle (n_b = 0) against all slots live (n_b = 1)
  (c) padded Nq = 512 with one sequence at 512 and the others at 1 (the split count follows the padded G * Nq), against the same
      batch un-ragged and against the one-token sequences alone at Nq = 1
  (d) the ragged append of 1 token in Nnew = 8 padding against the flat Nnew = 1 append, through the Python front ends and (d')
      through the C entries with the arguments prepared once
  (e) the descriptor with seqlens_q == NULL against the flat entry (the same kernels): the run-to-run spread
    python tools/ragged_bench.py [--B 8 --Hkv 16 --G 4 --Nk 32768 --d 128] [--rounds 7 --iters 40]
One line per variant: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds
(min .. max), the split count of the call, and the ratio of the medians to the group's first variant with the spread of the per-round
ratios.  Needs a GPU."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--Hkv", type=int, default=16)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--Nk", type=int, default=32768)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--pad", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    from flashattention_kernel_project_amd import capi
    assert torch.cuda.is_available(), "ragged_bench needs a GPU"
    torch.manual_seed(0)
    B, Hkv, G, Nk, d = args.B, args.Hkv, args.G, args.Nk, args.d
    dev = dict(device="cuda", dtype=torch.float16)
    k, v = torch.randn(B, Hkv, Nk, d, **dev), torch.randn(B, Hkv, Nk, d, **dev)
    lens = torch.full((B,), Nk - args.chunk, dtype=torch.int32, device="cuda")
    ints = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")

    def decode(Nq, nq=None, batch=slice(None)):
        """-> (call, split count) of one decode over the sequences `batch` with Nq padded rows"""
        b = len(range(B)[batch])
        q = torch.randn(b, Hkv * G, Nq, d, **dev)
        need = fa.kvcache_workspace_bytes(b, Hkv, G, Nq, Nk, d)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        kw = dict(cache_seqlens=lens[batch].contiguous(), causal=True, workspace=ws)
        if nq is not None:
            kw["seqlens_q"] = ints(nq)
        kk, vv = k[batch], v[batch]
        return (lambda: fa.fa_forward_kvcache(q, kk, vv, **kw)), max(need // (b * Hkv * G * Nq * (d + 2) * 4), 1)

    def run(title, variants):
        for _, (call, _) in variants:   # warm-up: code objects, the LDS attribute
            for _ in range(5):
                call()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, (call, _) in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        print(title)
        base = times[variants[0][0]]
        for name, (_, S) in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            print(f"  {name:34s} {med:9.2f} us/call ({min(t):.2f} .. {max(t):.2f})  S={S if S else '-':>3}  "
                  f"ratio to the first {med / statistics.median(base):.3f} (per round {min(ratios):.3f} .. {max(ratios):.3f})")

    head = f"B{B} Hkv{Hkv} G{G} Nk{Nk} (lengths {Nk - args.chunk}) d{d} fp16 causal rounds={args.rounds} iters={args.iters}"
    P = args.pad
    run(f"(a) {head}: padded Nq = {P}, every n_b = 1",
        ((f"ragged Nq={P} n_b=1", decode(P, [1] * B)), (f"un-ragged Nq={P}", decode(P)), ("un-ragged Nq=1", decode(1))))
    half = [1 if b % 2 == 0 else 0 for b in range(B)]
    run(f"(b) {head}: padded Nq = {P}, half the slots idle",
        ((f"ragged Nq={P} all n_b=1", decode(P, [1] * B)), (f"ragged Nq={P} half n_b=0", decode(P, half)),
         (f"un-ragged Nq=1, B={B // 2}", decode(1, batch=slice(0, B // 2)))))
    C = args.chunk
    run(f"(c) {head}: padded Nq = {C}, one sequence at {C} and {B - 1} at 1 (the known limit: splits follow the padded G * Nq)",
        ((f"ragged Nq={C} n=({C},1,..)", decode(C, [C] + [1] * (B - 1))), (f"un-ragged Nq={C}", decode(C)),
         (f"un-ragged Nq=1, B={B - 1}", decode(1, batch=slice(1, B))), (f"un-ragged Nq={C}, B=1", decode(C, batch=slice(0, 1)))))

    # (d) the append
    def append(Nnew, new=None):
        kn, vn = torch.randn(B, Hkv, Nnew, d, **dev), torch.randn(B, Hkv, Nnew, d, **dev)
        kw = dict(cache_seqlens=lens) if new is None else dict(cache_seqlens=lens, seqlens_new=ints(new))
        return (lambda: fa.fa_kvcache_append(kn, vn, k, v, **kw)), 0

    run(f"(d) {head}: append, through the Python front ends",
        ((f"ragged Nnew={P} m_b=1", append(P, [1] * B)), ("flat Nnew=1", append(1)), (f"flat Nnew={P}", append(P))))

    # ... and through the C entries, with every argument prepared once: what is left is the library's host path and the kernels
    L = capi.lib()
    st = torch.cuda.current_stream().cuda_stream

    def append_c(Nnew, new=None):
        kn, vn = torch.randn(B, Hkv, Nnew, d, **dev), torch.randn(B, Hkv, Nnew, d, **dev)
        if new is None:
            return (lambda: L.fa_kvcache_append(kn.data_ptr(), vn.data_ptr(), k.data_ptr(), v.data_ptr(), lens.data_ptr(), None, B, Hkv,
                                                Nnew, Nk, d, 0, st)), 0
        cnt = ints(new)
        desc = capi.KvAppendDesc(Knew=kn.data_ptr(), Vnew=vn.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), seqlens_k=lens.data_ptr(),
                                 seqlens_new=cnt.data_ptr(), B=B, Hkv=Hkv, Nnew=Nnew, d=d, Ncap=Nk, dtype=0, stream=st)
        keep = (kn, vn, cnt, desc)
        return (lambda: L.fa_kvcache_append_ex(ctypes.byref(keep[3]))), 0

    run(f"(d') {head}: append, through the C entries",
        ((f"ragged Nnew={P} m_b=1", append_c(P, [1] * B)), ("flat Nnew=1", append_c(1)), (f"flat Nnew={P}", append_c(P)),
         (f"ragged Nnew={P} m_b={P}", append_c(P, [P] * B))))

    # (e) the descriptor without the vector against the flat entry: the same kernels
    q = torch.randn(B, Hkv * G, 1, d, **dev)
    o = torch.empty(B, Hkv * G, 1, d, device="cuda", dtype=torch.float32)
    need = fa.kvcache_workspace_bytes(B, Hkv, G, 1, Nk, d)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    desc = capi.KvDecodeDesc(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=o.data_ptr(), seqlens_k=lens.data_ptr(), B=B, Hkv=Hkv, G=G,
                             Nq=1, d=d, Ncap=Nk, scale=d ** -0.5, causal=1, in_dtype=0, out_dtype=0, workspace=ws.data_ptr(),
                             workspace_bytes=need, stream=st)
    S = max(need // (B * Hkv * G * (d + 2) * 4), 1)
    flat = lambda: L.fa_forward_kvcache(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, lens.data_ptr(), B, Hkv, G, 1, Nk, d,
                                        d ** -0.5, 1, 0, 0, ws.data_ptr(), need, st)
    by_desc = lambda: L.fa_kvcache_decode(ctypes.byref(desc))
    run(f"(e) {head}: Nq = 1 through the C entries, seqlens_q == NULL",
        (("flat fa_forward_kvcache", (flat, S)), ("fa_kvcache_decode, no seqlens_q", (by_desc, S)), ("flat again", (flat, S))))


if __name__ == "__main__":
    main()
