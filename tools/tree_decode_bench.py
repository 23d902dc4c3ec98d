#!/usr/bin/env python3
"""What the tree mask costs on the packed split-KV decode, and explicit positions on the packed append (profiles/kvcache_tree.txt).
Per (d, cache form, cache type, keys, sequences x tree size) the contenders are timed alternately in one process, at the C ABI with
descriptors prepared once, so that what else the machine does falls on all alike and no front-end time is in the figures:
  (a)   fa_kvcache_decode_varlen_ex with a tree mask (random trees from fa.tree_from_parents) -- this build
  (b)   fa_kvcache_decode_varlen(causal = 1) on the same shape -- the PARENT commit's library
  (b')  (b) once more: the ratio (b') / (b) per round is the run's own A/A spread
  (b+)  fa_kvcache_decode_varlen(causal = 1) of this build (its kernels are the parent's, instruction for instruction)
  (c)   fa_kvcache_append_varlen_ex with positions against (c0) fa_kvcache_append_varlen: the extra 4-byte load per token (rotary,
        K and Q; only at the smaller key count -- the append does not depend on it)
The parent's library: in a checkout of the parent commit run `tools/build_variant.sh parent ""` and pass the lib_parent.so it
reports with --parent.
Workload: Hkv 8, G 4, fp16, causal, lengths = keys - 64 (the step's tokens included).
    python tools/tree_decode_bench.py [--d 64 128] [--rounds 5 --iters 20] [--forms contig paged] [--types f16 fp8] [--out FILE]
        --parent PATH
One line per contender: the median over the rounds of the time per call (device events around `iters` calls), the spread of the rounds,
the ratio of the medians to (b) with the spread of the per-round ratios.  Needs a GPU."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--forms", nargs="+", default=["contig", "paged"])
    ap.add_argument("--types", nargs="+", default=["f16", "fp8"])
    ap.add_argument("--keys", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--seqs", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--trees", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--page", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", required=True, help="libfa_mi355 built from the parent commit (tools/build_variant.sh in its checkout)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import flashattention_kernel_project_amd as fa
    from flashattention_kernel_project_amd import capi
    assert torch.cuda.is_available(), "tree_decode_bench needs a GPU"
    torch.manual_seed(0)
    Hkv, G = args.Hkv, args.G
    Hq = Hkv * G
    mine = fa.lib()
    parent = C.CDLL(os.path.abspath(args.parent))   # binds to the HIP runtime that is already in the process
    parent.fa_kvcache_decode_varlen.argtypes, parent.fa_kvcache_decode_varlen.restype = [C.POINTER(capi.KvDecodeVarlenDesc)], C.c_int
    assert not hasattr(parent, "fa_kvcache_decode_varlen_ex"), "--parent must be the PARENT commit's library"
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, base):
        for _, call in variants:   # warm-up: code objects, the LDS attribute, clocks
            for _ in range(5):
                assert call() == 0
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
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, times[base])]
            say(f"  {name:5s} {med:9.2f} us/call ({min(t):.2f} .. {max(t):.2f})  ratio to {base} {med / statistics.median(times[base]):.3f} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f})")

    say(f"Hkv{Hkv} G{G} fp16 causal rounds={args.rounds} iters={args.iters} page={args.page} parent={os.path.basename(args.parent)}")
    stream = torch.cuda.current_stream().cuda_stream
    for d in args.d:
        for Nk in args.keys:
            for B in args.seqs:
                for n in args.trees:
                    T = B * n
                    lens = torch.full((B,), Nk - 64, dtype=torch.int32, device="cuda")
                    before = lens - n
                    cu = torch.arange(0, T + 1, n, dtype=torch.int32, device="cuda")
                    rng = np.random.default_rng(B * 1000 + n)
                    par = np.concatenate([[-1] + [int(rng.integers(0, i)) for i in range(1, n)] for _ in range(B)]).astype(np.int32)
                    mask, depth = fa.tree_from_parents(torch.from_numpy(par).cuda(), cu)
                    pos = (depth + before.repeat_interleave(n)).contiguous()
                    fused = torch.randn(T, Hq + 2 * Hkv, d, device="cuda", dtype=torch.float16)
                    q = fused[:, :Hq]
                    out = torch.zeros(T, Hq, d, device="cuda", dtype=torch.float32)
                    half = d // 2
                    theta = torch.rand(Nk, half, device="cuda") * 6.2831853   # unit rotations: Q is rotated in place call after call
                    cos, sin = theta.cos(), theta.sin()
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
                            geo = dict(num_pages=shape[0], max_pages=Nk // args.page, page_size=args.page, block_table=table.data_ptr()) \
                                if table is not None else dict(Ncap=Nk)
                            wgeo = {x: y for x, y in geo.items() if x in ("max_pages", "page_size", "Ncap")}
                            need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, n, d, **wgeo)
                            ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
                            S = max(need // (B * Hkv * G * n * (d + 2) * 4), 1)
                            desc = capi.KvDecodeVarlenDesc(
                                Q=q.data_ptr(), O=out.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), cu_seqlens_q=cu.data_ptr(),
                                seqlens_k=lens.data_ptr(), kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT, B=B, Hkv=Hkv, G=G, d=d,
                                total_q=T, max_q=n, q_stride_t=q.stride(0), q_stride_h=q.stride(1), o_stride_t=out.stride(0),
                                o_stride_h=out.stride(1), scale=d ** -0.5, causal=1, in_dtype=0, out_dtype=0, workspace=ws.data_ptr(),
                                workspace_bytes=ws.numel(), stream=stream, **geo)
                            opts = capi.KvDecodeTreeOpts(tree_mask=mask.data_ptr())
                            run(f"d{d} {form} {typ} {B}x{n} over {Nk} keys (total_q={T} S={S})",
                                (("(b)", lambda: parent.fa_kvcache_decode_varlen(C.byref(desc))),
                                 ("(a)", lambda: mine.fa_kvcache_decode_varlen_ex(C.byref(desc), C.byref(opts))),
                                 ("(b+)", lambda: mine.fa_kvcache_decode_varlen(C.byref(desc))),
                                 ("(b')", lambda: parent.fa_kvcache_decode_varlen(C.byref(desc)))), "(b)")
                            if Nk == min(args.keys):
                                kn, vn = fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
                                ad = capi.KvAppendVarlenDesc(
                                    Knew=kn.data_ptr(), Vnew=vn.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), cu_seqlens_new=cu.data_ptr(),
                                    seqlens_k=before.data_ptr(), Q=q.data_ptr(), Qout=q.data_ptr(), rope_cos=cos.data_ptr(),
                                    rope_sin=sin.data_ptr(), kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT, B=B, Hkv=Hkv, d=d,
                                    total_new=T, G=G, rot_dim=d, max_pos=Nk, interleaved=0, dtype=0, k_stride_t=kn.stride(0),
                                    k_stride_h=kn.stride(1), v_stride_t=vn.stride(0), v_stride_h=vn.stride(1), q_stride_t=q.stride(0),
                                    q_stride_h=q.stride(1), qo_stride_t=q.stride(0), qo_stride_h=q.stride(1), stream=stream, **geo)
                                po = capi.KvAppendVarlenOpts(positions=pos.data_ptr())
                                run(f"d{d} {form} {typ} {B}x{n} append (total_new={T})",
                                    (("(c0)", lambda: mine.fa_kvcache_append_varlen(C.byref(ad))),
                                     ("(c)", lambda: mine.fa_kvcache_append_varlen_ex(C.byref(ad), C.byref(po))),
                                     ("(c0')", lambda: mine.fa_kvcache_append_varlen(C.byref(ad)))), "(c0)")
                            del k, v, ws
                    torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
