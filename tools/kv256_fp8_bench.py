#!/usr/bin/env python3
"""What fa_kvcache_decode_d256_fp8 and fa_kvcache_append_varlen_d256 cost (profiles/kv256_fp8.txt).  The contenders of a row are timed
alternately in one process, so that what else the machine does falls on all alike.
Decode, per (dtype, cache form, G, B, L, options), Hkv = 8, one token per sequence, causal, the library's split count:
  fp8      (a) fa_kvcache_decode_d256_fp8 on the e4m3fn cache (quantize_kv_fp8 of the 16-bit one, per-head scales)
  fp8'     the same call once more: fp8' / fp8 per round is the run's own A/A spread
  d256     (b) fa_kvcache_decode_d256 on the 16-bit cache of the same keys: the bandwidth yardstick
  widen    (c) cache.to(dtype) and then fa_kvcache_decode_d256: the only route to an fp8 d = 256 cache before this entry
Append, per (dtype, cache element, shape, rotary): the new entry against torch index_copy_ with prebuilt indices (for an fp8 cache:
quantize_kv_fp8 and then that scatter), the route there was; neither torch route rotates.
    python tools/kv256_fp8_bench.py [--G 2 4 8] [--B 8 64] [--L 4096 32768] [--types f16 bf16] [--forms contig paged]
                                    [--opts plain gemma] [--rounds 5 --iters 10] [--out FILE]
One line per contender: the median over the rounds of the time per call (device events around `iters` calls), the spread of the
rounds, the ratio to the row's first contender, and for the decode the rate at which the call's own K+V bytes stream.
"gemma" is W = 4096 with softcap 50.  Needs a GPU."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, PAGE, HKV = 256, 16, 8
OPTS = {"plain": (0, 0.0), "gemma": (4096, 50.0)}


def main():
    ap = argparse.ArgumentParser()
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
    assert torch.cuda.is_available(), "kv256_fp8_bench needs a GPU"
    torch.manual_seed(0)
    sink = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(title, variants, nbytes=None):
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
            rate = f"  {nbytes[name] / med * 1e-6:6.2f} TB/s of its K+V" if nbytes else ""
            say(f"  {name:6s} {med:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  x{med / statistics.median(base):.3f} of {variants[0][0]} "
                f"(per round {min(ratios):.3f} .. {max(ratios):.3f}){rate}")

    say(f"d = 256 on an fp8 cache, Hkv={HKV}, rounds={args.rounds} iters={args.iters} page={PAGE} ({fa.version()})")
    say("== append: fa_kvcache_append_varlen_d256[_fp8] against torch index_copy_ (fp8: quantize_kv_fp8 first)")
    for typ in args.types:
        tdt = torch.float16 if typ == "f16" else torch.bfloat16
        for nb, m in ((16, 512), (256, 1)):
            T, ncap = nb * m, 1024
            kn, vn = (torch.randn(T, HKV, D, device="cuda", dtype=tdt) for _ in range(2))
            qn = torch.randn(T, HKV * 2, D, device="cuda", dtype=tdt)
            cu = torch.arange(nb + 1, dtype=torch.int32, device="cuda") * m
            lens = torch.full((nb,), 256, dtype=torch.int32, device="cuda")
            cos, sin = (torch.rand(ncap, D // 2, device="cuda") for _ in range(2))
            # the scatter's prebuilt row indices into the cache seen as [B * Hkv * Ncap] rows, head by head
            bi, ti = torch.arange(nb, device="cuda").repeat_interleave(m), torch.arange(m, device="cuda").repeat(nb)
            idx = torch.stack([(bi * HKV + h) * ncap + 256 + ti for h in range(HKV)]).view(-1).long()
            for fp8 in (False, True):
                kc, vc = (torch.zeros(nb, HKV, ncap, D, device="cuda", dtype=torch.float8_e4m3fn if fp8 else tdt) for _ in range(2))
                ks, vs = (torch.full((HKV,), 0.01, device="cuda") for _ in range(2))

                def ours(rope=False):
                    kw = dict(q=qn, rotary_cos=cos, rotary_sin=sin) if rope else {}
                    if fp8:
                        return fa.fa_kvcache_append_varlen_d256_fp8(kn, vn, kc, vc, cu, lens, None, None, ks, vs, **kw)
                    return fa.fa_kvcache_append_varlen_d256(kn, vn, kc, vc, cu, lens, None, None, **kw)

                def torch_route():
                    for dst, src, sc in ((kc, kn, ks), (vc, vn, vs)):
                        rows = src.transpose(0, 1)   # [Hkv, T, D]
                        if fp8:
                            rows = fa.quantize_kv_fp8(rows.unsqueeze(0), sc)[0][0].view(torch.uint8)
                        dst.view(torch.uint8 if fp8 else tdt).view(-1, D).index_copy_(0, idx, rows.reshape(-1, D))

                run(f"{typ} {'fp8' if fp8 else '16-bit'} cache, {nb} x {m} tokens",
                    [("ours", ours), ("ours'", ours), ("rotary", lambda: ours(True)), ("torch", torch_route)])
    say("== decode: one token per sequence, causal")
    for typ in args.types:
        tdt = torch.float16 if typ == "f16" else torch.bfloat16
        for form in args.forms:
            for B in args.B:
                for L in args.L:
                    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
                    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
                    k, v = (torch.randn(B, HKV, L, D, device="cuda", dtype=tdt) for _ in range(2))
                    table, geo = None, dict(Ncap=L)
                    if form == "paged":
                        pages = B * L // PAGE
                        table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, L // PAGE)
                        k, v = (x.view(B, HKV, L // PAGE, PAGE, D).transpose(1, 2).reshape(pages, HKV, PAGE, D) for x in (k, v))
                        geo = dict(max_pages=L // PAGE, page_size=PAGE)
                    (k8, ks), (v8, vs) = fa.quantize_kv_fp8(k), fa.quantize_kv_fp8(v)
                    for G in args.G:
                        q = torch.randn(B, HKV * G, D, device="cuda", dtype=tdt)
                        out = torch.empty_like(q)
                        for opt in args.opts:
                            W, cap = OPTS[opt]
                            ws = torch.empty(max(fa.kvcache_decode_d256_fp8_workspace_bytes(B, HKV, G, 1, window=W, **geo), 1),
                                             dtype=torch.uint8, device="cuda")
                            kw = dict(cache_seqlens=lens, block_table=table, causal=True, window=W, softcap=cap, out=out, workspace=ws)

                            def a_fp8(q=q, kw=kw):
                                return fa.fa_kvcache_decode_d256_fp8(q, k8, v8, cu, 1, k_scale=ks, v_scale=vs, **kw)

                            def b_16(q=q, kw=kw):
                                return fa.fa_kvcache_decode_d256(q, k, v, cu, 1, **kw)

                            def c_widen(q=q, kw=kw):
                                return fa.fa_kvcache_decode_d256(q, k8.to(tdt), v8.to(tdt), cu, 1, **kw)

                            keys = min(L, W) if W else L
                            byt = 2.0 * B * HKV * keys * D
                            run(f"{typ} {form} G{G} B{B} L{L} {opt} ({2 * byt / 2 ** 30:.2f} GiB of 16-bit K+V)",
                                [("fp8", a_fp8), ("fp8'", a_fp8), ("d256", b_16), ("widen", c_widen)],
                                {"fp8": byt, "fp8'": byt, "d256": 2 * byt, "widen": 2 * byt})
                    del k, v, k8, v8
                    torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
