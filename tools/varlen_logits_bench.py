#!/usr/bin/env python3
"""fa_forward_varlen_ex (sliding window, soft-cap, sinks) against the un-windowed call of the same build
(profiles/varlen_logits.txt).  A causal self-attention prefill of B prompts, Hkv K/V heads, fp16, 16-bit output, in two model-like
configurations:
  gptoss   d 64, G 8, W 128 plus sinks
  gemma2   d 128, G 4, W 4096 plus a soft-cap of 50
The protocol is tools/varlen_bench.py's: a group's variants alternate in one process, the median over `rounds` of the time per call
(device events around `iters` calls), the spread of the rounds, and the ratio to the group's first variant with the spread of the
per-round ratios.  Variants:
  fa_forward_varlen                        the base entry: no window, plain kernels
  ex: W huge (no option acts)              the kLogits kernels with nothing to do: what the runtime switches themselves cost
  ex: window                               the window alone: the tile skip
  ex: cap | ex: sinks                      the configuration's second option alone, un-windowed: on/off against "W huge"
  ex: window + cap | window + sinks        the configuration
  parent: fa_forward_varlen                (with --parent-lib) the same descriptor through another build's fa_forward_varlen
TFLOP/s are over the VISIBLE query-key pairs of each variant, 4 d flops each; "pairs" is the ratio of the windowed to the
un-windowed pair count, which the time ratio of a perfect tile skip would equal.
    python tools/varlen_logits_bench.py [--configs gptoss gemma2] [--batches long skewed uniform short] [--parent-lib PATH]
Needs a GPU."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"gptoss": dict(d=64, G=8, W=128, softcap=0.0, sinks=True), "gemma2": dict(d=128, G=4, W=4096, softcap=50.0, sinks=False)}
HUGE = 1 << 30


def lengths(name):
    """long: 4 x 16384; skewed, uniform, short: tools/varlen_bench.py's (one 8192 plus fifteen of 128..1024; 16 x 2048; 256 x 64)"""
    if name == "long":
        return [16384] * 4
    if name == "uniform":
        return [2048] * 16
    if name == "short":
        return [64] * 256
    import random
    rng = random.Random(3)
    return [8192] + [rng.randrange(128, 1025) for _ in range(15)]


def pairs(lens, W):
    """visible (q, k) pairs of causal self-attention under a window of W (0: none)"""
    return sum(n * (n + 1) // 2 if not W or n <= W else W * (W + 1) // 2 + (n - W) * W for n in lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["gptoss", "gemma2"], choices=sorted(CONFIGS))
    ap.add_argument("--batches", nargs="+", default=["long", "skewed"])
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="another build of libfa_mi355.so: its fa_forward_varlen joins every group")
    args = ap.parse_args()
    import torch
    import flashattention_kernel_project_amd as fa
    from flashattention_kernel_project_amd import capi
    assert torch.cuda.is_available(), "varlen_logits_bench needs a GPU"
    torch.manual_seed(0)
    f16 = torch.float16
    parent = None
    if args.parent_lib:
        fa.lib()                      # the HIP runtime both libraries share is in the process first
        parent = ctypes.CDLL(args.parent_lib)
        parent.fa_forward_varlen.restype, parent.fa_forward_varlen.argtypes = ctypes.c_int, [ctypes.POINTER(capi.VarlenDesc)]

    def run(title, variants):
        for _, call, _ in variants:   # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, call, _ in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        print(title)
        base = times[variants[0][0]]
        for name, _, flops in variants:
            t = times[name]
            med = statistics.median(t)
            ratios = [x / y for x, y in zip(t, base)]
            print(f"  {name:40s} {med:10.2f} us/call ({min(t):.2f} .. {max(t):.2f})  {flops / med / 1e6:7.1f} TFLOP/s visible  "
                  f"ratio to the first {med / statistics.median(base):.3f} (per round {min(ratios):.3f} .. {max(ratios):.3f})")

    for name in args.configs:
        cfg = CONFIGS[name]
        d, G, W, cap = cfg["d"], cfg["G"], cfg["W"], cfg["softcap"]
        Hkv, Hq = args.Hkv, args.Hkv * G
        sinks = torch.linspace(-1.0, 2.0, Hq, device="cuda", dtype=torch.float32) if cfg["sinks"] else None
        for batch in args.batches:
            lens = lengths(batch)
            B, total = len(lens), sum(lens)
            cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(B)], dtype=torch.int32, device="cuda")
            q = torch.randn(total, Hq, d, device="cuda", dtype=f16)
            k = torch.randn(total, Hkv, d, device="cuda", dtype=f16)
            v = torch.randn(total, Hkv, d, device="cuda", dtype=f16)
            out = torch.empty_like(q)
            full, win = 4.0 * d * Hq * pairs(lens, 0), 4.0 * d * Hq * pairs(lens, W)

            def call(**kw):
                return lambda: fa.fa_forward_varlen(q, k, v, cu, causal=True, out=out, **kw)

            second = dict(softcap=cap) if cap else dict(sinks=sinks)
            what = "cap" if cap else "sinks"
            variants = [("fa_forward_varlen", call(), full), ("ex: W huge (no option acts)", call(window=HUGE), full),
                        ("ex: window", call(window=W), win), (f"ex: {what}", call(**second), full),
                        (f"ex: window + {what}", call(window=W, **second), win)]
            if parent is not None:
                desc = capi.VarlenDesc(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=out.data_ptr(), lse=None,
                                       cu_seqlens_q=cu.data_ptr(), cu_seqlens_k=cu.data_ptr(), B=B, Hkv=Hkv, G=G, d=d, total_q=total,
                                       total_k=total, q_stride_t=Hq * d, q_stride_h=d, k_stride_t=Hkv * d, k_stride_h=d,
                                       v_stride_t=Hkv * d, v_stride_h=d, o_stride_t=Hq * d, o_stride_h=d, scale=d ** -0.5, causal=1,
                                       in_dtype=capi.F16, out_dtype=capi.OUT_SAME, stream=torch.cuda.current_stream().cuda_stream)
                mine = fa.lib().fa_forward_varlen

                def through(fn):
                    def go():
                        assert fn(ctypes.byref(desc)) == 0
                    return go

                # the same raw call through both builds, so that the front end's cost falls on neither
                variants = [("this build: fa_forward_varlen (raw)", through(mine), full),
                            ("parent: fa_forward_varlen (raw)", through(parent.fa_forward_varlen), full)] + variants[1:]
            print(f"    {name} on {batch}: visible pairs windowed / un-windowed = {pairs(lens, W) / pairs(lens, 0):.4f}")
            run(f"{name} {batch}: B{B} lengths {min(lens)}..{max(lens)} total {total} Hkv{Hkv} G{G} d{d} W{W} fp16 causal, 16-bit out, "
                f"rounds={args.rounds} iters={args.iters}", variants)
            del q, k, v, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
