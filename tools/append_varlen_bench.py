#!/usr/bin/env python3
"""The packed append (fa_kvcache_append_varlen) against the only route there was before it, and against the padded entry alone.

    python tools/append_varlen_bench.py                     # Hkv 8, G 4, d 128 and 64, three batches, the four cache forms, +- rotary
    python tools/append_varlen_bench.py --alt-lib PATH      # a second build of the library (the other thread order,
                                                            # -DFA_APPEND_VARLEN_ORDER=1) as one more contender

Method and verdict of tools/append_bench.py: the contenders of one row run in one process, interleaved round by round, 5 rounds of 50
launches each between two device events; a line gives the median of the rounds and their range; the entry is "not slower" when its
median is at most the baseline's median plus the baseline's round-to-round spread (max - min of its rounds).  Before the timing every
contender runs once on fresh state and the results are compared byte for byte: caches or pools, seqlens_out and the rotated Q rows.

The sources are views of ONE fused (total, Hq + 2 Hkv, d) bf16 buffer, as a QKV projection leaves them.  Contenders:
  varlen      (a) fa_kvcache_append_varlen on the views, Q rotated in place inside the buffer; nothing is read on the host
  pad+entry   (b) the route before: the lengths are KNOWN ON THE HOST; K, V (and Q) are padded to max(m_b) and made head-major by torch
              -- one reshape + transpose copy when the lengths are equal, one gather through a precomputed index otherwise -- then
              fa_kvcache_append_ex(seqlens_new = m); with rotary the rotated Q is gathered back into a packed tensor for the prefill
  padded      (c) the padded entry alone on data that already lies padded and head-major: context and a floor, not a bar
  varlen-pk   (a) on contiguous packed copies (total, H, d) of the same rows: what of (a)'s distance to (c) the strided views cost
  alt         (--alt-lib) (a) through the other build, called through ctypes directly: no Python front end, which shows on rows that
              the host call bounds
Batches: 16 x 512 tokens; one 8192 plus fifteen of 128 .. 1024; 256 x 1.  Every sequence holds 1024 keys before the append.
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.append_bench import timed_rounds   # noqa: E402

BATCHES = {
    "16x512": [512] * 16,
    "8192+15": [8192] + [128 + 64 * i for i in range(15)],   # 128, 192, ... 1024
    "256x1": [1] * 256,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--d", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--batches", nargs="+", default=list(BATCHES))
    ap.add_argument("--layouts", nargs="+", default=["contiguous", "paged", "fp8", "paged_fp8"])
    ap.add_argument("--len", type=int, default=1024, dest="L", help="keys every sequence holds before the append")
    ap.add_argument("--page", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alt-lib", default=None, help="another build of libfa_mi355.so, timed as one more contender")
    args = ap.parse_args()

    import torch
    import flashattention_kernel_project_amd as fa
    from flashattention_kernel_project_amd import capi

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, bf16 = "cuda", torch.bfloat16
    Hkv, G, L, ps = args.Hkv, args.G, args.L, args.page
    Hq = Hkv * G
    fa.lib()   # the shared HIP runtime first
    alt = ctypes.CDLL(args.alt_lib) if args.alt_lib else None
    print(f"{fa.version()}; Hkv{Hkv} G{G}, length {L} before the append, pages of {ps}; median of {args.rounds} rounds of {args.iters} "
          f"launches; alt = {args.alt_lib}")
    gen = torch.Generator(device="cpu").manual_seed(0)

    for d in args.d:
        ang = torch.arange(1 << 15, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, d, 2, dtype=torch.float64) / d))[None]
        cos, sin = ang.cos().float().to(dev).contiguous(), ang.sin().float().to(dev).contiguous()
        for batch in args.batches:
            m = BATCHES[batch]
            B, total, nmax = len(m), sum(m), max(m)
            Ncap = 1 << (L + nmax - 1).bit_length()
            max_pages = Ncap // ps
            cu_host = [0]
            for x in m:
                cu_host.append(cu_host[-1] + x)
            cu = torch.tensor(cu_host, dtype=torch.int32, device=dev)
            m_dev = torch.tensor(m, dtype=torch.int32, device=dev)
            lens = torch.full((B,), L, dtype=torch.int32, device=dev)
            lens_out = {n: torch.zeros(B, dtype=torch.int32, device=dev) for n in ("varlen", "pad+entry", "padded", "varlen-pk", "alt")}
            table = torch.randperm(B * max_pages, generator=gen).to(dev).view(B, max_pages).to(torch.int32).contiguous()
            k_scale = torch.rand(Hkv, device=dev) * 0.02 + 0.005
            v_scale = torch.rand(Hkv, device=dev) * 0.02 + 0.005
            source = torch.randn(total, Hq + 2 * Hkv, d, device=dev).to(bf16)
            uniform = len(set(m)) == 1
            # (b)'s indices, from the host-known lengths: padded slot -> token row (padding reads row 0), and token row -> padded slot
            slot_rows = torch.zeros(B, nmax, dtype=torch.long)
            row_slots = torch.empty(total, dtype=torch.long)
            for b, x in enumerate(m):
                slot_rows[b, :x] = torch.arange(cu_host[b], cu_host[b] + x)
                row_slots[cu_host[b]:cu_host[b] + x] = b * nmax + torch.arange(x)
            slot_rows, row_slots = slot_rows.to(dev), row_slots.to(dev)

            def pad(x):   # packed view (total, H, d) -> padded head-major [B, H, nmax, d], contiguous
                if uniform:
                    return x.reshape(B, nmax, x.shape[1], d).transpose(1, 2).contiguous()
                return x[slot_rows].transpose(1, 2).contiguous()

            for layout in args.layouts:
                paged, fp8 = "paged" in layout, "fp8" in layout
                cdt = torch.float8_e4m3fn if fp8 else bf16
                shape = (B * max_pages, Hkv, ps, d) if paged else (B, Hkv, Ncap, d)
                padded_fn = {(False, False): fa.fa_kvcache_append, (True, False): fa.fa_kvcache_append_paged,
                             (False, True): fa.fa_kvcache_append_fp8, (True, True): fa.fa_kvcache_append_paged_fp8}[paged, fp8]
                varlen_fn = fa.fa_kvcache_append_varlen_fp8 if fp8 else fa.fa_kvcache_append_varlen
                extra = ((table,) if paged else ()) + ((k_scale, v_scale) if fp8 else ())
                tbl = table if paged else None
                names = ["varlen", "pad+entry", "padded", "varlen-pk"] + (["alt"] if alt else [])
                caches = {n: [torch.zeros(shape, dtype=torch.uint8 if fp8 else cdt, device=dev).view(cdt) for _ in range(2)] for n in names}
                for rope in (False, True):
                    fused = {n: source.clone() for n in ("varlen", "pad+entry", "alt")}
                    views = {n: (f[:, :Hq], f[:, Hq:Hq + Hkv], f[:, Hq + Hkv:]) for n, f in fused.items()}
                    ready = [pad(x) for x in views["pad+entry"]]       # (c)'s sources: already padded
                    views["varlen-pk"] = tuple(x.contiguous() for x in views["pad+entry"])
                    state = {}

                    def varlen(name="varlen"):
                        q, k, v = views[name]
                        kw = dict(q=q, rotary_cos=cos, rotary_sin=sin) if rope else {}
                        varlen_fn(k, v, *caches[name], cu, lens, lens_out[name], tbl, *((k_scale, v_scale) if fp8 else ()), **kw)

                    def pad_entry():
                        q, k, v = views["pad+entry"]
                        kw = {}
                        if rope:
                            qp = pad(q)
                            kw = dict(q=qp, rotary_cos=cos, rotary_sin=sin)
                        padded_fn(pad(k), pad(v), *caches["pad+entry"], *extra, cache_seqlens=lens, seqlens_out=lens_out["pad+entry"],
                                  seqlens_new=m_dev, **kw)
                        if rope:   # back to the packed layout the prefill reads
                            qt = qp.transpose(1, 2)
                            state["q"] = qt.reshape(total, Hq, d) if uniform else qt.reshape(B * nmax, Hq, d)[row_slots]

                    def padded():
                        kw = dict(q=state["qready"], rotary_cos=cos, rotary_sin=sin) if rope else {}
                        padded_fn(ready[1], ready[2], *caches["padded"], *extra, cache_seqlens=lens, seqlens_out=lens_out["padded"],
                                  seqlens_new=m_dev, **kw)

                    def alt_call():
                        q, k, v = views["alt"]
                        vp = lambda t: None if t is None else t.data_ptr()
                        desc = capi.KvAppendVarlenDesc(
                            Knew=vp(k), Vnew=vp(v), K=vp(caches["alt"][0]), V=vp(caches["alt"][1]), cu_seqlens_new=vp(cu), seqlens_k=vp(lens),
                            seqlens_out=vp(lens_out["alt"]), block_table=vp(tbl), k_scale=vp(k_scale) if fp8 else None,
                            v_scale=vp(v_scale) if fp8 else None, Q=vp(q) if rope else None, Qout=vp(q) if rope else None,
                            rope_cos=vp(cos) if rope else None, rope_sin=vp(sin) if rope else None, kv_dtype=1 if fp8 else 0, B=B, Hkv=Hkv,
                            d=d, total_new=total, Ncap=0 if paged else Ncap, num_pages=shape[0] if paged else 0, page_size=ps if paged else 0,
                            max_pages=max_pages if paged else 0, G=G if rope else 0, rot_dim=d if rope else 0,
                            max_pos=cos.shape[0] if rope else 0, interleaved=0, dtype=1, k_stride_t=k.stride(0), k_stride_h=k.stride(1),
                            v_stride_t=v.stride(0), v_stride_h=v.stride(1), q_stride_t=q.stride(0), q_stride_h=q.stride(1),
                            qo_stride_t=q.stride(0), qo_stride_h=q.stride(1), stream=torch.cuda.current_stream().cuda_stream)
                        code = alt.fa_kvcache_append_varlen(ctypes.byref(desc))
                        assert code == 0, code

                    calls = {"varlen": varlen, "pad+entry": pad_entry, "padded": padded, "varlen-pk": lambda: varlen("varlen-pk")}
                    if alt:
                        calls["alt"] = alt_call
                    tag = f"d{d} {batch:8s} {layout:10s} {'rope ' if rope else 'plain'}"
                    # ---- once on fresh state: the bytes --------------------------------------------------------------------------------
                    for pair in caches.values():
                        for c in pair:
                            c.view(torch.uint8).zero_()
                    state["qready"] = ready[0].clone()
                    for f in calls.values():
                        f()
                    torch.cuda.synchronize()
                    raw = {n: [c.view(torch.uint8) for c in caches[n]] for n in calls}
                    for n in calls:
                        assert all(torch.equal(x, y) for x, y in zip(raw[n], raw["varlen"])), f"{tag}: {n} and varlen wrote different caches"
                        assert torch.equal(lens_out[n], lens_out["varlen"]), f"{tag}: {n} lengths"
                    assert int(torch.count_nonzero(raw["varlen"][0])) > 0 and lens_out["varlen"].tolist() == [L + x for x in m]
                    if rope:
                        q16 = views["varlen"][0].contiguous().view(torch.int16)
                        assert torch.equal(q16, state["q"].contiguous().view(torch.int16)), f"{tag}: rotated Q differs from pad+entry's"
                        assert not torch.equal(q16, source[:, :Hq].contiguous().view(torch.int16))
                        if alt:
                            assert torch.equal(q16, views["alt"][0].contiguous().view(torch.int16)), f"{tag}: rotated Q differs from alt's"
                    # ---- the timing ----------------------------------------------------------------------------------------------------
                    for f in calls.values():
                        for _ in range(3):
                            f()
                    torch.cuda.synchronize()
                    times = timed_rounds(calls, args.rounds, args.iters)
                    med = {n: statistics.median(t) for n, t in times.items()}
                    moved = 2.0 * total * Hkv * d * (2 + (1 if fp8 else 2)) + (4.0 * total * Hq * d if rope else 0.0)
                    for n in calls:
                        rate = f", {moved / med[n] / 1e6:6.0f} GB/s over {moved / 1e6:.1f} MB read + written" if n in ("varlen", "alt", "padded", "varlen-pk") \
                            and total >= 1024 else ""
                        print(f"{tag} [{n:9s}]: median {med[n] * 1e3:8.1f} us (rounds {min(times[n]) * 1e3:.1f}-{max(times[n]) * 1e3:.1f}){rate}")
                    spread_b = max(times["pad+entry"]) - min(times["pad+entry"])
                    spread_c = max(times["padded"]) - min(times["padded"])
                    ok = med["varlen"] <= med["pad+entry"] + spread_b
                    vs_c = "within" if med["varlen"] <= med["padded"] + spread_c else "BEYOND"
                    line = (f"{tag}: varlen / pad+entry = {med['varlen'] / med['pad+entry']:.3f} (spread {spread_b * 1e3:.1f} us): "
                            f"{'not slower' if ok else 'SLOWER beyond the spread'}; varlen / padded = {med['varlen'] / med['padded']:.3f} "
                            f"({vs_c} padded's spread of {spread_c * 1e3:.1f} us)")
                    line += f"; varlen-pk / padded = {med['varlen-pk'] / med['padded']:.3f}"
                    if alt:
                        line += f"; alt / varlen = {med['alt'] / med['varlen']:.3f}"
                    print(line, flush=True)
                    del fused, views, ready, state
                del caches
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
