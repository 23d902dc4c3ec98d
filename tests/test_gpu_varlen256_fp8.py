"""GPU tier of fa_forward_varlen_kvcache_d256_fp8, on the batch of tests/test_gpu_varlen256.py (imported) with caches quantised by
quantize_kv_fp8.  The float64 reference sees decode(codes) * scale[h], so fp8 adds no error term and the bounds are dv.check's.  Every
row and page nothing may read holds the NaN code 0x7F, dead table entries garbage, Q rows of no sequence NaN, O and lse sentinels."""
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv
import fp8_inputs as f8
import test_gpu_varlen256 as base
from test_gpu_varlen256 import torch_cuda   # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

D, NCAP, B, LQ, LENS, MAXQ, LAY, SEEN = base.D, base.NCAP, base.B, base.LQ, base.LENS, base.MAXQ, base.LAY, base.SEEN
NAN8 = f8.NAN_CODES[0]
# (fmt, 16-bit output, Hkv, G, causal, W, softcap, page size or 0, per-head scales): a pruned product
CASES = [
    (0, False, 2, 4, True, 0, 0.0, 0, True), (1, False, 2, 4, True, 0, 0.0, 16, False), (0, True, 1, 8, True, 17, 0.0, 64, True),
    (1, True, 1, 8, False, 100, 0.0, 0, True), (0, False, 1, 1, False, 0, 30.0, 128, False), (1, False, 1, 1, True, 400, 30.0, 0, True),
    (0, False, 1, 8, True, 100, 30.0, 16, True), (1, True, 2, 4, True, 1, 30.0, 64, False), (0, True, 2, 4, False, 17, 0.0, 128, True),
    (1, False, 1, 8, True, 1, 0.0, 16, True),
]


@functools.lru_cache(maxsize=None)
def _quantised(fa, oracle, fmt, Hkv, G, scaled):
    import torch   # -> (q fp32, q bits, K codes, V codes [B, Hkv, NCAP, D] uint8, k_scale, v_scale [Hkv] fp32)
    (q, k, v), (qb, _, _) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2570 + Hkv)
    (k8, ks), (v8, vs) = (fa.quantize_kv_fp8(torch.from_numpy(x.reshape(B, Hkv, NCAP, D).copy()), None if scaled else torch.ones(Hkv))
                          for x in (k, v))
    return q, qb, k8.view(torch.uint8).numpy(), v8.view(torch.uint8).numpy(), ks.numpy(), vs.numpy()


@functools.lru_cache(maxsize=None)
def _reference(fa, oracle, fmt, Hkv, G, causal, W, softcap, scaled, zeroed=()):
    q, _, kc, vc, ks, vs = _quantised(fa, oracle, fmt, Hkv, G, scaled)
    k, v = ((f8.decode(c).astype(np.float64) * s[None, :, None, None]).reshape(B * Hkv, NCAP, D) for c, s in ((kc, ks), (vc, vs)))
    for b, j0, j1 in zeroed:
        k[b * Hkv:(b + 1) * Hkv, j0:j1] = v[b * Hkv:(b + 1) * Hkv, j0:j1] = 0.0
    return cm.expected_f64(q, k, v, LENS, B, Hkv, G, MAXQ, causal, W, scale=base.SOFTCAP_SCALE if softcap else None, softcap=softcap, nq=LQ)


def _run(fa, torch, qb, kc, vc, fmt, Hkv, G, causal, W, softcap, ps, out16=False, scales=(None, None), table_edit=None, wide=False,
         scale=None):
    """one call on sentinel-filled O and lse -> (O, lse); kc, vc: codes; wide: fa_forward_varlen_kvcache_d256 on the widened cache"""
    kc, vc = (np.concatenate([cm.poisoned(x[b:b + 1], SEEN[b:b + 1], max(LQ[b], 1), W, nan=NAN8) for b in range(B)]) for x in (kc, vc))
    q = cm.dev16(torch, dv.pack_rows(LAY, qb, cm.NAN16), fmt)
    bits, sent = (torch.int16, dv.SENTINEL_O16) if out16 else (torch.int32, dv.SENTINEL_O32)
    out = torch.empty((LAY.total_q, Hkv * G, D), dtype=q.dtype if out16 else torch.float32, device="cuda")
    out.view(bits).fill_(sent)
    lse = torch.full((Hkv * G, LAY.total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    table = None
    if ps:   # cm.scatter sequence by sequence (each has its own row count, hence its own lo_0), the pools stacked, the tables offset
        parts, n0 = [], 0
        for b in range(B):
            kp, vp, tb = cm.scatter(kc[b:b + 1], vc[b:b + 1], SEEN[b:b + 1], ps, 7 + ps + b, max(LQ[b], 1), W, nan=NAN8, spare=1)
            parts.append((kp, vp, np.where((tb != cm.GARBAGE[0]) & (tb != cm.GARBAGE[1]), tb + n0, tb)))
            n0 += kp.shape[0]
        kc, vc, tb = (np.concatenate([p[i] for p in parts]) for i in range(3))
        if table_edit:
            table_edit(tb, n0)
        table = torch.from_numpy(tb.astype(np.int32)).cuda()
    k8, v8 = cm.dev8(torch, kc), cm.dev8(torch, vc)
    args = (torch.from_numpy(LAY.cu).cuda(), torch.tensor(LENS, dtype=torch.int32, device="cuda"))
    kw = dict(block_table=table, causal=causal, window=W, softcap=softcap, out=out, lse=lse,
              scale=scale if scale is not None else base.SOFTCAP_SCALE if softcap else None)
    if wide:
        fa.fa_forward_varlen_kvcache_d256(q, k8.to(q.dtype), v8.to(q.dtype), *args, **kw)
    else:
        ks, vs = (None if s is None else torch.from_numpy(np.asarray(s, np.float32)).cuda() for s in scales)
        fa.fa_forward_varlen_kvcache_d256_fp8(q, k8, v8, *args, k_scale=ks, v_scale=vs, **kw)
    torch.cuda.synchronize()
    free = torch.from_numpy(~LAY.owned).cuda()
    assert (out[free].contiguous().view(bits) == sent).all() and (lse[:, free] == dv.SENTINEL_LSE).all(), "a token of no sequence was written"
    return out, lse


@pytest.mark.parametrize("fmt,out16,Hkv,G,causal,W,softcap,ps,scaled", CASES)
def test_against_float64(fa, oracle, torch_cuda, fmt, out16, Hkv, G, causal, W, softcap, ps, scaled):
    _, qb, kc, vc, ks, vs = _quantised(fa, oracle, fmt, Hkv, G, scaled)
    out, lse = _run(fa, torch_cuda, qb, kc, vc, fmt, Hkv, G, causal, W, softcap, ps, out16, (ks, vs) if scaled else (None, None))
    base._check(oracle, out, lse, _reference(fa, oracle, fmt, Hkv, G, causal, W, softcap, scaled), fmt,
                f"{cm.FMT_NAME[fmt]} out16={out16} Hkv={Hkv} G={G} causal={causal} W={W} softcap={softcap} pages={ps} scaled={scaled}")


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("W", [0, 100])
def test_bits_of_the_16_bit_entry(fa, oracle, torch_cuda, fmt, W):
    """all 254 finite codes, causal: null scales give the 16-bit entry's bits on the widened cache, k_scale = 2^-3 and v_scale = 2^2
    its bits at scale / 8, times 4, and pages of 16 the contiguous bits"""
    torch, Hkv, G = torch_cuda, 2, 4
    _, (qb, _, _) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2570 + Hkv)
    kc, vc = (f8.all_codes_cache(B, Hkv, NCAP, D, LENS, seed) for seed in (811, 812))
    run = functools.partial(_run, fa, torch, qb, kc, vc, fmt, Hkv, G, True, W, 0.0)
    sc = 2.0 ** -10   # the codes reach 448: logits of a few units
    own = torch.from_numpy(LAY.owned).cuda()   # the other tokens hold the sentinel, a NaN pattern
    want, want2 = run(0, wide=True, scale=sc), run(0, wide=True, scale=sc / 8)
    for ps in (0, 16):
        got = run(ps, scale=sc)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), f"null scales, pages {ps}"
        got = run(ps, scale=sc, scales=([0.125] * Hkv, [4.0] * Hkv))
        assert torch.equal(got[0][own], want2[0][own] * 4) and torch.equal(got[1], want2[1]), f"power-of-two scales, pages {ps}"


@pytest.mark.parametrize("bad", [-1, None])
def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda, bad):
    """entries -1 / num_pages in the place of the live pages 3 of sequence 1 and 0 of sequence 5: the bits of the call on the good
    table with those pages' codes zeroed, and the float64 reference with those K and V rows zeroed"""
    _, qb, kc, vc, ks, vs = _quantised(fa, oracle, 0, 2, 4, True)
    kz, vz = kc.copy(), vc.copy()
    kz[1, :, 48:64] = vz[1, :, 48:64] = kz[5, :, 0:16] = vz[5, :, 0:16] = 0
    run = lambda k, v, edit: _run(fa, torch_cuda, qb, k, v, 0, 2, 4, True, 0, 0.0, 16, scales=(ks, vs), table_edit=edit)   # noqa: E731
    out, lse = run(kc, vc, lambda tb, n: tb.__setitem__(([1, 5], [3, 0]), n if bad is None else bad))
    want = run(kz, vz, None)
    assert torch_cuda.equal(out.view(torch_cuda.int32), want[0].view(torch_cuda.int32)) and torch_cuda.equal(lse, want[1]), bad
    base._check(oracle, out, lse, _reference(fa, oracle, 0, 2, 4, True, 0, 0.0, True, ((1, 48, 64), (5, 0, 16))), 0, f"bad page {bad}")


def test_captured_append_then_prefill(fa, oracle, torch_cuda):
    """append_varlen_d256_fp8 -> the entry on pages of 16, captured once, replayed after cu_seqlens, lengths, table and scales are
    rewritten in place: against float64 on the codes the pool then holds, and on sequences of <= 32 rows against the fp8 decode"""
    torch = torch_cuda
    Hkv, G, ps, T, nb, MQ = 2, 4, 16, 200, 2, 192
    Hq, max_pages = Hkv * G, NCAP // ps
    num_pages = nb * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(2568)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen).to(torch.float16)   # noqa: E731
    ints = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")   # noqa: E731
    q, kn, vn = rnd(T, Hq, D), rnd(T, Hkv, D), rnd(T, Hkv, D)
    (kp, ks), (vp, vs) = (fa.quantize_kv_fp8(rnd(num_pages, Hkv, ps, D)) for _ in range(2))
    cu, lens, after = ints([0, 100, 200]), ints([200, 100]), ints([0, 0])
    table = torch.arange(nb * max_pages, dtype=torch.int32, device="cuda").view(nb, max_pages)
    out, lse = torch.zeros((T, Hq, D), device="cuda"), torch.zeros((Hq, T), device="cuda")

    def step(c, ln, aft, tb, k_pool, v_pool, o, l):
        fa.fa_kvcache_append_varlen_d256_fp8(kn, vn, k_pool, v_pool, c, ln, aft, tb, ks, vs)
        fa.fa_forward_varlen_kvcache_d256_fp8(q, k_pool, v_pool, c, aft, block_table=tb, k_scale=ks, v_scale=vs, causal=True, out=o, lse=l)

    step(cu.clone(), lens.clone(), after.clone(), table.clone(), kp.clone(), vp.clone(), out.clone(), lse.clone())   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(cu, lens, after, table, kp, vp, out, lse)
    qf = q.float().cpu().numpy()
    for r, (vec, L, mul) in enumerate((([1, 130, 162], [130, 251], 1.0), ([0, 0, 192], [63, 64], 1.25), ([2, 19, 199], [7, 190], 0.75))):
        perm = torch.randperm(num_pages, device="cuda", generator=gen)[:nb * max_pages].to(torch.int32).view(nb, max_pages)
        for dst, src in ((cu, ints(vec)), (lens, ints(L)), (table, perm), (ks, ks * mul), (vs, vs * mul)):
            dst.copy_(src)
        out.fill_(dv.SENTINEL_LSE), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        lay, m = dv.Layout(vec, T, MQ), [vec[b + 1] - vec[b] for b in range(nb)]
        free = torch.from_numpy(~lay.owned).cuda()
        assert (out[free] == dv.SENTINEL_LSE).all() and (lse[:, free] == dv.SENTINEL_LSE).all(), "a token of no sequence was written"
        tb = perm.cpu().numpy()   # the sequences' keys as the pool holds them now, behind the table
        k, v = ((f8.decode(p.view(torch.uint8).cpu().numpy()[tb].transpose(0, 2, 1, 3, 4).reshape(nb, Hkv, NCAP, D)).astype(np.float64)
                 * s.cpu().numpy().astype(np.float64)[None, :, None, None]).reshape(nb * Hkv, NCAP, D) for p, s in ((kp, ks), (vp, vs)))
        want = cm.expected_f64(dv.unpack_rows(lay, qf, nb), k, v, after.tolist(), nb, Hkv, G, MQ, True, nq=lay.n)
        dv.check(oracle, lay, np.where(lay.owned[:, None, None], out.cpu().numpy(), 0.0).astype(np.float32),
                 np.where(lay.owned[None, :], lse.cpu().numpy(), -np.inf).astype(np.float32), want[0], want[1], 0, f"replay {r}",
                 sentinel=False)
        o2, l2 = fa.fa_kvcache_decode_d256_fp8(q, kp, vp, cu, 32, cache_seqlens=after, block_table=table, k_scale=ks, v_scale=vs,
                                               causal=True, return_lse=True)
        torch.cuda.synchronize()
        for t in (slice(vec[b], vec[b + 1]) for b in range(nb) if 0 < m[b] <= 32):   # the same problem for both entries
            a, d2 = out[t].cpu().numpy(), o2[t].cpu().numpy()
            ma, rl, le = oracle.max_abs(a, d2), oracle.rel_l2(a, d2), float((lse[:, t] - l2[:, t]).abs().max())
            print(f"replay {r}, tokens {t} vs decode: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e}")
            assert ma <= cm.MAX_ABS and rl <= cm.REL_L2[0] and le <= 2 * cm.P_EPS[0], (r, t)
