"""GPU tier of fa_kvcache_decode_d256_fp8 and fa_kvcache_append_varlen_d256: the d = 256 decode on an e4m3fn cache and the packed
append that fills a d = 256 cache, 16-bit or e4m3fn.  The decode runs on the batch of tests/test_gpu_kv256.py (imported: layout,
lengths, sentinels) with caches quantised by quantize_kv_fp8; the float64 reference sees decode(codes) * scale[h], so fp8 adds no
error term and the bounds are cm.check_decode's.  Every row and page nothing may read holds the NaN code 0x7F.  The append is compared
byte for byte with tests/append_varlen_inputs.py's numpy model at d = 256."""
import functools

import numpy as np
import pytest

import append_varlen_inputs as av
import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv
import fp8_inputs as f8
import test_gpu_kv256 as base
from test_gpu_kv256 import torch_cuda   # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

D, NCAP, MAXQ, B, LENS, LAY = base.D, base.NCAP, base.MAXQ, base.B, base.LENS, base.LAY
NAN8 = f8.NAN_CODES[0]
# (fmt, 16-bit output, Hkv, G, causal, W, softcap, num_splits, page size or 0, per-head scales): a pruned product
CASES = [
    (0, False, 2, 4, True, 0, 0.0, 0, 0, True), (1, False, 2, 4, True, 0, 0.0, 1, 16, False), (0, True, 1, 8, True, 70, 0.0, 3, 64, True),
    (1, True, 1, 8, False, 70, 0.0, 3, 0, True), (0, False, 1, 8, False, 0, 30.0, 4, 16, True), (1, False, 2, 4, True, 70, 30.0, 1, 0, False),
    (0, False, 1, 8, True, 70, 30.0, 3, 64, False), (1, True, 2, 4, True, 70, 30.0, 4, 16, True), (0, True, 2, 4, False, 0, 0.0, 4, 0, False),
    (1, False, 1, 8, True, 0, 0.0, 4, 64, True), (0, False, 1, 8, False, 0, 0.0, 3, 16, False), (1, False, 2, 4, False, 70, 0.0, 0, 64, True),
]


@functools.lru_cache(maxsize=None)
def _quantised(fa, oracle, fmt, Hkv, G, scaled):
    """-> (q fp32, q bits, K codes, V codes [B, Hkv, NCAP, D] uint8, k_scale, v_scale [Hkv] fp32): quantize_kv_fp8 per head, or at 1.0"""
    import torch
    (q, k, v), (qb, _, _) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2560 + Hkv)
    out = []
    for x in (k, v):
        x8, s = fa.quantize_kv_fp8(torch.from_numpy(x.reshape(B, Hkv, NCAP, D).copy()), None if scaled else torch.ones(Hkv))
        out.append((x8.view(torch.uint8).numpy(), s.numpy()))
    return q, qb, out[0][0], out[1][0], out[0][1], out[1][1]


@functools.lru_cache(maxsize=None)
def _reference(fa, oracle, fmt, Hkv, G, causal, W, softcap, scaled, zeroed=()):
    q, _, kc, vc, ks, vs = _quantised(fa, oracle, fmt, Hkv, G, scaled)
    k, v = ((f8.decode(c).astype(np.float64) * s[None, :, None, None]).reshape(B * Hkv, NCAP, D) for c, s in ((kc, ks), (vc, vs)))
    for b, j0, j1 in zeroed:
        k[b * Hkv:(b + 1) * Hkv, j0:j1] = v[b * Hkv:(b + 1) * Hkv, j0:j1] = 0.0
    return cm.expected_f64(q, k, v, LENS, B, Hkv, G, MAXQ, causal, W, scale=base.SOFTCAP_SCALE if softcap else None, softcap=softcap,
                           nq=LAY.n)


def _run(fa, torch, qb, kc, vc, fmt, Hkv, G, causal, W, softcap, S, ps, out16=False, scales=(None, None), table_edit=None, wide=False,
         scale=None):
    """one call on sentinel-filled O and lse -> (O, lse); kc, vc: codes [B, Hkv, NCAP, D].  Rows and pages nothing may read get 0x7F,
    tokens of no sequence NaN (Q) and sentinels (O, lse), which must survive.  wide: fa_kvcache_decode_d256 on the widened cache."""
    seen = [L if n else 0 for L, n in zip(LENS, LAY.n)]
    kc, vc = (np.concatenate([cm.poisoned(x[b:b + 1], seen[b:b + 1], max(LAY.n[b], 1), W, nan=NAN8) for b in range(B)]) for x in (kc, vc))
    q = cm.dev16(torch, dv.pack_rows(LAY, qb, cm.NAN16), fmt)
    out = torch.empty((LAY.total_q, Hkv * G, D), dtype=q.dtype if out16 else torch.float32, device="cuda")
    out.view(torch.int16 if out16 else torch.int32).fill_(dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)
    lse = torch.full((Hkv * G, LAY.total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    table = None
    if ps:
        kc, vc, tb = cm.scatter(kc, vc, seen, ps, 7 + ps, MAXQ, W, nan=NAN8)
        if table_edit:
            table_edit(tb, kc.shape[0])
        table = torch.from_numpy(tb).cuda()
    k8, v8 = cm.dev8(torch, kc), cm.dev8(torch, vc)
    kw = dict(cache_seqlens=torch.tensor(LENS, dtype=torch.int32, device="cuda"), block_table=table, causal=causal, window=W,
              scale=scale if scale is not None else base.SOFTCAP_SCALE if softcap else None, softcap=softcap, out=out, lse=lse, num_splits=S)
    cu = torch.from_numpy(LAY.cu).cuda()
    if wide:
        fa.fa_kvcache_decode_d256(q, k8.to(q.dtype), v8.to(q.dtype), cu, MAXQ, **kw)
    else:
        ks, vs = (None if s is None else torch.from_numpy(np.asarray(s, np.float32)).cuda() for s in scales)
        fa.fa_kvcache_decode_d256_fp8(q, k8, v8, cu, MAXQ, k_scale=ks, v_scale=vs, **kw)
    torch.cuda.synchronize()
    free = torch.from_numpy(~LAY.owned).cuda()
    assert (out[free].contiguous().view(torch.int16 if out16 else torch.int32) == (dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)).all(), \
        "an O row of no sequence was written"
    assert (lse[:, free] == dv.SENTINEL_LSE).all(), "an lse entry of no sequence was written"
    return out, lse


def _check(oracle, out, lse, want, fmt, what):
    got = dv.unpack_rows(LAY, out.float().cpu().numpy(), B)
    got_lse = dv.unpack_rows(LAY, np.ascontiguousarray(lse.cpu().numpy().T), B, fill=-np.inf)
    cm.check_decode(oracle, got, got_lse, np.asarray(want[0], np.float32), want[1], fmt, what)


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,out16,Hkv,G,causal,W,softcap,S,ps,scaled", CASES)
def test_against_float64(fa, oracle, torch_cuda, fmt, out16, Hkv, G, causal, W, softcap, S, ps, scaled):
    _, qb, kc, vc, ks, vs = _quantised(fa, oracle, fmt, Hkv, G, scaled)
    out, lse = _run(fa, torch_cuda, qb, kc, vc, fmt, Hkv, G, causal, W, softcap, S, ps, out16, (ks, vs) if scaled else (None, None))
    _check(oracle, out, lse, _reference(fa, oracle, fmt, Hkv, G, causal, W, softcap, scaled), fmt,
           f"{cm.FMT_NAME[fmt]} out16={out16} Hkv={Hkv} G={G} causal={causal} W={W} softcap={softcap} S={S} pages={ps} scaled={scaled}")


# ---- 2. the 16-bit entry's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("S", [1, 3, 0])
def test_bits_of_the_16_bit_entry(fa, oracle, torch_cuda, fmt, S):
    """a cache of all 254 finite codes: null scales return fa_kvcache_decode_d256's bits on the widened cache; k_scale = 2^-3 and
    v_scale = 2^2 return the 16-bit call's at scale * 2^-3, times 4; pages of 16 return the contiguous bits"""
    torch, Hkv, G = torch_cuda, 2, 4
    _, (qb, _, _) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2560 + Hkv)
    kc, vc = (f8.all_codes_cache(B, Hkv, NCAP, D, LENS, seed) for seed in (801, 802))
    run = functools.partial(_run, fa, torch, qb, kc, vc, fmt, Hkv, G, True, 0, 0.0, S)
    sc = 2.0 ** -10   # the codes reach 448: logits of a few units
    own = torch.from_numpy(LAY.owned).cuda()   # the other tokens hold the sentinel, a NaN pattern
    want, want2 = run(0, wide=True, scale=sc), run(0, wide=True, scale=sc / 8)
    for ps in (0, 16):
        got = run(ps, scale=sc)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), f"null scales, pages {ps}"
        got = run(ps, scale=sc, scales=([0.125] * Hkv, [4.0] * Hkv))
        assert torch.equal(got[0][own], want2[0][own] * 4) and torch.equal(got[1], want2[1]), f"power-of-two scales, pages {ps}"


# ---- 3. a bad live page -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1, None])
def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda, bad):
    """entry -1 and entry num_pages in the place of live pages 3 (sequence 5) and 0 (sequence 6): the bits of the call on the good
    table with those pages' codes zeroed"""
    torch, fmt, Hkv, G, ps = torch_cuda, 0, 2, 4, 16
    _, qb, kc, vc, ks, vs = _quantised(fa, oracle, fmt, Hkv, G, True)

    def edit(tb, num_pages):
        tb[5, 3] = tb[6, 0] = num_pages if bad is None else bad

    kz, vz = kc.copy(), vc.copy()
    kz[5, :, 48:64] = vz[5, :, 48:64] = kz[6, :, 0:16] = vz[6, :, 0:16] = 0
    for S in (1, 3):
        out, lse = _run(fa, torch, qb, kc, vc, fmt, Hkv, G, True, 0, 0.0, S, ps, scales=(ks, vs), table_edit=edit)
        want = _run(fa, torch, qb, kz, vz, fmt, Hkv, G, True, 0, 0.0, S, ps, scales=(ks, vs))
        assert torch.equal(out.view(torch.int32), want[0].view(torch.int32)) and torch.equal(lse, want[1]), (bad, S)
        _check(oracle, out, lse, _reference(fa, oracle, fmt, Hkv, G, True, 0, 0.0, True, ((5, 48, 64), (6, 0, 16))), fmt, f"bad page {bad}")


# ---- 4. append bytes --------------------------------------------------------------------------------------------------------------------
def _bits(torch, t):
    return t.contiguous().view(torch.uint8).cpu().numpy() if t.element_size() == 1 else \
        t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("paged,fp8,rope", [pytest.param(*f, id=av.form_id(*f)) for f in av.FORMS])
@pytest.mark.parametrize("fmt", [0, 1])
def test_append_bytes(fa, torch_cuda, fmt, paged, fp8, rope):
    """the whole cache or pool, the rotated Q and seqlens_out against the numpy model at d = 256 (NaN patterns in every row no kept
    token touches): once from packed sources into a q_out of its own, once from the views of one fused buffer with Q rotated in place
    and, in the rotary forms, positions[s_b + i] = L_b + i, which are the plain call's bytes"""
    torch = torch_cuda
    x = av.inputs(fmt, D, paged, fp8, rope)
    ints = lambda v: torch.tensor([int(i) for i in v], dtype=torch.int32, device="cuda")   # noqa: E731
    flt = lambda v: None if v is None else torch.from_numpy(np.array(v, np.float32)).cuda()   # noqa: E731
    Hkv, Hq = x["knb"].shape[1], x["qsrc"].shape[1]
    pos = np.full(x["total"], -5, np.int32)
    for (s, e), L in zip(av.bounds(x["cu"], x["total"]), x["lens"]):
        pos[s:e] = cm.clamp(L, av.CASE["Ncap"]) + np.arange(e - s)
    for fused in (False, True):
        dk, dv_ = ((cm.dev8(torch, x[n]) if fp8 else cm.dev16(torch, x[n], fmt)) for n in ("kc0", "vc0"))
        if fused:
            buf = cm.dev16(torch, np.concatenate([x["qsrc"], x["knb"], x["vnb"]], axis=1), fmt)
            dq, dkn, dvn, dqo = buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:], None
        else:
            dq, dkn, dvn = (cm.dev16(torch, x[n], fmt) for n in ("qsrc", "knb", "vnb"))
            dqo = cm.dev16(torch, np.full(x["qsrc"].shape, av.QOUT_NAN, np.uint16), fmt)
        lens = ints(x["lens"])
        kw = dict(block_table=None if x["table"] is None else torch.from_numpy(np.array(x["table"])).cuda())
        if rope:
            kw.update(q=dq, q_out=dqo, rotary_cos=flt(x["cos"]), rotary_sin=flt(x["sin"]), rotary_interleaved=rope == 2,
                      positions=torch.from_numpy(pos).cuda() if fused else None)
        if fp8:
            fa.fa_kvcache_append_varlen_d256_fp8(dkn, dvn, dk, dv_, ints(x["cu"]), lens, lens, k_scale=flt(x["ks"]), v_scale=flt(x["vs"]), **kw)
        else:
            fa.fa_kvcache_append_varlen_d256(dkn, dvn, dk, dv_, ints(x["cu"]), lens, lens, **kw)
        torch.cuda.synchronize()
        want = av.model(fmt, D, paged, fp8, rope, qout0=x["qsrc"] if fused else None)
        assert np.array_equal(_bits(torch, dk), want["k"]) and np.array_equal(_bits(torch, dv_), want["v"]), f"fused={fused}: K or V differs"
        assert lens.tolist() == [int(v) for v in want["lens"]]
        if rope:
            assert np.array_equal(_bits(torch, dq if fused else dqo), want["qout"]), f"fused={fused}: the rotated Q differs"
        assert np.array_equal(_bits(torch, dkn), x["knb"]) and np.array_equal(_bits(torch, dvn), x["vnb"]), "a source was written"


# ---- 5. the captured step -----------------------------------------------------------------------------------------------------------------
def test_captured_append_then_decode(fa, oracle, torch_cuda):
    """append_varlen_d256_fp8 -> decode_d256_fp8 on pages of 16 behind a split, captured once and replayed after cu_seqlens, the
    lengths, the table and the scales are rewritten in place; each replay against float64 on the codes the pool then holds"""
    torch = torch_cuda
    Hkv, G, ps, T, S, W, nb = 2, 4, 16, 9, 2, 70, 2
    Hq, max_pages = Hkv * G, NCAP // ps
    num_pages = nb * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(2560)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen).to(torch.float16)   # noqa: E731
    ints = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")   # noqa: E731
    q, kn, vn = rnd(T, Hq, D), rnd(T, Hkv, D), rnd(T, Hkv, D)
    (kp, ks), (vp, vs) = (fa.quantize_kv_fp8(rnd(num_pages, Hkv, ps, D)) for _ in range(2))
    cu, lens, after = ints([0, 4, 9]), ints([200, 100]), ints([0, 0])
    table = torch.arange(nb * max_pages, dtype=torch.int32, device="cuda").view(nb, max_pages)
    out, lse = torch.zeros((T, Hq, D), device="cuda"), torch.zeros((Hq, T), device="cuda")
    ws = torch.empty(fa.kvcache_decode_d256_fp8_workspace_bytes(nb, Hkv, G, MAXQ, max_pages=max_pages, page_size=ps, window=W, num_splits=S),
                     dtype=torch.uint8, device="cuda")

    def step(c, ln, aft, tb, k_pool, v_pool, o, l):
        fa.fa_kvcache_append_varlen_d256_fp8(kn, vn, k_pool, v_pool, c, ln, aft, tb, ks, vs)
        fa.fa_kvcache_decode_d256_fp8(q, k_pool, v_pool, c, MAXQ, cache_seqlens=aft, block_table=tb, k_scale=ks, v_scale=vs, causal=True,
                                      window=W, out=o, lse=l, workspace=ws, num_splits=S)

    step(cu.clone(), lens.clone(), after.clone(), table.clone(), kp.clone(), vp.clone(), out.clone(), lse.clone())   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(cu, lens, after, table, kp, vp, out, lse)
    qf = q.float().cpu().numpy()
    for r, (vec, L, mul) in enumerate((([1, 3, 8], [130, 251], 1.0), ([0, 0, 5], [63, 64], 1.25), ([2, 7, 9], [7, 190], 0.75))):
        perm = torch.randperm(num_pages, device="cuda", generator=gen)[:nb * max_pages].to(torch.int32).view(nb, max_pages)
        for dst, src in ((cu, ints(vec)), (lens, ints(L)), (table, perm), (ks, ks * mul), (vs, vs * mul)):
            dst.copy_(src)
        out.fill_(dv.SENTINEL_LSE), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        lay = dv.Layout(vec, T, MAXQ)
        m = [vec[b + 1] - vec[b] for b in range(nb)]
        assert after.tolist() == [min(L[b] + m[b], NCAP) for b in range(nb)]
        free = torch.from_numpy(~lay.owned).cuda()
        assert (out[free] == dv.SENTINEL_LSE).all() and (lse[:, free] == dv.SENTINEL_LSE).all()
        # the sequences' keys as the pool holds them now, behind the table
        tb = perm.cpu().numpy()
        k, v = ((f8.decode(_bits(torch, p)[tb].transpose(0, 2, 1, 3, 4).reshape(nb, Hkv, NCAP, D)).astype(np.float64)
                 * s.cpu().numpy().astype(np.float64)[None, :, None, None]).reshape(nb * Hkv, NCAP, D) for p, s in ((kp, ks), (vp, vs)))
        qpad = dv.unpack_rows(lay, qf, nb)
        want = cm.expected_f64(qpad, k, v, after.tolist(), nb, Hkv, G, MAXQ, True, W, nq=lay.n)
        got = dv.unpack_rows(lay, np.where(lay.owned[:, None, None], out.cpu().numpy(), 0.0).astype(np.float32), nb)
        got_lse = dv.unpack_rows(lay, np.where(lay.owned[:, None], lse.cpu().numpy().T, -np.inf).astype(np.float32), nb, fill=-np.inf)
        cm.check_decode(oracle, got, got_lse, np.asarray(want[0], np.float32), want[1], 0, f"replay {r}")
