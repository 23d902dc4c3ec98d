"""GPU tier of fa_forward_varlen_kvcache_d256 and fa_forward_varlen_d256: the varlen prefill at head dimension 256.  One batch of six
sequences throughout (Ncap = 640): Lq = (1, 63, 65, 0, 129, 257) rows over cache lengths (0, 200, 15, 5, 70, 300) -- a block edge at
128 rows, a tile edge at 64 keys, a sequence without rows, sequences without keys and with Lk < Lq -- with tokens of no sequence in
front of the first and behind the last.  Reference: cm.expected_f64 (float64, row by row) on the padded rows; bounds: the project's
(MAX_ABS, REL_L2, 2 * P_EPS on lse), none new.  Caches come from cm.poisoned / cm.scatter: every row and page nothing may read holds
NaN, the table entries of dead pages hold garbage, and so do the Q rows of no sequence."""
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv

pytestmark = pytest.mark.gpu

D, NCAP, B = 256, 640, 6
LQ = (1, 63, 65, 0, 129, 257)
LENS = (0, 200, 15, 5, 70, 300)
MAXQ = max(LQ)
CU = np.cumsum((dv.LEAD,) + LQ)
LAY = dv.Layout(CU, int(CU[-1]) + dv.TRAIL, MAXQ)
SEEN = tuple(L if n else 0 for L, n in zip(LENS, LQ))   # a sequence without rows reads nothing
SOFTCAP_SCALE = 0.25                        # logits of about N(0, 4^2): a cap of 30 bends the large ones by far more than the bounds
# (fmt, 16-bit output, Hkv, G, causal, W, softcap, page size or 0): a pruned product
CASES = [
    (0, False, 2, 4, True, 0, 0.0, 0), (1, False, 2, 4, True, 0, 0.0, 16), (0, True, 1, 8, True, 17, 0.0, 64),
    (1, True, 1, 8, False, 100, 0.0, 0), (0, False, 1, 1, False, 0, 30.0, 128), (1, False, 1, 1, True, 400, 30.0, 0),
    (0, False, 1, 8, True, 100, 30.0, 16), (1, True, 2, 4, True, 1, 30.0, 64), (0, True, 2, 4, False, 17, 0.0, 128),
    (1, False, 1, 8, True, 1, 0.0, 16), (0, False, 1, 8, False, 400, 0.0, 64), (1, False, 2, 4, False, 0, 30.0, 128),
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _inputs(oracle, fmt, Hkv, G):
    return di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2570 + Hkv)


@functools.lru_cache(maxsize=None)
def _reference(oracle, fmt, Hkv, G, causal, W, softcap, zeroed=()):
    """the padded float64 pair, computed once; zeroed: (sequence, first key, last key) ranges whose K and V rows read as zeros"""
    (q, k, v), _ = _inputs(oracle, fmt, Hkv, G)
    if zeroed:
        k, v = k.copy(), v.copy()
        for b, j0, j1 in zeroed:
            k[b * Hkv:(b + 1) * Hkv, j0:j1] = v[b * Hkv:(b + 1) * Hkv, j0:j1] = 0.0
    return cm.expected_f64(q, k, v, LENS, B, Hkv, G, MAXQ, causal, W, scale=SOFTCAP_SCALE if softcap else None, softcap=softcap, nq=LQ)


def _run(fa, torch, oracle, fmt, Hkv, G, causal, W, softcap, ps, out16=False, table_edit=None, fused=False, packed=False):
    """one call on sentinel-filled O and lse -> (O, lse) device tensors; every token of no sequence must still hold its sentinel.
    packed: fa_forward_varlen_d256 on the gathered K/V rows [0, Lk) of every sequence, NaN rows of no sequence in front and behind"""
    _, (qb, kb, vb) = _inputs(oracle, fmt, Hkv, G)
    Hq = Hkv * G
    q = cm.dev16(torch, dv.pack_rows(LAY, qb, cm.NAN16), fmt)   # tokens of no sequence hold NaN
    odt = q.dtype if out16 else torch.float32
    out = torch.empty((LAY.total_q, Hq, D), dtype=odt, device="cuda")
    if fused:   # Q as the slice of a fused (total, Hq + 2 Hkv, D) buffer, O with a padded token stride
        buf = torch.full((LAY.total_q, Hq + 2 * Hkv, D), float("nan"), dtype=q.dtype, device="cuda")
        buf[:, :Hq] = q
        q = buf[:, :Hq]
        out = torch.empty((LAY.total_q, Hq * D + 64), dtype=odt, device="cuda")[:, :Hq * D].view(LAY.total_q, Hq, D)
    out.view(torch.int16 if out16 else torch.int32).fill_(dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)
    lse = torch.full((Hq, LAY.total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    kw = dict(causal=causal, scale=SOFTCAP_SCALE if softcap else None, window=W, softcap=softcap, out=out, lse=lse)
    cu = torch.from_numpy(LAY.cu).cuda()
    kc, vc = (x.reshape(B, Hkv, NCAP, D) for x in (kb, vb))
    if packed:
        cu_k = np.cumsum((2,) + SEEN).astype(np.int32)
        kp, vp = (np.full((int(cu_k[-1]) + 3, Hkv, D), cm.NAN16, np.uint16) for _ in range(2))
        for b in range(B):
            for dst, src in ((kp, kc), (vp, vc)):
                dst[cu_k[b]:cu_k[b + 1]] = src[b, :, :SEEN[b]].transpose(1, 0, 2)
        o = fa.fa_forward_varlen_d256(q, cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), cu, torch.from_numpy(cu_k).cuda(), **kw)
    else:
        kc, vc = (np.concatenate([cm.poisoned(x[b:b + 1], SEEN[b:b + 1], max(LQ[b], 1), W) for b in range(B)]) for x in (kc, vc))
        table = None
        if ps:
            kc, vc, tb = _scatter(kc, vc, ps, W)
            if table_edit:
                table_edit(tb, kc.shape[0])
            table = torch.from_numpy(tb).cuda()
        o = fa.fa_forward_varlen_kvcache_d256(q, cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), cu,
                                              torch.tensor(LENS, dtype=torch.int32, device="cuda"), block_table=table, **kw)
    torch.cuda.synchronize()
    assert o[0] is out and o[1] is lse
    free = torch.from_numpy(~LAY.owned).cuda()
    assert (out[free].contiguous().view(torch.int16 if out16 else torch.int32) == (dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)).all(), \
        "an O row of no sequence was written"
    assert (lse[:, free] == dv.SENTINEL_LSE).all(), "an lse entry of no sequence was written"
    return out, lse


def _scatter(kc, vc, ps, W):
    """cm.scatter sequence by sequence (each has its own row count, hence its own lo_0), the pools stacked and the tables offset"""
    pools_k, pools_v, rows, base = [], [], [], 0
    for b in range(B):
        kp, vp, tb = cm.scatter(kc[b:b + 1], vc[b:b + 1], SEEN[b:b + 1], ps, 7 + ps + b, max(LQ[b], 1), W, spare=1)
        live = (tb != cm.GARBAGE[0]) & (tb != cm.GARBAGE[1])
        rows.append(np.where(live, tb + base, tb))
        pools_k.append(kp), pools_v.append(vp)
        base += kp.shape[0]
    return np.concatenate(pools_k), np.concatenate(pools_v), np.concatenate(rows).astype(np.int32)


def _check(oracle, out, lse, want, fmt, what):
    dv.check(oracle, LAY, out.float().cpu().numpy(), lse.cpu().numpy(), want[0], want[1], fmt, what, sentinel=False)


@pytest.mark.parametrize("fmt,out16,Hkv,G,causal,W,softcap,ps", CASES)
def test_against_float64(fa, oracle, torch_cuda, fmt, out16, Hkv, G, causal, W, softcap, ps):
    out, lse = _run(fa, torch_cuda, oracle, fmt, Hkv, G, causal, W, softcap, ps, out16)
    _check(oracle, out, lse, _reference(oracle, fmt, Hkv, G, causal, W, softcap), fmt,
           f"{cm.FMT_NAME[fmt]} out16={out16} Hkv={Hkv} G={G} causal={causal} W={W} softcap={softcap} pages={ps}")


@pytest.mark.parametrize("causal,W,softcap", [(True, 0, 0.0), (True, 100, 30.0), (False, 17, 0.0)])
def test_bit_ties_and_views(fa, oracle, torch_cuda, causal, W, softcap):
    """pages of 16, 64 and 128, the packed entry on the gathered K/V, and the call on a fused Q buffer with a padded O stride all
    return the contiguous call's bits, for O and lse; the packed result is checked against float64 too"""
    torch = torch_cuda
    base = _run(fa, torch, oracle, 0, 2, 4, causal, W, softcap, 0)
    for kw in (dict(ps=16), dict(ps=64), dict(ps=128), dict(ps=0, packed=True), dict(ps=0, fused=True), dict(ps=16, fused=True)):
        got = _run(fa, torch, oracle, 0, 2, 4, causal, W, softcap, **kw)
        assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)) and torch.equal(got[1], base[1]), kw
    _check(oracle, *_run(fa, torch, oracle, 1, 1, 8, causal, W, softcap, 0, packed=True), _reference(oracle, 1, 1, 8, causal, W, softcap), 1,
           f"packed causal={causal} W={W} softcap={softcap}")


@pytest.mark.parametrize("bad", [-1, None])
def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda, bad):
    """entry -1 and entry num_pages in the place of the live pages 3 (sequence 1, 200 keys) and 0 (sequence 5, 300 keys): the result is
    the reference with those pages' K and V rows zeroed -- keys of logit 0 and value 0, not masked ones"""
    fmt, Hkv, G, ps = 0, 2, 4, 16

    def edit(tb, num_pages):
        tb[1, 3] = tb[5, 0] = num_pages if bad is None else bad

    out, lse = _run(fa, torch_cuda, oracle, fmt, Hkv, G, True, 0, 0.0, ps, table_edit=edit)
    _check(oracle, out, lse, _reference(oracle, fmt, Hkv, G, True, 0, 0.0, ((1, 48, 64), (5, 0, 16))), fmt, f"bad page {bad}")


@pytest.mark.parametrize("W,softcap", [(0, 0.0), (100, 30.0)])
def test_the_decode_entry_agrees_on_the_short_sequences(fa, oracle, torch_cuda, W, softcap):
    """fa_kvcache_decode_d256, causal, on the same cache with max_seqlen_q = 65: the sequences of at most 65 rows are the same
    problem for both entries; twice the bounds, as two kernels' errors add"""
    torch = torch_cuda
    fmt, Hkv, G = 0, 2, 4
    out, lse = _run(fa, torch, oracle, fmt, Hkv, G, True, W, softcap, 0)
    _, (qb, kb, vb) = _inputs(oracle, fmt, Hkv, G)
    kc, vc = (cm.dev16(torch, x.reshape(B, Hkv, NCAP, D), fmt) for x in (kb, vb))
    q = cm.dev16(torch, dv.pack_rows(LAY, qb, 0), fmt)
    o2, l2 = fa.fa_kvcache_decode_d256(q, kc, vc, torch.from_numpy(LAY.cu).cuda(), 65,
                                       cache_seqlens=torch.tensor(LENS, dtype=torch.int32, device="cuda"), causal=True,
                                       scale=SOFTCAP_SCALE if softcap else None, window=W, softcap=softcap, return_lse=True)
    torch.cuda.synchronize()
    t = slice(int(CU[0]), int(CU[3]))   # the tokens of the sequences 0, 1, 2 (1, 63 and 65 rows)
    a, b2 = out[t].cpu().numpy(), o2[t].cpu().numpy()
    ma, rl = oracle.max_abs(a, b2), oracle.rel_l2(a, b2)
    la, lb = lse[:, t].cpu().numpy(), l2[:, t].cpu().numpy()
    fin = np.isfinite(lb)
    le = float(np.abs(la[fin] - lb[fin]).max())
    print(f"prefill vs decode W={W} softcap={softcap}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e}")
    assert ma <= 2 * cm.MAX_ABS and rl <= 2 * cm.REL_L2[fmt] and le <= 4 * cm.P_EPS[fmt]
    assert (np.isfinite(la) == fin).all() and (a[~fin.T] == 0).all() and (b2[~fin.T] == 0).all()


def test_captured_call_follows_its_vectors(fa, oracle, torch_cuda):
    """a paged call captured once; replayed after cu_seqlens_q, the lengths and the table are rewritten in place, each replay against
    the eager call from the same state, bit for bit"""
    torch = torch_cuda
    Hkv, G, ps, T, cap = 2, 4, 16, 300, 512
    Hq, max_pages = Hkv * G, cap // ps
    num_pages = 2 * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(256)
    rnd = lambda *s: (torch.rand(s, device="cuda", generator=gen) * 2 - 1).to(torch.float16)   # noqa: E731
    q, kp, vp = rnd(T, Hq, D), rnd(num_pages, Hkv, ps, D), rnd(num_pages, Hkv, ps, D)
    ints = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
    cu, lens, table = ints([0, 140, 300]), ints([512, 100]), torch.arange(2 * max_pages, dtype=torch.int32, device="cuda").view(2, max_pages)
    out, lse = torch.zeros((T, Hq, D), device="cuda"), torch.zeros((Hq, T), device="cuda")

    def step(c, ln, tb, o, l):
        fa.fa_forward_varlen_kvcache_d256(q, kp, vp, c, ln, block_table=tb, causal=True, window=100, softcap=30.0, out=o, lse=l)

    step(cu.clone(), lens.clone(), table.clone(), out.clone(), lse.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(cu, lens, table, out, lse)
    for s, (vec, L) in enumerate((([1, 130, 290], [130, 400]), ([0, 0, 257], [64, 300]), ([2, 299, 299], [7, 200]))):
        perm = torch.randperm(num_pages, device="cuda", generator=gen)[:2 * max_pages].to(torch.int32).view(2, max_pages)
        for dst, src in ((cu, ints(vec)), (lens, ints(L)), (table, perm)):
            dst.copy_(src)
        out.fill_(dv.SENTINEL_LSE), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        eo, el = torch.full_like(out, dv.SENTINEL_LSE), torch.full_like(lse, dv.SENTINEL_LSE)
        step(cu.clone(), lens.clone(), table.clone(), eo, el)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eo.view(torch.int32)) and torch.equal(lse, el), f"replay {s} differs from the eager call"
        live = torch.from_numpy(dv.Layout(vec, T, T).owned).cuda()
        assert torch.isfinite(out[live]).all() and (out[~live] == dv.SENTINEL_LSE).all(), s
