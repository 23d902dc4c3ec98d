"""GPU tier of fa_kvcache_decode_d256: token-packed split-KV decode at head dimension 256.  One batch of eight sequences throughout
(Ncap = 256, max_q = 5): lengths at the tile's edges and a raw one above the capacity, row counts 0, 1, 3, 5 and one sequence that owns
more tokens than max_q, so the packed tensors have tokens of no sequence before s_0, behind the cut sequence and past the last one.
Reference: cm.expected_f64 (float64, row by row) on the padded rows, scattered to the packed layout; bounds: the project's (MAX_ABS,
REL_L2, 2 * P_EPS on lse), which are also the soft-cap tier's (tests/test_gpu_kvcache_logits.py).  Caches come from cm.poisoned /
cm.scatter: every row and page nothing may read holds NaN, and the table entries of dead pages hold garbage."""
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv

pytestmark = pytest.mark.gpu

D, NCAP, MAXQ, B = 256, 256, 5, 8
LENS = (0, 1, 63, 64, 65, 200, 256, 300)
SPANS = (3, 1, 5, 0, 7, 3, 5, 1)            # tokens each sequence owns; n_b = min(span, MAXQ): 40 rows at G = 8 cross the 32-row block
CU = np.cumsum((dv.LEAD,) + SPANS)
LAY = dv.Layout(CU, int(CU[-1]) + dv.TRAIL, MAXQ)
SOFTCAP_SCALE = 0.25                        # logits of about N(0, 4^2): a cap of 30 bends the large ones by far more than the bounds
# (fmt, 16-bit output, Hkv, G, causal, W, softcap, num_splits, page size or 0): a pruned product
CASES = [
    (0, False, 2, 4, True, 0, 0.0, 0, 0), (1, False, 2, 4, True, 0, 0.0, 1, 16), (0, True, 1, 8, True, 5, 0.0, 2, 64),
    (1, True, 1, 8, False, 70, 0.0, 3, 0), (0, False, 1, 1, False, 0, 30.0, 4, 16), (1, False, 1, 1, True, 70, 30.0, 2, 0),
    (0, False, 1, 8, True, 70, 30.0, 3, 64), (1, True, 2, 4, True, 5, 30.0, 4, 16), (0, True, 2, 4, False, 5, 0.0, 4, 0),
    (1, False, 1, 8, True, 0, 0.0, 4, 64), (0, False, 1, 8, False, 0, 0.0, 3, 16), (1, False, 2, 4, False, 70, 0.0, 2, 64),
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _reference(oracle, fmt, Hkv, G, causal, W, softcap, zeroed=()):
    """the padded float64 pair, computed once; zeroed: (sequence, first key, last key) ranges whose K and V rows read as zeros"""
    (q, k, v), _ = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2560 + Hkv)
    if zeroed:
        k, v = k.copy(), v.copy()
        for b, j0, j1 in zeroed:
            k[b * Hkv:(b + 1) * Hkv, j0:j1] = v[b * Hkv:(b + 1) * Hkv, j0:j1] = 0.0
    return cm.expected_f64(q, k, v, LENS, B, Hkv, G, MAXQ, causal, W, scale=SOFTCAP_SCALE if softcap else None, softcap=softcap, nq=LAY.n)


def _caches(oracle, fmt, Hkv, G, W):
    """the K and V caches [B, Hkv, NCAP, D] with NaN in every row no row of the sequence sees (all rows where n_b = 0)"""
    _, (_, kb, vb) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2560 + Hkv)
    seen = [L if n else 0 for L, n in zip(LENS, LAY.n)]
    return [np.concatenate([cm.poisoned(x.reshape(B, Hkv, NCAP, D)[b:b + 1], seen[b:b + 1], max(LAY.n[b], 1), W) for b in range(B)])
            for x in (kb, vb)], seen


def _run(fa, torch, oracle, fmt, Hkv, G, causal, W, softcap, S, ps, out16=False, table_edit=None, fused=False):
    """one call on sentinel-filled O and lse -> (O, lse) device tensors; every token of no sequence must still hold its sentinel"""
    _, (qb, _, _) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2560 + Hkv)
    Hq = Hkv * G
    (kc, vc), seen = _caches(oracle, fmt, Hkv, G, W)
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
    table = None
    if ps:
        kc, vc, tb = cm.scatter(kc, vc, seen, ps, 7 + ps, MAXQ, W)
        if table_edit:
            table_edit(tb, kc.shape[0])
        table = torch.from_numpy(tb).cuda()
    o = fa.fa_kvcache_decode_d256(q, cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), torch.from_numpy(LAY.cu).cuda(), MAXQ,
                                  cache_seqlens=torch.tensor(LENS, dtype=torch.int32, device="cuda"), block_table=table, causal=causal,
                                  scale=SOFTCAP_SCALE if softcap else None, window=W, softcap=softcap, out=out, lse=lse, num_splits=S)
    torch.cuda.synchronize()
    assert o[0] is out and o[1] is lse
    free = torch.from_numpy(~LAY.owned).cuda()
    assert (out[free].contiguous().view(torch.int16 if out16 else torch.int32) == (dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)).all(), \
        "an O row of no sequence was written"
    assert (lse[:, free] == dv.SENTINEL_LSE).all(), "an lse entry of no sequence was written"
    return out, lse


def _check(oracle, out, lse, want, fmt, what):
    dv.check(oracle, LAY, out.float().cpu().numpy(), lse.cpu().numpy(), want[0], want[1], fmt, what, sentinel=False)


@pytest.mark.parametrize("fmt,out16,Hkv,G,causal,W,softcap,S,ps", CASES)
def test_against_float64(fa, oracle, torch_cuda, fmt, out16, Hkv, G, causal, W, softcap, S, ps):
    out, lse = _run(fa, torch_cuda, oracle, fmt, Hkv, G, causal, W, softcap, S, ps, out16)
    _check(oracle, out, lse, _reference(oracle, fmt, Hkv, G, causal, W, softcap), fmt,
           f"{cm.FMT_NAME[fmt]} out16={out16} Hkv={Hkv} G={G} causal={causal} W={W} softcap={softcap} S={S} pages={ps}")


@pytest.mark.parametrize("W,softcap", [(0, 0.0), (70, 30.0)])
def test_paged_bits_and_views(fa, oracle, torch_cuda, W, softcap):
    """for every split count: pages of 16 and of 64 return the contiguous call's bits, and so does the call on a fused Q buffer with a
    padded O stride"""
    torch = torch_cuda
    for S in range(5):
        base = _run(fa, torch, oracle, 0, 2, 4, True, W, softcap, S, 0)
        for kw in (dict(ps=16), dict(ps=64), dict(ps=0, fused=True)):
            got = _run(fa, torch, oracle, 0, 2, 4, True, W, softcap, S, **kw)
            assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)) and torch.equal(got[1], base[1]), (S, kw)


def test_a_sequence_alone_has_the_bits_it_has_in_the_batch(fa, oracle, torch_cuda):
    torch = torch_cuda
    fmt, Hkv, G, S, b = 1, 2, 4, 2, 5
    out, lse = _run(fa, torch, oracle, fmt, Hkv, G, True, 70, 0.0, S, 0)
    _, (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, MAXQ, NCAP, D, fmt, 2560 + Hkv)
    n, Hq = LAY.n[b], Hkv * G
    q1 = cm.dev16(torch, np.ascontiguousarray(qb[b * Hq:(b + 1) * Hq, :n].transpose(1, 0, 2)), fmt)
    k1, v1 = (cm.dev16(torch, x.reshape(B, Hkv, NCAP, D)[b:b + 1], fmt) for x in (kb, vb))
    o1, l1 = fa.fa_kvcache_decode_d256(q1, k1, v1, torch.tensor([0, n], dtype=torch.int32, device="cuda"), MAXQ,
                                       cache_seqlens=torch.tensor(LENS[b:b + 1], dtype=torch.int32, device="cuda"), causal=True, window=70,
                                       return_lse=True, num_splits=S)
    t = slice(LAY.s[b], LAY.s[b] + n)
    assert torch.equal(o1, out[t]) and torch.equal(l1, lse[:, t])


@pytest.mark.parametrize("bad", [-1, None])
def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda, bad):
    """entry -1 and entry num_pages in the place of the live pages 3 (sequence 5, 200 keys) and 0 (sequence 6, full): the result is the
    reference with those pages' K and V rows zeroed -- keys of logit 0 and value 0, not masked ones"""
    fmt, Hkv, G, ps = 0, 2, 4, 16

    def edit(tb, num_pages):
        tb[5, 3] = tb[6, 0] = num_pages if bad is None else bad

    for S in (1, 3):
        out, lse = _run(fa, torch_cuda, oracle, fmt, Hkv, G, True, 0, 0.0, S, ps, table_edit=edit)
        _check(oracle, out, lse, _reference(oracle, fmt, Hkv, G, True, 0, 0.0, ((5, 48, 64), (6, 0, 16))), fmt, f"bad page {bad} S={S}")


def test_captured_call_follows_its_vectors(fa, oracle, torch_cuda):
    """a paged call behind a split, captured once; replayed after cu_seqlens_q, the lengths and the table are rewritten in place, each
    replay against the eager call from the same state, bit for bit"""
    torch = torch_cuda
    Hkv, G, ps, T, S = 2, 4, 16, 9, 2
    Hq, max_pages = Hkv * G, NCAP // ps
    num_pages = 2 * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(256)
    rnd = lambda *s: (torch.rand(s, device="cuda", generator=gen) * 2 - 1).to(torch.float16)   # noqa: E731
    q, kp, vp = rnd(T, Hq, D), rnd(num_pages, Hkv, ps, D), rnd(num_pages, Hkv, ps, D)
    ints = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
    cu, lens, table = ints([0, 4, 9]), ints([256, 100]), torch.arange(2 * max_pages, dtype=torch.int32, device="cuda").view(2, max_pages)
    out, lse = torch.zeros((T, Hq, D), device="cuda"), torch.zeros((Hq, T), device="cuda")
    ws = torch.empty(fa.kvcache_decode_d256_workspace_bytes(2, Hkv, G, MAXQ, max_pages=max_pages, page_size=ps, window=70, num_splits=S),
                     dtype=torch.uint8, device="cuda")

    def step(c, ln, tb, o, l):
        fa.fa_kvcache_decode_d256(q, kp, vp, c, MAXQ, cache_seqlens=ln, block_table=tb, causal=True, window=70, softcap=30.0, out=o, lse=l,
                                  workspace=ws, num_splits=S)

    step(cu.clone(), lens.clone(), table.clone(), out.clone(), lse.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(cu, lens, table, out, lse)
    for s, (vec, L) in enumerate((([1, 3, 8], [130, 300]), ([0, 0, 5], [64, 65]), ([2, 9, 9], [7, 200]))):
        perm = torch.randperm(num_pages, device="cuda", generator=gen)[:2 * max_pages].to(torch.int32).view(2, max_pages)
        for dst, src in ((cu, ints(vec)), (lens, ints(L)), (table, perm)):
            dst.copy_(src)
        ws.fill_(0xFF), out.fill_(dv.SENTINEL_LSE), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        eo, el = torch.full_like(out, dv.SENTINEL_LSE), torch.full_like(lse, dv.SENTINEL_LSE)
        ws.fill_(0xFF)
        step(cu.clone(), lens.clone(), table.clone(), eo, el)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eo.view(torch.int32)) and torch.equal(lse, el), f"replay {s} differs from the eager call"
        live = torch.from_numpy(dv.Layout(vec, T, MAXQ).owned).cuda()
        assert torch.isfinite(out[live]).all() and (out[~live] == dv.SENTINEL_LSE).all(), s
