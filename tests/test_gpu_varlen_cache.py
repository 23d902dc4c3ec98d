"""GPU tier of fa_forward_varlen_kvcache (the varlen prefill with its K/V rows taken from the KV cache, contiguous or paged), through
the Python front end, which goes through the C ABI.  Inputs, the page layout and the float64 reference are
tests/varlen_cache_inputs.py's, the check is tests/varlen_inputs.py's; tests/test_varlen_cache_inputs.py shows without a GPU that the
check rejects six wrong kernels (a length without the chunk, a wrong table pitch, a row or a tile taken from the wrong page, a head
index outside the page block, a window restarted at the prefix boundary).  Every cache holds NaN in every row and page no visible key
lies in and garbage in every table entry nothing may read; every launch writes into O and lse buffers pre-filled with a poison value."""
import numpy as np
import pytest

import common_inputs as cm
import varlen_cache_inputs as ci
import varlen_inputs as vi
import varlen_logit_inputs as li

pytestmark = pytest.mark.gpu
LAYOUTS = (0,) + ci.PAGE_SIZES          # 0: the contiguous cache


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _i32(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.int32)).cuda()


def _f32(torch, x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.float32)).cuda()


def _np(t):
    return t.float().cpu().numpy()


def _poisoned(torch, c, shape_q):
    tdt = torch.float32 if c["f32"] else (torch.bfloat16 if c["fmt"] else torch.float16)
    return (torch.full(shape_q, vi.POISON, dtype=tdt, device="cuda"),
            torch.full((shape_q[1], shape_q[0]), vi.POISON, dtype=torch.float32, device="cuda"))


def _opts(torch, c, over):
    o = dict(window=c["W"], softcap=c["softcap"], sinks=c["sinks"], scale=c["scale"], causal=c["causal"])
    o.update(over)
    if not (o["sinks"] is None or hasattr(o["sinks"], "is_cuda")):
        o["sinks"] = _f32(torch, o["sinks"])
    return o


def _cache(torch, case, ps):
    """(K, V, table or None) on the device: the contiguous cache (ps = 0) or the pools of page size ps"""
    c = ci.make(case)
    if ps == 0:
        return cm.dev16(torch, c["kc"], c["fmt"]), cm.dev16(torch, c["vc"], c["fmt"]), None
    kp, vp, table = ci.paged(case, ps)
    return cm.dev16(torch, kp, c["fmt"]), cm.dev16(torch, vp, c["fmt"]), _i32(torch, table)


def _run(torch, fa, c, q, kc, vc, cu_q, lens, table, **over):
    """one launch into poisoned buffers -> (O, lse) device tensors; the case's options unless `over` replaces them"""
    out, lse = _poisoned(torch, c, tuple(q.shape))
    o2, l2 = fa.fa_forward_varlen_kvcache(q, kc, vc, cu_q, lens, block_table=table, out=out, lse=lse, **_opts(torch, c, over))
    torch.cuda.synchronize()
    assert o2 is out and l2 is lse
    return out, lse


def _packed(torch, fa, c, q, cu_q, **over):
    """fa_forward_varlen on the gathered packed K/V with the same keywords"""
    out, lse = _poisoned(torch, c, tuple(q.shape))
    k, v = cm.dev16(torch, c["kb"], c["fmt"]), cm.dev16(torch, c["vb"], c["fmt"])
    fa.fa_forward_varlen(q, k, v, cu_q, _i32(torch, c["cu_k"]), out=out, lse=lse, **_opts(torch, c, over))
    torch.cuda.synchronize()
    return out, lse


def _judge(c, o, lse, want, want_lse, cu_q, what):
    own = vi.owned(cu_q, o.shape[0])
    got, got_lse = _np(o), _np(lse)
    ma, rl, le = vi.figures(got, got_lse, want, want_lse, own)
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {cm.REL_L2[c['fmt']]:.1e} "
          f"{2 * cm.P_EPS[c['fmt']]:.2e})")
    found = vi.problems(got, got_lse, want, want_lse, own, c["fmt"])
    assert not found, f"{what}: {found}"


def _same(torch, a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ci.CASES, ids=ci.case_id)
def test_parity(fa, torch, case):
    """the contiguous form and the four page sizes against the float64 reference on the gathered keys; rows of no sequence keep the
    poison (vi.problems)"""
    c = ci.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    assert torch.isnan(q[-vi.TAIL:]).all()
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    want, want_lse = ci.expected(case)
    for ps in LAYOUTS:
        kc, vc, table = _cache(torch, case, ps)
        assert torch.isnan(kc).any() and torch.isnan(vc).any()
        o, lse = _run(torch, fa, c, q, kc, vc, cu_q, lens, table)
        _judge(c, o, lse, want, want_lse, c["cu_q"], f"{ci.case_id(case)} {'contiguous' if ps == 0 else 'pages of %d' % ps}")


# ---- 2. the packed entry's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ci.CASES[i] for i in (0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16)], ids=ci.case_id)
def test_bits_of_the_packed_entry(fa, torch, case):
    """O and lse are those of fa_forward_varlen(...) on the gathered packed K/V with the same keywords, plain and with options"""
    c = ci.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    ref = _packed(torch, fa, c, q, cu_q)
    for ps in (0, 16, 128):
        kc, vc, table = _cache(torch, case, ps)
        _same(torch, _run(torch, fa, c, q, kc, vc, cu_q, lens, table), ref, f"layout {ps}")


# ---- 3. paged against contiguous ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ci.CASES[i] for i in (2, 3, 6, 10, 13)], ids=ci.case_id)
def test_paged_is_the_contiguous_form_bit_for_bit(fa, torch, case):
    c = ci.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    kc, vc, _ = _cache(torch, case, 0)
    ref = _run(torch, fa, c, q, kc, vc, cu_q, lens, None)
    for ps in ci.PAGE_SIZES:
        kp, vp, table = _cache(torch, case, ps)
        _same(torch, _run(torch, fa, c, q, kp, vp, cu_q, lens, table), ref, f"pages of {ps}")


# ---- 4. census (exact) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,causal,d,fmt,W,snk,ps", [("chunk", 1, 64, 0, 0, 0, 16), ("chunk", 1, 128, 1, 100, 1, 32),
                                                         ("short", 0, 64, 1, 17, 1, 0), ("chunk", 0, 128, 0, 64, 0, 128),
                                                         ("short", 1, 128, 0, 1, 1, 16), ("chunk", 1, 64, 0, 400, 0, 64)])
def test_census(fa, torch, batch, causal, d, fmt, W, snk, ps):
    """scale 0 and one-hot V rows: every key of [lo_i, c_i) is counted exactly once and no other; with sinks alternating 0 and -inf a
    head divides by cnt + 1 resp. cnt.  With weights of exactly 1 the fp32 sums are exact, and both decisions -- the row total and
    exp(lse) -- are between neighbouring integers."""
    case = (batch, 2, 2, d, fmt, causal, 1, None, W, 0, snk)
    c = ci.make(case)
    Hq = 4
    sinks = np.array([0.0 if h % 2 == 0 else -np.inf for h in range(Hq)], np.float32) if snk else None
    one = vi.encode16(np.float32([1.0]), fmt)[0]
    lo0 = ci.lo0_of(c["lq"], c["lk"], W)
    vc = np.full(c["vc"].shape, cm.NAN16, np.uint16)
    for b, Lk in enumerate(c["lk"]):
        vc[b, :, lo0[b]:Lk] = 0
        for j in range(lo0[b], Lk):
            vc[b, :, j, (j + 7 * b) % d] = one
    kc = c["kc"]
    if ps:
        kc, vc, table = ci.scatter(kc, vc, c["lk"], lo0, ps, seed=77)
    q = cm.dev16(torch, c["qb"], fmt)
    o, lse = _run(torch, fa, c, q, cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), _i32(torch, c["cu_q"]), _i32(torch, c["lens"]),
                  _i32(torch, table) if ps else None, scale=0.0, sinks=sinks)
    got, got_lse = _np(o).astype(np.float64), _np(lse).astype(np.float64)
    worst = 0.0
    for b, (sq, eq) in enumerate(vi.bounds(c["cu_q"], q.shape[0])):
        lo, lim = li.limits(eq - sq, c["lk"][b], bool(causal), W)
        for i in range(eq - sq):
            cnt = max(int(lim[i] - lo[i]), 0)
            want = np.bincount((np.arange(lo[i], lim[i]) + 7 * b) % d, minlength=d) if cnt else np.zeros(d, np.int64)
            for hq in range(Hq):
                den = cnt + int(snk and np.isfinite(sinks[hq]))
                if den == 0:
                    assert (got[sq + i, hq] == 0).all() and got_lse[hq, sq + i] == -np.inf, (b, i, hq)
                    continue
                n = np.exp(got_lse[hq, sq + i])
                col = got[sq + i, hq] * den
                worst = max(worst, abs(n - den), float(np.abs(col - want).max()), abs(col.sum() - cnt))
                assert np.rint(n) == den and abs(n - den) < 0.25, (b, i, hq, n, den)
                assert (np.rint(col) == want).all() and abs(col.sum() - cnt) < 0.25, (b, i, hq)
    print(f"CENSUS|fa_forward_varlen_kvcache|{batch} causal={causal} d={d} {cm.FMT_NAME[fmt]} W={W} sinks={snk} ps={ps}|{worst:.3e}")
    own = vi.owned(c["cu_q"], q.shape[0])
    assert (got[~own] == vi.POISON).all() and (got_lse[:, ~own] == vi.POISON).all()


# ---- 5. clamps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", (0, 32))
def test_lengths_are_clamped_into_the_capacity(fa, torch, ps):
    """seqlens_k above Ncap counts as Ncap, a negative one as 0"""
    Hkv, G, d, fmt, Ncap = 2, 2, 64, 0, 256
    lq, raw, lk = (40, 70, 5), (10000, -5, 100), (256, 0, 100)
    q, qb = vi.packed(lq, Hkv * G, d, fmt, 81)
    k, kb = vi.packed(lk, Hkv, d, fmt, 82)
    v, vb = vi.packed(lk, Hkv, d, fmt, 83)
    cu_q, cu_k = vi.cu_of(lq), vi.cu_of(lk)
    kc, vc = (np.full((3, Hkv, Ncap, d), cm.NAN16, np.uint16) for _ in range(2))
    for b in range(3):
        kc[b, :, :lk[b]] = kb[cu_k[b]:cu_k[b + 1]].transpose(1, 0, 2)
        vc[b, :, :lk[b]] = vb[cu_k[b]:cu_k[b + 1]].transpose(1, 0, 2)
    table = None
    if ps:
        kc, vc, table = ci.scatter(kc, vc, lk, (0, 0, 0), ps, seed=5)
    c = dict(fmt=fmt, f32=True, W=0, softcap=0.0, sinks=None, scale=0.125, causal=True)
    for window in (0, 90):
        want, want_lse = li.varlen_logits_f64(q, k, v, cu_q, cu_k, Hkv, G, True, 0.125, W=window)
        o, lse = _run(torch, fa, c, cm.dev16(torch, qb, fmt), cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), _i32(torch, cu_q),
                      _i32(torch, raw), None if table is None else _i32(torch, table), window=window)
        _judge(c, o, lse, want, want_lse, cu_q, f"clamped lengths, layout {ps}, W={window}")


@pytest.mark.parametrize("case", (ci.CASES[0], ci.CASES[6]), ids=ci.case_id)
def test_a_live_entry_outside_the_pool_is_a_page_of_zeros(fa, torch, case):
    """two live table entries of the longest sequence are set outside [0, num_pages): the result is the reference with those key
    rows zeroed in K and V"""
    c = ci.make(case)
    ps, b = 16, 5
    kp, vp, table = ci.paged(case, ps)
    table = np.array(table)
    lo0 = ci.lo0_of(c["lq"], c["lk"], c["W"])[b]
    hit = (lo0 // ps + 1, (c["lk"][b] - 1) // ps)          # a whole page inside the visible range, and the last, partial one
    assert hit[0] < hit[1] and all(0 <= table[b, pi] < kp.shape[0] for pi in hit)
    table[b, hit[0]], table[b, hit[1]] = kp.shape[0], -3
    k, v = np.array(c["k"]), np.array(c["v"])
    for pi in hit:
        k[c["cu_k"][b] + pi * ps:min(c["cu_k"][b] + (pi + 1) * ps, c["cu_k"][b + 1])] = 0.0
        v[c["cu_k"][b] + pi * ps:min(c["cu_k"][b] + (pi + 1) * ps, c["cu_k"][b + 1])] = 0.0
    want, want_lse = li.varlen_logits_f64(c["q"], k, v, c["cu_q"], c["cu_k"], c["Hkv"], c["G"], c["causal"], c["scale"], W=c["W"],
                                          softcap=c["softcap"], sinks=c["sinks"])
    assert not np.array_equal(want, ci.expected(case)[0])
    o, lse = _run(torch, fa, c, cm.dev16(torch, c["qb"], c["fmt"]), cm.dev16(torch, kp, c["fmt"]), cm.dev16(torch, vp, c["fmt"]),
                  _i32(torch, c["cu_q"]), _i32(torch, c["lens"]), _i32(torch, table))
    _judge(c, o, lse, want, want_lse, c["cu_q"], f"{ci.case_id(case)} with two entries outside the pool")


# ---- 6. chunked prefill end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", (0, 100))
def test_chunked_prefill_is_the_one_shot_prefill(fa, torch, window):
    """one 300-token prompt fed as chunks (128, 100, 72) through fa_kvcache_append_paged + the entry (causal), concatenated, against ONE
    fa_forward_varlen causal over the whole prompt -- at the parity bounds: the chunk boundaries move rows between 128-row blocks, so
    the running-max history of a row, and with it bits, may differ"""
    Hkv, G, d, fmt, ps, N = 2, 2, 64, 0, 16, 300
    chunks = (128, 100, 72)
    q, qb = vi.packed((N,), Hkv * G, d, fmt, 91, tail=0)
    k, kb = vi.packed((N,), Hkv, d, fmt, 92, tail=0)
    v, vb = vi.packed((N,), Hkv, d, fmt, 93, tail=0)
    qd, kd, vd = (cm.dev16(torch, x, fmt) for x in (qb, kb, vb))
    max_pages = 20
    num_pages = max_pages + ci.SPARE
    perm = np.random.default_rng(94).permutation(num_pages)[:max_pages]
    nan = torch.tensor([cm.NAN16], dtype=torch.int16).view(torch.float16).cuda()
    k_pool = nan.expand(num_pages * Hkv * ps * d).reshape(num_pages, Hkv, ps, d).contiguous()
    v_pool = k_pool.clone()
    table = _i32(torch, perm[None, :])
    lens = _i32(torch, [0])
    outs, lses = [], []
    done = 0
    for n in chunks:
        k_new = kd[done:done + n].transpose(0, 1).contiguous()[None]
        v_new = vd[done:done + n].transpose(0, 1).contiguous()[None]
        fa.fa_kvcache_append_paged(k_new, v_new, k_pool, v_pool, table, cache_seqlens=lens, seqlens_out=lens)
        o, lse = fa.fa_forward_varlen_kvcache(qd[done:done + n].contiguous(), k_pool, v_pool, _i32(torch, [0, n]), lens, block_table=table,
                                              causal=True, return_lse=True, window=window)
        outs.append(o), lses.append(lse)
        done += n
    torch.cuda.synchronize()
    assert int(lens.item()) == N
    o, lse = torch.cat(outs, 0), torch.cat(lses, 1)
    cu = _i32(torch, [0, N])
    o1, l1 = fa.fa_forward_varlen(qd, kd, vd, cu, cu, causal=True, return_lse=True, window=window)
    torch.cuda.synchronize()
    c = dict(fmt=fmt)
    cu_np = np.array([0, N], np.int32)
    want, want_lse = li.varlen_logits_f64(q, k, v, cu_np, cu_np, Hkv, G, True, 1.0 / np.sqrt(d), W=window)
    _judge(c, o, lse, want, want_lse, cu_np, f"chunked prefill W={window} against float64")
    _judge(c, o, lse, _np(o1).astype(np.float64), _np(l1).astype(np.float64), cu_np, f"chunked prefill W={window} against one fa_forward_varlen")
    # the first chunk has no prefix: there the two calls stream the same tiles for the same rows
    assert torch.equal(o[:chunks[0]], o1[:chunks[0]]) and torch.equal(lse[:, :chunks[0]], l1[:, :chunks[0]])


# ---- 7. the torch op -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,ps", ((ci.CASES[0], 0), (ci.CASES[9], 16), (ci.CASES[7], 64)),
                         ids=lambda x: ci.case_id(x) if isinstance(x, tuple) else f"layout{x}")
def test_torch_op_returns_the_front_ends_bits(fa, torch, case, ps):
    from flashattention_kernel_project_amd.torch_op import register
    register()
    c = ci.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    kc, vc, table = _cache(torch, case, ps)
    o, lse = _run(torch, fa, c, q, kc, vc, cu_q, lens, table)
    o2, l2 = torch.ops.fa_mi355.forward_varlen_kvcache(q, kc, vc, cu_q, lens, table, c["scale"], c["causal"], c["W"],
                                                       _f32(torch, c["sinks"]), c["softcap"], c["f32"])
    torch.cuda.synchronize()
    own = torch.from_numpy(vi.owned(c["cu_q"], q.shape[0])).cuda()
    assert o2.dtype == o.dtype and torch.equal(o2[own], o[own]) and torch.equal(l2[:, own], lse[:, own])


# ---- 8. captured call ------------------------------------------------------------------------------------------------------------------
def test_captured_call_follows_rewritten_vectors_table_and_sinks(fa, torch):
    """a torch.cuda.graph capture replayed after cu_seqlens_q, cache_seqlens, block_table and sinks are rewritten in place equals a
    fresh call bit for bit"""
    case = ci.CASES[11]                    # short, causal, W = 100, sinks; a cache with no freed page is laid out below
    c = ci.make(case)
    ps = 32
    plain = ci.make(case[:8] + (0, 0, 0))  # the same keys (another seed) in a cache whose rows [0, Lk) all hold keys
    q = cm.dev16(torch, plain["qb"], c["fmt"])
    lo0 = [0] * len(plain["lk"])
    kp, vp, t0 = ci.scatter(plain["kc"], plain["vc"], plain["lk"], lo0, ps, seed=1)
    # the second state: other chunk lengths over the same total, shorter caches (a prefix of each sequence's keys), the table of the
    # first state with two sequences' rows exchanged -- their keys change -- and other sinks
    new_lq = (100, 64, 215, 0, 8, 128)     # sequence 3 keeps no row: the layout holds none of its keys (ci.lo0_of)
    new_q = vi.cu_of(new_lq)
    new_lens = np.array([0, 40, 33, 3, 36, 300], np.int32)
    t1 = np.array(t0)
    t1[[1, 4]] = t1[[4, 1]]
    new_s = np.array([-np.inf, 0.75, 2.5, 1.0], np.float32)
    assert new_q[-1] == c["cu_q"][-1] and new_s.shape == c["sinks"].shape and (new_lens <= plain["lens"]).all()
    assert new_lens[1] <= plain["lens"][4] and new_lens[4] <= plain["lens"][1]          # every key read is a key of the layout
    kd, vd = cm.dev16(torch, kp, c["fmt"]), cm.dev16(torch, vp, c["fmt"])
    cu_q, lens, table, sinks = _i32(torch, c["cu_q"]), _i32(torch, plain["lens"]), _i32(torch, t0), _f32(torch, c["sinks"])
    eager0 = _run(torch, fa, c, q, kd, vd, cu_q, lens, table, sinks=sinks)
    eager1 = _run(torch, fa, c, q, kd, vd, _i32(torch, new_q), _i32(torch, new_lens), _i32(torch, t1), sinks=new_s)
    assert not torch.equal(eager0[1], eager1[1])
    out, lse = _poisoned(torch, c, tuple(q.shape))
    kw = dict(block_table=table, causal=c["causal"], scale=c["scale"], window=c["W"], softcap=c["softcap"], sinks=sinks, out=out, lse=lse)
    fa.fa_forward_varlen_kvcache(q, kd, vd, cu_q, lens, **kw)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.fa_forward_varlen_kvcache(q, kd, vd, cu_q, lens, **kw)
    for vec_q, vec_l, tbl, vec_s, eager in ((c["cu_q"], plain["lens"], t0, c["sinks"], eager0), (new_q, new_lens, t1, new_s, eager1)):
        cu_q.copy_(_i32(torch, vec_q)), lens.copy_(_i32(torch, vec_l)), table.copy_(_i32(torch, tbl)), sinks.copy_(_f32(torch, vec_s))
        out.fill_(vi.POISON), lse.fill_(vi.POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(lse, eager[1])
    c2 = dict(c, q=plain["q"], cu_q=new_q, sinks=new_s)
    want, want_lse = ci.attend_f64(c2, ci.gather(kp, vp, t1, new_lens, new_lq, c["Hkv"], ps, c["fmt"]))
    _judge(c, out, lse, want, want_lse, new_q, "replayed on rewritten vectors, table and sinks")
