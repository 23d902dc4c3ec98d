"""GPU tier of fa_forward_varlen_kvcache_fp8 (the varlen prefill against an fp8 e4m3fn KV cache, contiguous or paged, with one scale
per K/V head), through the Python front end, which goes through the C ABI.  Inputs, the page layout and the float64 reference are
tests/varlen_cache_fp8_inputs.py's, the check is tests/varlen_inputs.py's; tests/test_varlen_cache_fp8_inputs.py shows without a GPU
that the check rejects seven wrong kernels (a scale dropped, swapped, indexed by the query head or applied to lse; the 16-bit row
pitch on the byte cache; the two widened halves of a load swapped).  Every cache holds the NaN code 0x7F in every row and page no
visible key lies in and garbage in every table entry nothing may read; every launch writes into O and lse buffers pre-filled with a
poison value."""
import numpy as np
import pytest

import common_inputs as cm
import fp8_inputs as f8
import varlen_cache_fp8_inputs as v8
import varlen_inputs as vi
import varlen_logit_inputs as li

pytestmark = pytest.mark.gpu
LAYOUTS = (0,) + v8.PAGE_SIZES          # 0: the contiguous cache
ONE8 = int(f8.encode(np.float32([1.0]))[0])


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _i32(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.int32)).cuda()


def _f32(torch, x):
    return x if x is None or hasattr(x, "is_cuda") else torch.from_numpy(np.asarray(x, np.float32)).cuda()


def _np(t):
    return t.float().cpu().numpy()


def _tdt(torch, fmt):
    return torch.bfloat16 if fmt else torch.float16


def _poisoned(torch, c, shape_q):
    tdt = torch.float32 if c["f32"] else _tdt(torch, c["fmt"])
    return (torch.full(shape_q, vi.POISON, dtype=tdt, device="cuda"),
            torch.full((shape_q[1], shape_q[0]), vi.POISON, dtype=torch.float32, device="cuda"))


def _opts(torch, c, over):
    o = dict(window=c["W"], softcap=c["softcap"], sinks=c["sinks"], scale=c["scale"], causal=c["causal"])
    o.update(over)
    o["sinks"] = _f32(torch, o["sinks"])
    return o


def _cache(torch, case, ps):
    """(K, V, table or None) on the device: the contiguous cache of codes (ps = 0) or the pools of page size ps"""
    c = v8.make(case)
    if ps == 0:
        return cm.dev8(torch, c["kc"]), cm.dev8(torch, c["vc"]), None
    kp, vp, table = v8.paged(case, ps)
    return cm.dev8(torch, kp), cm.dev8(torch, vp), _i32(torch, table)


def _run(torch, fa, c, q, kc, vc, cu_q, lens, table, **over):
    """one launch of the fp8 entry into poisoned buffers -> (O, lse) device tensors; the case's scales and options unless `over`
    replaces them (k_scale / v_scale None: null pointers)"""
    out, lse = _poisoned(torch, c, tuple(q.shape))
    ks, vs = (_f32(torch, over.pop(n, c.get(n))) for n in ("k_scale", "v_scale"))
    o2, l2 = fa.fa_forward_varlen_kvcache_fp8(q, kc, vc, cu_q, lens, block_table=table, k_scale=ks, v_scale=vs, out=out, lse=lse,
                                              **_opts(torch, c, over))
    torch.cuda.synchronize()
    assert o2 is out and l2 is lse
    return out, lse


def _run16(torch, fa, c, q, kc, vc, cu_q, lens, table, **over):
    """fa_forward_varlen_kvcache on a 16-bit cache with the same keywords"""
    out, lse = _poisoned(torch, c, tuple(q.shape))
    fa.fa_forward_varlen_kvcache(q, kc, vc, cu_q, lens, block_table=table, out=out, lse=lse, **_opts(torch, c, over))
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
@pytest.mark.parametrize("case", v8.CASES, ids=v8.case_id)
def test_parity(fa, torch, case):
    """the contiguous form and the four page sizes against the float64 reference on the decoded codes, at the 16-bit entry's bounds
    (the widening is exact); rows of no sequence keep the poison (vi.problems)"""
    c = v8.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    assert torch.isnan(q[-vi.TAIL:]).all()
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    want, want_lse = v8.expected(case)
    for ps in LAYOUTS:
        kc, vc, table = _cache(torch, case, ps)
        assert (kc.view(torch.uint8) == v8.NAN8).any() and (vc.view(torch.uint8) == v8.NAN8).any()
        o, lse = _run(torch, fa, c, q, kc, vc, cu_q, lens, table)
        _judge(c, o, lse, want, want_lse, c["cu_q"], f"{v8.case_id(case)} {'contiguous' if ps == 0 else 'pages of %d' % ps}")


# ---- 2. the 16-bit entry's bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", ("plain", "options"))
@pytest.mark.parametrize("d,fmt", ((64, 0), (128, 1)))
def test_bits_of_the_16_bit_entry(fa, torch, d, fmt, opts):
    """on caches that run through all 254 finite codes: with null scales O and lse are fa_forward_varlen_kvcache's on the cache widened
    by torch; k_scale = 2^-3 is the 16-bit call at scale * 2^-3; v_scale = 2^2 with fp32 output is 4 x the 16-bit O, lse equal"""
    Hkv, G = 2, 2
    lq, lk = v8.BATCHES["chunk"]
    q = cm.dev16(torch, vi.packed(lq, Hkv * G, d, fmt, 61)[1], fmt)
    cu_q, lens = _i32(torch, vi.cu_of(lq)), _i32(torch, lk)
    c = dict(fmt=fmt, f32=True, W=100 if opts == "options" else 0, softcap=li.SOFTCAP if opts == "options" else 0.0,
             sinks=li.sinks_for(Hkv * G) if opts == "options" else None, scale=1.0 / 64, causal=True, k_scale=None, v_scale=None)
    kc = f8.all_codes_cache(len(lk), Hkv, v8.NCAP, d, lk, 62)
    vc = f8.all_codes_cache(len(lk), Hkv, v8.NCAP, d, lk, 63)
    assert set(np.unique(kc[5, 0, :lk[5]])) == set(f8.FINITE_CODES.tolist())
    eighth, four = np.full(Hkv, 0.125, np.float32), np.full(Hkv, 4.0, np.float32)
    for ps in (0, 16, 128):
        table = None
        k8, v8_ = kc, vc
        if ps:
            k8, v8_, table = v8.scatter(kc, vc, lk, [0] * len(lk), ps, seed=64)
            table = _i32(torch, table)
        k8, v8_ = cm.dev8(torch, k8), cm.dev8(torch, v8_)
        k16, v16 = k8.to(_tdt(torch, fmt)), v8_.to(_tdt(torch, fmt))
        ref = _run16(torch, fa, c, q, k16, v16, cu_q, lens, table)
        assert not torch.isnan(ref[0][:-vi.TAIL]).any()
        _same(torch, _run(torch, fa, c, q, k8, v8_, cu_q, lens, table), ref, f"null scales, layout {ps}")
        _same(torch, _run(torch, fa, c, q, k8, v8_, cu_q, lens, table, k_scale=eighth),
              _run16(torch, fa, c, q, k16, v16, cu_q, lens, table, scale=c["scale"] * 0.125), f"k_scale 2^-3, layout {ps}")
        o, lse = _run(torch, fa, c, q, k8, v8_, cu_q, lens, table, v_scale=four)
        own = torch.from_numpy(vi.owned(vi.cu_of(lq), q.shape[0])).cuda()
        assert torch.equal(o[own], 4.0 * ref[0][own]) and torch.equal(o[~own], ref[0][~own]) and torch.equal(lse, ref[1]), \
            f"v_scale 2^2, layout {ps}"
        if opts == "plain" and ps == 0:      # and with a 16-bit output the null-scale bits hold too
            c16 = dict(c, f32=False)
            _same(torch, _run(torch, fa, c16, q, k8, v8_, cu_q, lens, table), _run16(torch, fa, c16, q, k16, v16, cu_q, lens, table), "o16")


# ---- 3. paged against contiguous ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [v8.CASES[i] for i in (1, 2, 5, 8, 11)], ids=v8.case_id)
def test_paged_is_the_contiguous_form_bit_for_bit(fa, torch, case):
    c = v8.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    kc, vc, _ = _cache(torch, case, 0)
    ref = _run(torch, fa, c, q, kc, vc, cu_q, lens, None)
    for ps in v8.PAGE_SIZES:
        kp, vp, table = _cache(torch, case, ps)
        _same(torch, _run(torch, fa, c, q, kp, vp, cu_q, lens, table), ref, f"pages of {ps}")


# ---- 4. null scales are ones ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,ps", ((v8.CASES[0], 0), (v8.CASES[6], 32), (v8.CASES[8], 128)),
                         ids=lambda x: v8.case_id(x) if isinstance(x, tuple) else f"layout{x}")
def test_null_scales_are_ones_bit_for_bit(fa, torch, case, ps):
    c = v8.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    kc, vc, table = _cache(torch, case, ps)
    ones = np.ones(c["Hkv"], np.float32)
    ref = _run(torch, fa, c, q, kc, vc, cu_q, lens, table, k_scale=ones, v_scale=ones)
    _same(torch, _run(torch, fa, c, q, kc, vc, cu_q, lens, table, k_scale=None, v_scale=None), ref, "both null")
    _same(torch, _run(torch, fa, c, q, kc, vc, cu_q, lens, table, k_scale=None, v_scale=ones), ref, "k_scale null")
    _same(torch, _run(torch, fa, c, q, kc, vc, cu_q, lens, table, k_scale=ones, v_scale=None), ref, "v_scale null")
    assert not torch.equal(_run(torch, fa, c, q, kc, vc, cu_q, lens, table)[0], ref[0])     # the case's own scales are not ones


# ---- 5. census (exact) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,causal,d,fmt,W,snk,ps", [("chunk", 1, 64, 0, 0, 0, 16), ("chunk", 1, 128, 1, 100, 1, 32),
                                                         ("short", 0, 64, 1, 17, 1, 0), ("chunk", 0, 128, 0, 1, 0, 128),
                                                         ("short", 1, 128, 0, 400, 1, 64)])
def test_census(fa, torch, batch, causal, d, fmt, W, snk, ps):
    """scale 0 with k_scale 0.5 -- the clamp applies to the product -- and one-hot V rows (the code of 1.0): every key of [lo_i, c_i) is
    counted exactly once and no other; with sinks alternating 0 and -inf a head divides by cnt + 1 resp. cnt.  With weights of exactly 1
    the fp32 sums are exact, and both decisions -- the row total and exp(lse) -- are between neighbouring integers."""
    case = (batch, 2, 2, d, fmt, causal, 1, None, W, 0, snk)
    c = v8.make(case)
    Hq = 4
    sinks = np.array([0.0 if h % 2 == 0 else -np.inf for h in range(Hq)], np.float32) if snk else None
    lo0 = v8.lo0_of(c["lq"], c["lk"], W)
    vc = np.full(c["vc"].shape, v8.NAN8, np.uint8)
    for b, Lk in enumerate(c["lk"]):
        vc[b, :, lo0[b]:Lk] = 0
        for j in range(lo0[b], Lk):
            vc[b, :, j, (j + 7 * b) % d] = ONE8
    kc = c["kc"]
    if ps:
        kc, vc, table = v8.scatter(kc, vc, c["lk"], lo0, ps, seed=77)
    q = cm.dev16(torch, c["qb"], fmt)
    o, lse = _run(torch, fa, c, q, cm.dev8(torch, kc), cm.dev8(torch, vc), _i32(torch, c["cu_q"]), _i32(torch, c["lens"]),
                  _i32(torch, table) if ps else None, scale=0.0, sinks=sinks, k_scale=np.full(2, 0.5, np.float32), v_scale=None)
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
    print(f"CENSUS|fa_forward_varlen_kvcache_fp8|{batch} causal={causal} d={d} {cm.FMT_NAME[fmt]} W={W} sinks={snk} ps={ps}|{worst:.3e}")
    own = vi.owned(c["cu_q"], q.shape[0])
    assert (got[~own] == vi.POISON).all() and (got_lse[:, ~own] == vi.POISON).all()


# ---- 6. the fp8 decode entries as a second oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,ps", ((v8.CASES[0], 0), (v8.CASES[3], 16), (v8.CASES[6], 64), (v8.CASES[8], 0), (v8.CASES[11], 32)),
                         ids=lambda x: v8.case_id(x) if isinstance(x, tuple) else f"layout{x}")
def test_the_fp8_decode_entries_agree(fa, torch, oracle, case, ps):
    """fa_forward_kvcache_fp8 / _paged_fp8 with seqlens_q on the same cache, scales and options: other kernels (128-row blocks of
    G * n packed rows, split-KV), the same function"""
    c = v8.make(case)
    Hq, d, B, Nq = c["Hkv"] * c["G"], c["d"], len(c["lq"]), max(c["lq"])
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    kc, vc, table = _cache(torch, case, ps)
    o, lse = _run(torch, fa, c, q, kc, vc, cu_q, lens, table)
    q4 = torch.zeros(B, Hq, Nq, d, dtype=q.dtype, device="cuda")
    got, got_lse = np.zeros((B, Hq, Nq, d), np.float32), np.full((B, Hq, Nq), -np.inf, np.float32)
    on, ln = _np(o), _np(lse)
    for b, (s, e) in enumerate(vi.bounds(c["cu_q"], q.shape[0])):
        q4[b, :, :e - s] = q[s:e].transpose(0, 1)
        got[b, :, :e - s] = on[s:e].transpose(1, 0, 2)
        got_lse[b, :, :e - s] = ln[:, s:e]
    kw = dict(k_scale=_f32(torch, c["k_scale"]), v_scale=_f32(torch, c["v_scale"]), cache_seqlens=lens, causal=c["causal"],
              scale=c["scale"], out_dtype=o.dtype, return_lse=True, window=c["W"], sinks=_f32(torch, c["sinks"]), softcap=c["softcap"],
              seqlens_q=_i32(torch, c["lq"]))
    if ps:
        o2, l2 = fa.fa_forward_kvcache_paged_fp8(q4, kc, vc, table, **kw)
    else:
        o2, l2 = fa.fa_forward_kvcache_fp8(q4, kc, vc, **kw)
    torch.cuda.synchronize()
    cm.check_decode(oracle, got.reshape(B * Hq, Nq, d), got_lse.reshape(B * Hq, Nq).astype(np.float64),
                    _np(o2).reshape(B * Hq, Nq, d), _np(l2).reshape(B * Hq, Nq).astype(np.float64), c["fmt"],
                    f"{v8.case_id(case)} layout {ps} against the decode entry")


# ---- 7. chunked prefill end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,window", ((16, 0), (16, 50), (0, 0), (0, 50)))
def test_chunked_prefill_through_the_fp8_append(fa, torch, ps, window):
    """three prompts fed as two ragged chunks each through fa_kvcache_append_paged_fp8 (ps = 0: fa_kvcache_append_fp8 on a contiguous
    cache), each append followed by the prefill of that chunk (causal): against the float64 reference on numpy's encoding of the same
    rows"""
    Hkv, G, d, fmt, B, Ncap = 2, 2, 64, 0, 3, 256
    chunks = ((100, 1, 64), (77, 129, 0))
    total = tuple(a + b for a, b in zip(*chunks))
    ks, vs = v8.scales_for(Hkv)
    k, kb = vi.packed(total, Hkv, d, fmt, 92, tail=0)
    v, vb = vi.packed(total, Hkv, d, fmt, 93, tail=0)
    k8 = f8.encode(k / ks[None, :, None])
    v8_ = f8.encode(v / vs[None, :, None])
    cu_t = vi.cu_of(total)
    ksd, vsd = _f32(torch, ks), _f32(torch, vs)
    if ps:
        max_pages = Ncap // ps
        num_pages = B * max_pages + 3
        table = _i32(torch, np.random.default_rng(94).permutation(num_pages)[:B * max_pages].reshape(B, max_pages))
        shape = (num_pages, Hkv, ps, d)
    else:
        table, shape = None, (B, Hkv, Ncap, d)
    k_cache = torch.full(shape, v8.NAN8, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
    v_cache = k_cache.clone()
    lens = _i32(torch, [0] * B)
    done = [0] * B
    for step, lq in enumerate(chunks):
        Nnew = max(lq)
        k_new, v_new = (torch.zeros(B, Hkv, Nnew, d, dtype=torch.float16, device="cuda") for _ in range(2))
        for b in range(B):
            rows = slice(cu_t[b] + done[b], cu_t[b] + done[b] + lq[b])
            k_new[b, :, :lq[b]] = cm.dev16(torch, kb[rows], fmt).transpose(0, 1)
            v_new[b, :, :lq[b]] = cm.dev16(torch, vb[rows], fmt).transpose(0, 1)
        new = _i32(torch, lq)
        if ps:
            fa.fa_kvcache_append_paged_fp8(k_new, v_new, k_cache, v_cache, table, ksd, vsd, cache_seqlens=lens, seqlens_out=lens,
                                           seqlens_new=new)
        else:
            fa.fa_kvcache_append_fp8(k_new, v_new, k_cache, v_cache, ksd, vsd, cache_seqlens=lens, seqlens_out=lens, seqlens_new=new)
        done = [a + n for a, n in zip(done, lq)]
        q, qb = vi.packed(lq, Hkv * G, d, fmt, 95 + step)
        c = dict(q=q, Hkv=Hkv, G=G, d=d, fmt=fmt, f32=True, causal=True, scale=1.0 / np.sqrt(d), W=window, softcap=0.0, sinks=None,
                 k_scale=ks, v_scale=vs, cu_q=vi.cu_of(lq), cu_k=vi.cu_of(done))
        # the keys so far, from numpy's codes
        c["k"] = np.concatenate([f8.decode(k8[cu_t[b]:cu_t[b] + done[b]]) for b in range(B)] + [np.full((vi.TAIL, Hkv, d), np.nan, np.float32)])
        c["v"] = np.concatenate([f8.decode(v8_[cu_t[b]:cu_t[b] + done[b]]) for b in range(B)] + [np.full((vi.TAIL, Hkv, d), np.nan, np.float32)])
        o, lse = _run(torch, fa, c, cm.dev16(torch, qb, fmt), k_cache, v_cache, _i32(torch, c["cu_q"]), lens, table)
        assert lens.cpu().tolist() == done
        want, want_lse = v8.reference_f64(c)
        _judge(c, o, lse, want, want_lse, c["cu_q"], f"chunk {step} through the append, layout {ps}, W={window}")


# ---- 8. clamps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", (0, 32))
def test_lengths_are_clamped_into_the_capacity(fa, torch, ps):
    """seqlens_k above Ncap counts as Ncap, a negative one as 0"""
    Hkv, G, d, fmt, Ncap = 2, 2, 64, 0, 256
    lq, raw, lk = (40, 70, 5), (10000, -5, 100), (256, 0, 100)
    ks, vs = v8.scales_for(Hkv)
    q, qb = vi.packed(lq, Hkv * G, d, fmt, 81)
    k8, v8_ = v8.packed8(lk, Hkv, d, ks, 82), v8.packed8(lk, Hkv, d, vs, 83)
    cu_q, cu_k = vi.cu_of(lq), vi.cu_of(lk)
    kc, vc = v8.cache_of(k8, cu_k, lq, lk, 0, Ncap), v8.cache_of(v8_, cu_k, lq, lk, 0, Ncap)
    table = None
    if ps:
        kc, vc, table = v8.scatter(kc, vc, lk, (0, 0, 0), ps, seed=5)
    for window in (0, 90):
        c = dict(q=q, k=f8.decode(k8), v=f8.decode(v8_), cu_q=cu_q, cu_k=cu_k, Hkv=Hkv, G=G, fmt=fmt, f32=True, W=window, softcap=0.0,
                 sinks=None, scale=0.125, causal=True, k_scale=ks, v_scale=vs)
        want, want_lse = v8.reference_f64(c)
        o, lse = _run(torch, fa, c, cm.dev16(torch, qb, fmt), cm.dev8(torch, kc), cm.dev8(torch, vc), _i32(torch, cu_q),
                      _i32(torch, raw), None if table is None else _i32(torch, table))
        _judge(c, o, lse, want, want_lse, cu_q, f"clamped lengths, layout {ps}, W={window}")


@pytest.mark.parametrize("case", (v8.CASES[0], v8.CASES[5]), ids=v8.case_id)
def test_a_live_entry_outside_the_pool_is_a_page_of_zeros(fa, torch, case):
    """two live table entries of the longest sequence are set outside [0, num_pages): the result is the reference with those key
    rows zeroed in K and V"""
    c = v8.make(case)
    ps, b = 16, 5
    kp, vp, table = v8.paged(case, ps)
    table = np.array(table)
    lo0 = v8.lo0_of(c["lq"], c["lk"], c["W"])[b]
    hit = (lo0 // ps + 1, (c["lk"][b] - 1) // ps)          # a whole page inside the visible range, and the last, partial one
    assert hit[0] < hit[1] and all(0 <= table[b, pi] < kp.shape[0] for pi in hit)
    table[b, hit[0]], table[b, hit[1]] = kp.shape[0], -3
    k, v = np.array(c["k"]), np.array(c["v"])
    for pi in hit:
        k[c["cu_k"][b] + pi * ps:min(c["cu_k"][b] + (pi + 1) * ps, c["cu_k"][b + 1])] = 0.0
        v[c["cu_k"][b] + pi * ps:min(c["cu_k"][b] + (pi + 1) * ps, c["cu_k"][b + 1])] = 0.0
    want, want_lse = v8.reference_f64(dict(c, k=k, v=v))
    assert not np.array_equal(want, v8.expected(case)[0])
    o, lse = _run(torch, fa, c, cm.dev16(torch, c["qb"], c["fmt"]), cm.dev8(torch, kp), cm.dev8(torch, vp), _i32(torch, c["cu_q"]),
                  _i32(torch, c["lens"]), _i32(torch, table))
    _judge(c, o, lse, want, want_lse, c["cu_q"], f"{v8.case_id(case)} with two entries outside the pool")


# ---- 9. the torch op and the captured call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,ps", ((v8.CASES[1], 0), (v8.CASES[8], 16)),
                         ids=lambda x: v8.case_id(x) if isinstance(x, tuple) else f"layout{x}")
def test_torch_op_returns_the_front_ends_bits(fa, torch, case, ps):
    from flashattention_kernel_project_amd.torch_op import register
    register()
    c = v8.make(case)
    q = cm.dev16(torch, c["qb"], c["fmt"])
    cu_q, lens = _i32(torch, c["cu_q"]), _i32(torch, c["lens"])
    kc, vc, table = _cache(torch, case, ps)
    o, lse = _run(torch, fa, c, q, kc, vc, cu_q, lens, table)
    o2, l2 = torch.ops.fa_mi355.forward_varlen_kvcache_fp8(q, kc, vc, cu_q, lens, table, _f32(torch, c["k_scale"]),
                                                           _f32(torch, c["v_scale"]), c["scale"], c["causal"], c["W"],
                                                           _f32(torch, c["sinks"]), c["softcap"], c["f32"])
    torch.cuda.synchronize()
    own = torch.from_numpy(vi.owned(c["cu_q"], q.shape[0])).cuda()
    assert o2.dtype == o.dtype and torch.equal(o2[own], o[own]) and torch.equal(l2[:, own], lse[:, own])


def test_captured_call_follows_rewritten_lengths_table_scales_and_sinks(fa, torch):
    """a torch.cuda.graph capture (one stream, after a warm-up call) replayed after cache_seqlens, block_table, both scales and sinks
    are rewritten in place equals a fresh call bit for bit"""
    case = ("short", 2, 2, 64, 0, 1, 1, None, 100, 0, 1)
    c = v8.make(case)
    ps = 32
    plain = v8.make(case[:8] + (0, 0, 0))  # the same geometry in a cache whose rows [0, Lk) all hold keys
    q = cm.dev16(torch, plain["qb"], c["fmt"])
    kp, vp, t0 = v8.scatter(plain["kc"], plain["vc"], plain["lk"], [0] * len(plain["lk"]), ps, seed=1)
    # the second state: shorter caches (a prefix of each sequence's keys), the table with two sequences' rows exchanged -- their keys
    # change -- other scales and other sinks
    new_lens = np.array([0, 40, 33, 3, 36, 300], np.int32)
    t1 = np.array(t0)
    t1[[1, 4]] = t1[[4, 1]]
    new_s = np.array([-np.inf, 0.75, 2.5, 1.0], np.float32)
    new_ks, new_vs = np.array([1.25, 0.5], np.float32), np.array([0.875, 3.0], np.float32)
    assert new_s.shape == c["sinks"].shape and (new_lens <= plain["lens"]).all()
    assert new_lens[1] <= plain["lens"][4] and new_lens[4] <= plain["lens"][1]          # every key read is a key of the layout
    kd, vd = cm.dev8(torch, kp), cm.dev8(torch, vp)
    cu_q = _i32(torch, c["cu_q"])
    lens, table, sinks = _i32(torch, plain["lens"]), _i32(torch, t0), _f32(torch, c["sinks"])
    ksd, vsd = _f32(torch, c["k_scale"]), _f32(torch, c["v_scale"])
    eager0 = _run(torch, fa, c, q, kd, vd, cu_q, lens, table)
    eager1 = _run(torch, fa, c, q, kd, vd, cu_q, _i32(torch, new_lens), _i32(torch, t1), sinks=new_s, k_scale=new_ks, v_scale=new_vs)
    assert not torch.equal(eager0[1], eager1[1])
    out, lse = _poisoned(torch, c, tuple(q.shape))
    kw = dict(block_table=table, k_scale=ksd, v_scale=vsd, causal=c["causal"], scale=c["scale"], window=c["W"], softcap=c["softcap"],
              sinks=sinks, out=out, lse=lse)
    fa.fa_forward_varlen_kvcache_fp8(q, kd, vd, cu_q, lens, **kw)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.fa_forward_varlen_kvcache_fp8(q, kd, vd, cu_q, lens, **kw)
    for vec_l, tbl, vec_s, k_s, v_s, eager in ((plain["lens"], t0, c["sinks"], c["k_scale"], c["v_scale"], eager0),
                                               (new_lens, t1, new_s, new_ks, new_vs, eager1)):
        lens.copy_(_i32(torch, vec_l)), table.copy_(_i32(torch, tbl)), sinks.copy_(_f32(torch, vec_s))
        ksd.copy_(_f32(torch, k_s)), vsd.copy_(_f32(torch, v_s))
        out.fill_(vi.POISON), lse.fill_(vi.POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(lse, eager[1])
    c2 = dict(c, q=plain["q"], sinks=new_s, k_scale=new_ks, v_scale=new_vs)
    want, want_lse = v8.attend(c2, v8.gather(kp, vp, t1, new_lens, c["Hkv"], ps))
    _judge(c, out, lse, want, want_lse, c["cu_q"], "replayed on rewritten lengths, table, scales and sinks")
