"""GPU tier of the token-packed decode entry fa_kvcache_decode_varlen (fa.fa_kvcache_decode_varlen, _fp8).

Inputs, packing, the float64 reference and the check are tests/decode_varlen_inputs.py's (its CPU tier shows that six numpy "wrong
kernels" fail that check).  Bounds are the project's: cm.MAX_ABS and cm.REL_L2 on O, 2 * cm.P_EPS absolute on the lse of live rows
with a key, exact 0 / -inf on rows without one.  The bit ties are against the padded entry, fa_forward_kvcache*(seqlens_q=n_b) with
Nq = max_q on the padded copy of the same rows.  The census is left out: the bit tie to the padded entry, which has one, covers it.

Poison: O and lse are pre-filled with sentinels, the workspace with NaN bytes; every cache row at or past L_b holds NaN bit patterns;
every pool page no table names holds NaN; every table entry past the live pages holds garbage.
"""
import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv
import fp8_inputs as f8
import logit_inputs as li
import ragged_inputs as ri
import rope_inputs as rp

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
MASKS = [pytest.param(c, W, id=f"{'causal' if c else 'full'}-W{W}") for c in (True, False) for W in ri.WINDOWS]
KS, VS = (0.5, 0.75, 1.25), (2.0, 1.5, 0.37)   # per-head scales, the first Hkv of each


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ints(torch, values):
    return None if values is None else torch.tensor([int(x) for x in values], dtype=torch.int32, device="cuda")


def _floats(torch, values):
    return None if values is None else torch.tensor(np.asarray(values, np.float32), dtype=torch.float32, device="cuda")


def _sentinel_out(torch, shape, out_dtype):
    """O with the sentinel bit pattern in every element, lse-like sentinels are made by the caller"""
    if out_dtype == torch.float32:
        return torch.full(shape, dv.SENTINEL_O32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, dv.SENTINEL_O16, dtype=torch.int16, device="cuda").view(out_dtype)


def _bits(torch, t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Case:
    """The device tensors of one (family, d, fmt, cache form): made once, used by the packed and the padded call"""

    def __init__(self, oracle, torch, name, d, fmt, ps=0, fp8=False, seed=0):
        self.f, self.lay, self.name, self.d, self.fmt, self.ps, self.fp8 = dv.family(name), dv.layout(name), name, d, fmt, ps, fp8
        B, Hkv, G, Nq, Ncap = ri.shape(self.f)
        (_, k, v), (qb, kb, vb) = dv.inputs(oracle, name, d, fmt)
        self.qb = qb
        lens = self.f["lens"]
        if fp8:
            kb, vb, nan, dev = f8.encode(k), f8.encode(v), f8.NAN_CODES[0], lambda a: cm.dev8(torch, a)
            self.scales = (_floats(torch, KS[:Hkv]), _floats(torch, VS[:Hkv]))
        else:
            nan, dev = cm.NAN16, lambda a: cm.dev16(torch, a, fmt)
        kc, vc = (x.reshape(B, Hkv, Ncap, d) for x in (kb, vb))
        if ps:
            kp, vp, table = cm.scatter(kc, vc, lens, ps, seed, nan=nan)
            self.k, self.v, self.table = dev(kp), dev(vp), torch.from_numpy(table).cuda()
        else:
            self.k, self.v, self.table = dev(cm.poisoned(kc, lens, nan=nan)), dev(cm.poisoned(vc, lens, nan=nan)), None
        self.lens = _ints(torch, lens)
        self.tdt = torch.bfloat16 if fmt else torch.float16

    def need(self, fa, W):
        B, Hkv, G, Nq, Ncap = ri.shape(self.f)
        kw = dict(max_pages=Ncap // self.ps, page_size=self.ps) if self.ps else dict(Ncap=Ncap)
        need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, self.lay.max_q, self.d, window=W, **kw)
        assert di.splits_of(need, B * Hkv, G * Nq, self.d) == dv.want_S(self.name, W)
        return need

    def packed(self, fa, torch, W, causal, variant="none", out_dtype=None, poison=False, q=None, out=None, lse=None, cu=None, total_q=None):
        """the entry under test -> (O [total_q, Hq, d], lse [Hq, total_q]), both pre-filled with the sentinels unless given"""
        B, Hkv, G, Nq, Ncap = ri.shape(self.f)
        Hq, lay = Hkv * G, self.lay
        out_dtype = out_dtype or torch.float32
        total_q = total_q or lay.total_q
        if q is None:
            q = cm.dev16(torch, dv.pack_rows(lay, self.qb, cm.NAN16 if poison else 0), self.fmt)
        if out is None:
            out = _sentinel_out(torch, (total_q, Hq, self.d), out_dtype)
        if lse is None:
            lse = torch.full((Hq, total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
        sinks, softcap = li.options(variant, Hq)
        ws = torch.full((max(self.need(fa, W), 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN
        kw = dict(cache_seqlens=self.lens, block_table=self.table, causal=causal, out=out, lse=lse, workspace=ws, window=W,
                  softcap=softcap, sinks=_floats(torch, sinks))
        cu = _ints(torch, lay.cu if cu is None else cu)
        if self.fp8:
            o, l = fa.fa_kvcache_decode_varlen_fp8(q, self.k, self.v, cu, lay.max_q, k_scale=self.scales[0], v_scale=self.scales[1], **kw)
        else:
            o, l = fa.fa_kvcache_decode_varlen(q, self.k, self.v, cu, lay.max_q, **kw)
        torch.cuda.synchronize()
        assert o.data_ptr() == out.data_ptr() and l.data_ptr() == lse.data_ptr() and o.dtype == out_dtype
        return o, l

    def padded(self, fa, torch, W, causal, variant="none", out_dtype=None):
        """fa_kvcache_decode with seqlens_q = n_b and Nq = max_q on the padded head-major copy -> (O [B, Hq, Nq, d], lse [B, Hq, Nq])"""
        B, Hkv, G, Nq, Ncap = ri.shape(self.f)
        Hq = Hkv * G
        sinks, softcap = li.options(variant, Hq)
        dq = cm.dev16(torch, self.qb, self.fmt).view(B, Hq, Nq, self.d)
        need = fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, self.d, W)
        kw = dict(cache_seqlens=self.lens, causal=causal, return_lse=True, window=W, sinks=_floats(torch, sinks), softcap=softcap,
                  workspace=torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda"), seqlens_q=_ints(torch, self.lay.n),
                  out_dtype=out_dtype or torch.float32)
        if self.fp8:
            kw.update(k_scale=self.scales[0], v_scale=self.scales[1])
        fn = getattr(fa, "fa_forward_kvcache" + ("_paged" if self.ps else "") + ("_fp8" if self.fp8 else ""))
        args = (dq, self.k, self.v) + ((self.table,) if self.ps else ())
        o, l = fn(*args, **kw)
        torch.cuda.synchronize()
        return o, l


def _live_index(torch, lay):
    b, i = np.nonzero(lay.tok >= 0)
    return torch.from_numpy(b).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(lay.tok[b, i]).cuda()


def _same_as_padded(torch, lay, packed, padded, what):
    """torch.equal on O and lse of the live rows: packed (O [T, Hq, d], lse [Hq, T]) against padded (O [B, Hq, Nq, d], lse [B, Hq, Nq])"""
    b, i, t = _live_index(torch, lay)
    assert len(t) > 0
    o, l = packed[0][t], packed[1].t()[t]                                   # [live, Hq, d], [live, Hq]
    po, pl = padded[0].permute(0, 2, 1, 3)[b, i], padded[1].permute(0, 2, 1)[b, i]
    assert torch.isfinite(po).all() and not torch.isnan(pl).any(), what
    assert torch.equal(o, po), f"{what}: O differs from the padded entry's in {int((o != po).sum())} places"
    assert torch.equal(l, pl), f"{what}: lse differs from the padded entry's in {int((l != pl).sum())} places"


def _free_tokens_hold_the_sentinel(torch, lay, o, lse, what):
    free = torch.from_numpy(~lay.owned).cuda()
    want = dv.SENTINEL_O32 if o.dtype == torch.float32 else dv.SENTINEL_O16
    assert (_bits(torch, o[free]) == want).all(), what + ": an O row of no sequence was written"
    assert (lse[:, free] == dv.SENTINEL_LSE).all(), what + ": an lse entry of no sequence was written"


def _pages(f):
    return [ps for ps in (16, 256) if f["Ncap"] % ps == 0]


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal,W", MASKS)
@pytest.mark.parametrize("name", dv.NAMES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity(fa, oracle, torch_cuda, fmt, d, name, causal, W):
    torch = torch_cuda
    case = Case(oracle, torch, name, d, fmt)
    if name == "split" and W == 0:   # (a window of 100 keys is one pass on any capacity)
        assert dv.want_S(name, W) > 1 and case.need(fa, W) > 0   # behind the merge
    want, want_lse = dv.reference(oracle, name, d, fmt, W, causal)
    o, lse = case.packed(fa, torch, W, causal)
    dv.check(oracle, case.lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"{name} {'causal' if causal else 'full'} W={W}")


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity_with_sinks_softcap_and_fp8_scales(fa, oracle, torch_cuda, fmt, d):
    torch = torch_cuda
    for name, causal, W in (("spec", True, 100), ("split", True, 0), ("overlong", False, 0)):
        f = dv.family(name)
        B, Hkv, G, Nq, Ncap = ri.shape(f)
        want, want_lse = dv.reference(oracle, name, d, fmt, W, causal, "both")
        o, lse = Case(oracle, torch, name, d, fmt).packed(fa, torch, W, causal, "both", poison=True)
        dv.check(oracle, dv.layout(name), o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"{name} sinks + softcap")
        # an fp8 cache with per-head scales: the reference on the dequantised cache
        (q, k, v), _ = dv.inputs(oracle, name, d, fmt)
        kd = f8.decode(f8.encode(k)) * np.tile(np.array(KS[:Hkv], np.float32), B)[:, None, None]
        vd = f8.decode(f8.encode(v)) * np.tile(np.array(VS[:Hkv], np.float32), B)[:, None, None]
        want, want_lse = cm.expected_f64(q, kd, vd, f["lens"], B, Hkv, G, Nq, causal, W, nq=f["nq"])
        o, lse = Case(oracle, torch, name, d, fmt, fp8=True).packed(fa, torch, W, causal)
        dv.check(oracle, dv.layout(name), o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"{name} fp8 per-head scales")


# ---- 2. the bits of the padded entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dv.NAMES + ["tail"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bits_of_the_padded_entry(fa, oracle, torch_cuda, fmt, d, name):
    """contiguous, pages of 16 and 256 where they divide the capacity, fp8 with non-unit scales (contiguous and pages of 16); plain and
    with sinks + soft-cap; fp32 and 16-bit outputs.  `tail`: every n_b = max_q, with a partly filled last wave."""
    torch, f = torch_cuda, dv.family(name)
    tdt = torch.bfloat16 if fmt else torch.float16
    forms = [(0, False)] + [(ps, False) for ps in _pages(f)] + [(0, True)] + [(ps, True) for ps in _pages(f)[:1]]
    for ps, fp8 in forms:
        case = Case(oracle, torch, name, d, fmt, ps=ps, fp8=fp8, seed=ps + 1)
        for causal, W, variant, out_dtype in ((True, 0, "none", torch.float32), (True, 100, "both", tdt), (False, 0, "both", torch.float32),
                                              (False, 100, "none", tdt)):
            what = f"{name} ps={ps} fp8={fp8} causal={causal} W={W} {variant} {out_dtype}"
            got = case.packed(fa, torch, W, causal, variant, out_dtype)
            _same_as_padded(torch, case.lay, got, case.padded(fa, torch, W, causal, variant, out_dtype), what)
            _free_tokens_hold_the_sentinel(torch, case.lay, *got, what)


# ---- 3. untouched tokens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spec", "overlong", "split"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_tokens_of_no_sequence_are_neither_read_nor_written(fa, oracle, torch_cuda, fmt, d, name):
    """S = 1 (spec, overlong) and S > 1 (split): NaN in the Q row of every token that is no live row -- the lead, the holes, the trail,
    the rows past max_q of an over-long sequence -- changes no bit of a live row, and those tokens' O rows and lse entries keep the
    sentinel"""
    torch = torch_cuda
    tdt = torch.bfloat16 if fmt else torch.float16
    assert (dv.want_S(name, 0) > 1) == (name == "split")
    for ps in [0] + _pages(dv.family(name))[:1]:
        case = Case(oracle, torch, name, d, fmt, ps=ps, seed=3)
        for out_dtype in (torch.float32, tdt):
            clean = case.packed(fa, torch, 0, True, "sinks", out_dtype)
            dirty = case.packed(fa, torch, 0, True, "sinks", out_dtype, poison=True)
            for x, y, n in zip(dirty, clean, ("O", "lse")):
                assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{name} ps={ps}: {n} moved under NaN in the free tokens' Q rows"
            _free_tokens_hold_the_sentinel(torch, case.lay, *dirty, f"{name} ps={ps} {out_dtype}")
            t = _live_index(torch, case.lay)[2]
            assert torch.isfinite(dirty[0][t]).all() and not torch.isnan(dirty[1][:, t]).any()


# ---- 4. views ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spec", "split"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_strided_views(fa, oracle, torch_cuda, fmt, d, name):
    torch = torch_cuda
    case = Case(oracle, torch, name, d, fmt)
    B, Hkv, G, Nq, Ncap = ri.shape(case.f)
    Hq, T = Hkv * G, case.lay.total_q
    tdt = case.tdt
    q = cm.dev16(torch, dv.pack_rows(case.lay, case.qb, cm.NAN16), fmt)
    base = case.packed(fa, torch, 100, True, "both", tdt, q=q)
    # Q as the Q slice of a fused (total, Hq + 2 Hkv, d) buffer whose K and V parts hold NaN
    fused = torch.full((T, Hq + 2 * Hkv, d), float("nan"), dtype=tdt, device="cuda")
    fused[:, :Hq] = q
    got = case.packed(fa, torch, 100, True, "both", tdt, q=fused[:, :Hq])
    assert not fused[:, :Hq].is_contiguous()
    # a head-major Q: (Hq, total, d) seen token-major
    hm = q.transpose(0, 1).contiguous().transpose(0, 1)
    assert hm.stride(0) == d and hm.stride(1) == T * d
    got_hm = case.packed(fa, torch, 100, True, "both", tdt, q=hm)
    # out= as a slice of a wider tensor, along the heads and along the tokens
    wide = _sentinel_out(torch, (T + 4, Hq + 3, d), tdt)
    before = _bits(torch, wide).clone()
    got_out = case.packed(fa, torch, 100, True, "both", tdt, q=q, out=wide[3:3 + T, 2:2 + Hq])
    for g, what in ((got, "fused Q"), (got_hm, "head-major Q"), (got_out, "out= slice")):
        for x, y, n in zip(g, base, ("O", "lse")):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{what}: {n} differs from the contiguous call"
    after = _bits(torch, wide)
    inside = torch.zeros_like(after, dtype=torch.bool)
    inside[3:3 + T, 2:2 + Hq] = True
    assert torch.equal(after[~inside], before[~inside]), "bytes outside the out= slice changed"


# ---- 5. clamps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_clamps_of_cu_seqlens_q(fa, oracle, torch_cuda, fmt, d):
    """a negative entry, a decreasing pair and an entry beyond total_q, on overlong's caches (B = 4, max_q = 4): the result is the call
    on the clamped vector, and nothing outside O and lse is written (guard rows around both allocations)"""
    torch = torch_cuda
    case = Case(oracle, torch, "overlong", d, fmt)
    f = case.f
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    Hq, T, GUARD = Hkv * G, 16, 5
    raw = [-7, 10, 5, 8, 99]               # s = (0, 10, 5, 8), e = (10, 10, 8, 16): n = (4, 0, 3, 4)
    lay = dv.Layout(raw, T, Nq)
    assert lay.n == [4, 0, 3, 4] and lay.s == [0, 10, 5, 8]
    clamped = dv.Layout([0, 10, 5, 8, 16], T, Nq)
    assert clamped.n == lay.n and np.array_equal(clamped.tok, lay.tok)
    (qv, k, v), _ = dv.inputs(oracle, "overlong", d, fmt)
    q = cm.dev16(torch, dv.pack_rows(lay, case.qb, cm.NAN16), fmt)
    case.lay = lay
    res = []
    for cu in (raw, clamped.cu):
        obuf = _sentinel_out(torch, (T + 2 * GUARD, Hq, d), torch.float32)
        lbuf = torch.full((Hq * T + 2 * GUARD * T,), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
        o, lse = case.packed(fa, torch, 0, True, out_dtype=torch.float32, q=q, out=obuf[GUARD:GUARD + T],
                             lse=lbuf[GUARD * T:GUARD * T + Hq * T].view(Hq, T), cu=cu, total_q=T)
        assert (_bits(torch, obuf[:GUARD]) == dv.SENTINEL_O32).all() and (_bits(torch, obuf[GUARD + T:]) == dv.SENTINEL_O32).all()
        assert (lbuf[:GUARD * T] == dv.SENTINEL_LSE).all() and (lbuf[GUARD * T + Hq * T:] == dv.SENTINEL_LSE).all()
        res.append((o.clone(), lse.clone()))
    for x, y in zip(*res):
        assert torch.equal(_bits(torch, x), _bits(torch, y)), "the raw vector and its clamp differ"
    want, want_lse = cm.expected_f64(qv, k, v, f["lens"], B, Hkv, G, Nq, True, 0, nq=lay.n)
    dv.check(oracle, lay, res[0][0].cpu().numpy(), res[0][1].cpu().numpy(), want, want_lse, fmt, "clamped cu_seqlens_q")


# ---- 6. end to end: the packed append, then the packed decode ------------------------------------------------------------------------
def _gather_pages(pool, table, lens, ps, Ncap):
    """pool [num_pages, Hkv, ps, d] float32 -> [B, Hkv, Ncap, d] with the rows below each length (the rest zeros)"""
    B = table.shape[0]
    out = np.zeros((B, pool.shape[1], Ncap, pool.shape[3]), np.float32)
    for b in range(B):
        for pi in range(-(-int(lens[b]) // ps)):
            out[b, :, pi * ps:(pi + 1) * ps] = pool[table[b, pi]]
        out[b, :, int(lens[b]):] = 0
    return out


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16_pages16", "fp8_contiguous"])
@pytest.mark.parametrize("d", [64, 128])
def test_append_varlen_then_decode_varlen(fa, oracle, torch_cuda, d, fp8):
    """fa_kvcache_append_varlen with rotary, seqlens_out = lens and Q rotated in place in the fused buffer, then this entry with
    cu_seqlens_q = cu_seqlens_new and cache_seqlens = lens; the float64 reference on what the append left (the rotated Q rows and the
    cache, read back), and fa_forward_varlen_kvcache[_fp8] on the same tensors as a second oracle"""
    torch = torch_cuda
    fmt, B, Hkv, G, Ncap, ps, max_q = 0, 4, 2, 2, 256, 16, 3
    Hq = Hkv * G
    before, m = [100, 0, 37, 253], [1, 3, 2, 1]
    cu = np.cumsum([2] + m)                              # two tokens of no sequence in front, three behind
    T = int(cu[-1]) + 3
    after = [min(L + x, Ncap) for L, x in zip(before, m)]
    (_, k, v), (_, kb, vb) = di.inputs(oracle, B, Hkv, G, 1, Ncap, d, fmt, 8900)
    rng = np.random.default_rng(8901)
    fused = torch.from_numpy(rng.uniform(-1, 1, (T, Hq + 2 * Hkv, d)).astype(np.float32)).cuda().to(torch.float16)
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    dcu, dl = _ints(torch, cu), _ints(torch, before)
    ks, vs = (_floats(torch, KS[:Hkv]), _floats(torch, VS[:Hkv])) if fp8 else (None, None)
    if fp8:
        kc = cm.dev8(torch, cm.poisoned(f8.encode(k).reshape(B, Hkv, Ncap, d), before, nan=f8.NAN_CODES[0]))
        vc = cm.dev8(torch, cm.poisoned(f8.encode(v).reshape(B, Hkv, Ncap, d), before, nan=f8.NAN_CODES[0]))
        table, tb = None, None
        fa.fa_kvcache_append_varlen_fp8(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, dcu, cache_seqlens=dl, seqlens_out=dl,
                                        k_scale=ks, v_scale=vs, q=fused[:, :Hq], rotary_cos=cos, rotary_sin=sin)
    else:
        kp, vp, tb = cm.scatter(kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), after, ps, 8902)
        kc, vc, table = cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(tb).cuda()
        fa.fa_kvcache_append_varlen(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, dcu, cache_seqlens=dl, seqlens_out=dl,
                                    block_table=table, q=fused[:, :Hq], rotary_cos=cos, rotary_sin=sin)
    torch.cuda.synchronize()
    assert dl.tolist() == after
    kw = dict(block_table=table, causal=True, return_lse=True)
    if fp8:
        o, lse = fa.fa_kvcache_decode_varlen_fp8(fused[:, :Hq], kc, vc, dcu, max_q, dl, k_scale=ks, v_scale=vs, **kw)
        o2, lse2 = fa.fa_forward_varlen_kvcache_fp8(fused[:, :Hq], kc, vc, dcu, dl, k_scale=ks, v_scale=vs, **kw)
    else:
        o, lse = fa.fa_kvcache_decode_varlen(fused[:, :Hq], kc, vc, dcu, max_q, dl, **kw)
        o2, lse2 = fa.fa_forward_varlen_kvcache(fused[:, :Hq], kc, vc, dcu, dl, **kw)
    torch.cuda.synchronize()
    # what the append left: the rotated Q rows and the caches, as float32
    lay = dv.Layout(cu, T, max_q)
    assert lay.n == m
    qrot = dv.unpack_rows(lay, fused[:, :Hq].float().cpu().numpy(), B).reshape(B * Hq, max_q, d)
    if fp8:
        kf = f8.decode(kc.view(torch.uint8).cpu().numpy()) * np.array(KS[:Hkv], np.float32)[None, :, None, None]
        vf = f8.decode(vc.view(torch.uint8).cpu().numpy()) * np.array(VS[:Hkv], np.float32)[None, :, None, None]
        for b in range(B):
            kf[b, :, after[b]:], vf[b, :, after[b]:] = 0, 0
    else:
        kf, vf = (_gather_pages(x.float().cpu().numpy(), tb, after, ps, Ncap) for x in (kc, vc))
    assert np.isfinite(kf).all() and np.isfinite(vf).all() and np.isfinite(qrot).all()
    want, want_lse = cm.expected_f64(qrot, kf.reshape(B * Hkv, Ncap, d), vf.reshape(B * Hkv, Ncap, d), after, B, Hkv, G, max_q, True, nq=m)
    # a fresh result: zeros and -inf in the tokens of no sequence
    free = torch.from_numpy(~lay.owned).cuda()
    assert (o[free] == 0).all() and (lse[:, free] == float("-inf")).all()
    dv.check(oracle, lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, "append_varlen -> decode_varlen", sentinel=False)
    # the prefill entry on the same tensors: within the bounds of the reference itself, and of this entry (two kernels that round
    # independently: the tolerance model of cm.peaked_tol with kernels = 2, and twice the lse bound)
    dv.check(oracle, lay, o2.cpu().numpy(), lse2.cpu().numpy(), want, want_lse, fmt, "append_varlen -> forward_varlen_kvcache", sentinel=False)
    t = _live_index(torch, lay)[2]
    diff = float((o[t] - o2[t]).abs().max())
    ldiff = float((lse[:, t] - lse2[:, t]).abs().max())
    print(f"decode_varlen against forward_varlen_kvcache: max_abs={diff:.3e} lse_abs={ldiff:.3e}")
    assert diff <= cm.peaked_tol(fmt, float(np.abs(vf).max()), kernels=2) and ldiff <= 4 * cm.P_EPS[fmt]


# ---- 7. the captured step -------------------------------------------------------------------------------------------------------------
def test_captured_packed_step(fa, oracle, torch_cuda):
    """append_varlen (paged, rotary, lengths and Q in place) -> decode_varlen behind a split, captured once as a linear graph; replayed
    after cu_seqlens_new, the lengths, the table and the sinks are rewritten in place; each replay equals the eager call bit for bit"""
    torch = torch_cuda
    d, B, Hkv, G, Ncap, ps, max_q, T = 64, 2, 1, 2, 8192, 16, 2, 6
    Hq, max_pages = Hkv * G, Ncap // ps
    num_pages = B * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(8950)
    pool = lambda: (torch.rand((num_pages, Hkv, ps, d), device="cuda", generator=gen) * 2 - 1).to(torch.float16)
    kp0, vp0 = pool(), pool()
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, max_q, d, max_pages=max_pages, page_size=ps)
    assert need > 0                                       # S > 1: the merge is in the graph
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    # the graph's tensors
    fused = torch.zeros(T, Hq + 2 * Hkv, d, dtype=torch.float16, device="cuda")
    kp, vp = kp0.clone(), vp0.clone()
    cu, lens = _ints(torch, [0, 1, 2]), _ints(torch, [0, 0])
    table = torch.zeros(B, max_pages, dtype=torch.int32, device="cuda")
    sinks = torch.zeros(Hq, dtype=torch.float32, device="cuda")
    out = torch.zeros(T, Hq, d, dtype=torch.float32, device="cuda")
    lse = torch.zeros(Hq, T, dtype=torch.float32, device="cuda")

    def step(fz, ck, cv, cl, o, l):
        fa.fa_kvcache_append_varlen(fz[:, Hq:Hq + Hkv], fz[:, Hq + Hkv:], ck, cv, cu, cache_seqlens=cl, seqlens_out=cl, block_table=table,
                                    q=fz[:, :Hq], rotary_cos=cos, rotary_sin=sin)
        fa.fa_kvcache_decode_varlen(fz[:, :Hq], ck, cv, cu, max_q, cl, table, causal=True, out=o, lse=l, workspace=ws, sinks=sinks)

    def state(s):
        """the inputs of step s: tokens, the vector (with tokens of no sequence), lengths, a permuted table, sinks"""
        g = torch.Generator(device="cuda").manual_seed(9000 + s)
        tokens = (torch.rand((T, Hq + 2 * Hkv, d), device="cuda", generator=g) * 2 - 1).to(torch.float16)
        vec = ([1, 3, 4], [0, 1, 2], [2, 2, 6])[s]       # n = (2, 1); (1, 1); (0, 2 of 4: cut at max_q)
        L = ([8000, 4100], [37, 8190], [5000, 0])[s]
        perm = torch.randperm(num_pages, device="cuda", generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
        return tokens, _ints(torch, vec), _ints(torch, L), perm, _floats(torch, [0.5 * s - 0.3 * h for h in range(Hq)])

    step(fused.clone(), kp.clone(), vp.clone(), lens.clone(), out.clone(), lse.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(fused, kp, vp, lens, out, lse)
    for s in range(3):
        tokens, vec, L, perm, sk = state(s)
        for dst, src in ((fused, tokens), (cu, vec), (lens, L), (table, perm), (sinks, sk), (kp, kp0), (vp, vp0)):
            dst.copy_(src)
        ws.fill_(0xFF), out.fill_(dv.SENTINEL_LSE), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in (out, lse, fused, kp, vp, lens)]
        # the eager call from the same state
        ef, ek, ev, el = tokens.clone(), kp0.clone(), vp0.clone(), L.clone()
        eo, elz = torch.full_like(out, dv.SENTINEL_LSE), torch.full_like(lse, dv.SENTINEL_LSE)
        ws.fill_(0xFF)
        step(ef, ek, ev, el, eo, elz)
        torch.cuda.synchronize()
        for x, y, n in zip(got, (eo, elz, ef, ek, ev, el), ("O", "lse", "the fused buffer", "K pool", "V pool", "lengths")):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), f"step {s}: {n} of the replay differs from the eager call"
        lay = dv.Layout(vec.tolist(), T, max_q)
        t = _live_index(torch, lay)[2]
        assert torch.isfinite(out[t]).all() and torch.isfinite(lse[:, t]).all(), s
        free = torch.from_numpy(~lay.owned).cuda()
        assert (out[free] == dv.SENTINEL_LSE).all() and (lse[:, free] == dv.SENTINEL_LSE).all(), s


# ---- 8. the torch ops -----------------------------------------------------------------------------------------------------------------
def test_ops_are_the_front_ends(fa, oracle, torch_cuda):
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    name, d, fmt = "spec", 128, 1
    sc = 1.0 / np.sqrt(d)
    for fp8, ps in ((False, 0), (False, 16), (True, 0)):
        case = Case(oracle, torch, name, d, fmt, ps=ps, fp8=fp8, seed=4)
        Hq = case.f["Hkv"] * case.f["G"]
        q = cm.dev16(torch, dv.pack_rows(case.lay, case.qb, 0), fmt)
        cu, sk = _ints(torch, case.lay.cu), _floats(torch, li.sinks_for(Hq))
        kw = dict(cache_seqlens=case.lens, block_table=case.table, causal=True, scale=sc, window=100, sinks=sk, softcap=li.SOFTCAP,
                  out_dtype=torch.float32, return_lse=True)
        if fp8:
            got = ops.decode_varlen_fp8(q, case.k, case.v, cu, case.lay.max_q, case.lens, case.table, *case.scales, sc, True, 100, sk,
                                        li.SOFTCAP, True)
            want = fa.fa_kvcache_decode_varlen_fp8(q, case.k, case.v, cu, case.lay.max_q, k_scale=case.scales[0], v_scale=case.scales[1], **kw)
        else:
            got = ops.decode_varlen(q, case.k, case.v, cu, case.lay.max_q, case.lens, case.table, sc, True, 100, sk, li.SOFTCAP, True)
            want = fa.fa_kvcache_decode_varlen(q, case.k, case.v, cu, case.lay.max_q, **kw)
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y) and not torch.isnan(x).any(), (fp8, ps)
        free = torch.from_numpy(~case.lay.owned).cuda()
        assert (got[0][free] == 0).all() and (got[1][:, free] == float("-inf")).all()
