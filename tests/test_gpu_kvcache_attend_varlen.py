"""GPU tier of the mixed prefill + decode step fa_kvcache_attend_varlen (fa.fa_kvcache_attend_varlen, _fp8).

Families, classes, the float64 reference and the check are tests/attend_varlen_inputs.py's (its CPU tier shows that eight wrong routing
rules fail that check).  The bit ties are against the two existing entries on the same tensors: the rows of a sequence of at most T
rows against fa_kvcache_decode_varlen(max_seqlen_q=T, causal=True), the rows of a longer one against fa_forward_varlen_kvcache[_fp8]
(causal=True).  The bounds of the value checks are those tiers' own (av.problems takes them from their modules).  T = 4 unless stated.

Poison: O and lse are pre-filled with sentinels, the workspace with NaN bytes; the Q row of every token of no sequence, every cache row
at or past L_b and every pool page no table names hold NaN bit patterns; every table entry past the live pages holds garbage.
"""
import numpy as np
import pytest

import attend_varlen_inputs as av
import common_inputs as cm
import decode_varlen_inputs as dv
import fp8_inputs as f8
import rope_inputs as rp

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
FORMS = [(0, False), (av.PAGE, False), (0, True), (av.PAGE, True)]   # (page size or 0, fp8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ints(torch, values):
    return torch.tensor([int(x) for x in values], dtype=torch.int32, device="cuda")


def _floats(torch, values):
    return None if values is None else torch.tensor(np.asarray(values, np.float32), dtype=torch.float32, device="cuda")


def _sentinels(torch, total_q, Hq, d, out_dtype):
    if out_dtype == torch.float32:
        o = torch.full((total_q, Hq, d), dv.SENTINEL_O32, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        o = torch.full((total_q, Hq, d), dv.SENTINEL_O16, dtype=torch.int16, device="cuda").view(out_dtype)
    return o, torch.full((Hq, total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")


def _bits(torch, t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _mask(torch, rows):
    return torch.from_numpy(np.asarray(rows, bool)).cuda()


class Case:
    """the device tensors of one (family, d, fmt, cache form), made once and used by the entry under test and by the two it is tied to"""

    def __init__(self, torch, name, d, fmt, ps=0, fp8=False):
        self.name, self.d, self.fmt, self.ps, self.fp8, self.lay, self.T = name, d, fmt, ps, fp8, av.layout(name), av.threshold(name)
        B, Hkv, G, Ncap = av.shape(name)
        self.Hq, lens = Hkv * G, av.FAMILIES[name]["lens"]
        (_, k, v), (qb, kb, vb) = av.inputs(name, d, fmt)
        qb = np.array(qb)
        qb[~self.lay.rows(3)] = cm.NAN16                      # tokens of no sequence: never read
        self.q = cm.dev16(torch, qb, fmt)
        if fp8:
            kb, vb, nan, dev = f8.encode(k), f8.encode(v), f8.NAN_CODES[0], lambda a: cm.dev8(torch, a)
            self.scales = dict(k_scale=_floats(torch, av.KS), v_scale=_floats(torch, av.VS))
        else:
            nan, dev, self.scales = cm.NAN16, (lambda a: cm.dev16(torch, a, fmt)), {}
        kc, vc = (x.reshape(B, Hkv, Ncap, d) for x in (kb, vb))
        if ps:
            kp, vp, table = cm.scatter(kc, vc, lens, ps, 9900 + ps, nan=nan)
            self.k, self.v, self.table = dev(kp), dev(vp), torch.from_numpy(table).cuda()
        else:
            self.k, self.v, self.table = dev(cm.poisoned(kc, lens, nan=nan)), dev(cm.poisoned(vc, lens, nan=nan)), None
        self.lens, self.cu = _ints(torch, lens), _ints(torch, self.lay.cu)
        self.tdt = torch.bfloat16 if fmt else torch.float16

    def _options(self, torch, on):
        W, softcap, sinks = av.options(on, self.Hq)
        return dict(window=W, softcap=softcap, sinks=_floats(torch, sinks))

    def _workspace(self, fa, torch, W):
        B, Hkv, G, Ncap = av.shape(self.name)
        kw = dict(max_pages=Ncap // self.ps, page_size=self.ps) if self.ps else dict(Ncap=Ncap)
        need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, self.T, self.d, window=W, **kw)
        assert (need > 0) == (av.want_S(self.name, W) > 1)
        return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN

    def attend(self, fa, torch, parts=3, on=False, out_dtype=None, out=None, lse=None):
        """the entry under test into sentinel-filled buffers (or the given ones) -> (O, lse)"""
        o, l = _sentinels(torch, self.lay.total_q, self.Hq, self.d, out_dtype or torch.float32)
        out, lse = (o if out is None else out), (l if lse is None else lse)
        opts = self._options(torch, on)
        fn = fa.fa_kvcache_attend_varlen_fp8 if self.fp8 else fa.fa_kvcache_attend_varlen
        got = fn(self.q, self.k, self.v, self.cu, self.lens, self.table, split_rows=self.T, out=out, lse=lse, parts=parts,
                 workspace=self._workspace(fa, torch, opts["window"]), **opts, **self.scales)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lse.data_ptr()
        return out, lse

    def decode(self, fa, torch, on=False, out_dtype=None):
        """fa_kvcache_decode_varlen with max_seqlen_q = T on the same arguments"""
        out, lse = _sentinels(torch, self.lay.total_q, self.Hq, self.d, out_dtype or torch.float32)
        opts = self._options(torch, on)
        fn = fa.fa_kvcache_decode_varlen_fp8 if self.fp8 else fa.fa_kvcache_decode_varlen
        fn(self.q, self.k, self.v, self.cu, self.T, self.lens, self.table, causal=True, out=out, lse=lse,
           workspace=self._workspace(fa, torch, opts["window"]), **opts, **self.scales)
        torch.cuda.synchronize()
        return out, lse

    def prefill(self, fa, torch, on=False, out_dtype=None):
        """fa_forward_varlen_kvcache[_fp8] on the same arguments"""
        out, lse = _sentinels(torch, self.lay.total_q, self.Hq, self.d, out_dtype or torch.float32)
        fn = fa.fa_forward_varlen_kvcache_fp8 if self.fp8 else fa.fa_forward_varlen_kvcache
        fn(self.q, self.k, self.v, self.cu, self.lens, self.table, causal=True, out=out, lse=lse, **self._options(torch, on), **self.scales)
        torch.cuda.synchronize()
        return out, lse


def _same_rows(torch, got, other, rows, what):
    """O and lse of `got` equal `other`'s on the tokens `rows` (numpy bool), bit for bit; nothing there is NaN"""
    m = _mask(torch, rows)
    assert int(m.sum()) > 0, what
    assert torch.equal(_bits(torch, got[0][m]), _bits(torch, other[0][m])), f"{what}: O differs"
    assert torch.equal(_bits(torch, got[1][:, m]), _bits(torch, other[1][:, m])), f"{what}: lse differs"
    assert not torch.isnan(got[0][m]).any() and not torch.isnan(got[1][:, m]).any(), f"{what}: NaN in a live row"


def _keeps_sentinels(torch, got, rows, what):
    """the tokens `rows` (numpy bool) hold every sentinel byte"""
    m = _mask(torch, rows)
    if int(m.sum()) == 0:
        return
    want = dv.SENTINEL_O32 if got[0].dtype == torch.float32 else dv.SENTINEL_O16
    assert (_bits(torch, got[0][m]) == want).all(), f"{what}: an O row that must stay untouched was written"
    assert (got[1][:, m] == dv.SENTINEL_LSE).all(), f"{what}: an lse entry that must stay untouched was written"


def _tied_to_both(fa, torch, case, on, out_dtype):
    lay = case.lay
    what = f"{case.name} d={case.d} fmt={case.fmt} ps={case.ps} fp8={case.fp8} on={on} {out_dtype}"
    got = case.attend(fa, torch, 3, on, out_dtype)
    if lay.rows(av.SHORT).any():
        _same_rows(torch, got, case.decode(fa, torch, on, out_dtype), lay.rows(av.SHORT), what + " SHORT rows against decode_varlen")
    if lay.rows(av.LONG).any():
        _same_rows(torch, got, case.prefill(fa, torch, on, out_dtype), lay.rows(av.LONG), what + " LONG rows against varlen_kvcache")
    _keeps_sentinels(torch, got, ~lay.rows(3), what)
    return got


# ---- 1. the bits of the two existing entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "clamped", "nokey"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bits_of_the_two_entries(fa, torch_cuda, fmt, d, name):
    """contiguous and pages of 16, 16-bit and e4m3fn caches with per-head scales, both output types; the options off, and window 48,
    soft-cap 30 and sinks with one -inf head on together.  One pass in the SHORT half (the families' capacity of 256 keys)"""
    torch = torch_cuda
    assert av.want_S(name) == 1 and av.want_S(name, av.WINDOW) == 1
    for ps, fp8 in FORMS:
        case = Case(torch, name, d, fmt, ps, fp8)
        for on in (False, True):
            for out_dtype in (torch.float32, case.tdt):
                _tied_to_both(fa, torch, case, on, out_dtype)


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bits_behind_the_merge(fa, torch_cuda, fmt, d):
    """"mixed" on a capacity of 1024 keys: the SHORT half runs split with its merge (want_S > 1), whose waves of a LONG sequence must
    return without writing"""
    torch = torch_cuda
    assert av.want_S("split") > 1
    for ps, fp8 in ((0, False), (av.PAGE, True)):
        case = Case(torch, "split", d, fmt, ps, fp8)
        for on, out_dtype in ((False, torch.float32), (True, case.tdt)):
            _tied_to_both(fa, torch, case, on, out_dtype)
        for parts in (1, 2):
            got = case.attend(fa, torch, parts)
            _keeps_sentinels(torch, got, ~case.lay.rows(parts), f"split parts={parts}")


# ---- 2. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "clamped", "nokey", "all_short", "all_long", "tiny"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_values(fa, torch_cuda, fmt, d, name):
    """against the float64 reference, at the bounds of the packed-decode and the varlen-cache tiers; rows without a key exact"""
    torch = torch_cuda
    for (ps, fp8), on in zip(FORMS, (False, True, True, False)):
        o, lse = Case(torch, name, d, fmt, ps, fp8).attend(fa, torch, 3, on)
        want = av.model(name, d, fmt, 3, on, fp8)
        found = av.problems(name, o.cpu().numpy(), lse.cpu().numpy(), *want, 3, fmt)
        assert not found, f"{name} ps={ps} fp8={fp8} on={on}: {found}"


# ---- 3. parts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "clamped", "nokey"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parts(fa, torch_cuda, fmt, d, name):
    """parts = 1 and parts = 2 into sentinel-filled buffers: the other class's rows and the tokens of no sequence keep every sentinel
    byte; the two outputs overlaid are the parts = 3 output bit for bit"""
    torch = torch_cuda
    for (ps, fp8), on in zip(FORMS, (True, False, False, True)):
        case = Case(torch, name, d, fmt, ps, fp8)
        for out_dtype in (torch.float32, case.tdt):
            both = case.attend(fa, torch, 3, on, out_dtype)
            halves = {}
            for parts in (1, 2):
                halves[parts] = case.attend(fa, torch, parts, on, out_dtype)
                what = f"{name} ps={ps} fp8={fp8} parts={parts} {out_dtype}"
                _keeps_sentinels(torch, halves[parts], ~case.lay.rows(parts), what)
                _same_rows(torch, halves[parts], both, case.lay.rows(parts), what + " against parts=3")
            short = _mask(torch, case.lay.rows(1))
            o = torch.where(short[:, None, None], _bits(torch, halves[1][0]), _bits(torch, halves[2][0]))
            l = torch.where(short[None, :], halves[1][1], halves[2][1])
            assert torch.equal(o, _bits(torch, both[0])) and torch.equal(_bits(torch, l), _bits(torch, both[1])), name
            # parts = 2 after parts = 1 into the SAME buffers: the two-stream form
            out, lse = case.attend(fa, torch, 1, on, out_dtype)
            case.attend(fa, torch, 2, on, out_dtype, out=out, lse=lse)
            assert torch.equal(_bits(torch, out), _bits(torch, both[0])) and torch.equal(_bits(torch, lse), _bits(torch, both[1])), name


# ---- 4. class-uniform batches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_class_uniform_batches(fa, torch_cuda, fmt, d):
    """all_short equals the decode entry everywhere, all_long the prefill entry everywhere, tiny (total_q <= T: the LONG half is not
    launched) the decode entry, and tiny's parts = 2 call writes nothing"""
    torch = torch_cuda
    for ps, fp8 in FORMS:
        for on in (False, True):
            for name, other in (("all_short", "decode"), ("all_long", "prefill"), ("tiny", "decode")):
                case = Case(torch, name, d, fmt, ps, fp8)
                got = case.attend(fa, torch, 3, on)
                ref = getattr(case, other)(fa, torch, on)
                for x, y, n in zip(got, ref, ("O", "lse")):
                    assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{name} ps={ps} fp8={fp8} on={on}: {n} differs from {other}"
                assert int(_mask(torch, case.lay.rows(3)).sum()) > 0 and not torch.isnan(got[1][:, _mask(torch, case.lay.rows(3))]).any()
    case = Case(torch, "tiny", d, fmt)
    assert case.lay.total_q <= av.T
    nothing = case.attend(fa, torch, 2)
    _keeps_sentinels(torch, nothing, np.ones(case.lay.total_q, bool), "tiny parts=2")


# ---- 5. end to end: the packed append, then the mixed step ----------------------------------------------------------------------------
def _gather_pages(pool, table, lens, ps, Ncap):
    B = table.shape[0]
    out = np.zeros((B, pool.shape[1], Ncap, pool.shape[3]), np.float32)
    for b in range(B):
        for pi in range(-(-int(lens[b]) // ps)):
            out[b, :, pi * ps:(pi + 1) * ps] = pool[table[b, pi]]
        out[b, :, int(lens[b]):] = 0
    return out


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16_pages16", "fp8_contiguous"])
@pytest.mark.parametrize("d", [64, 128])
def test_append_varlen_then_attend_varlen(fa, torch_cuda, d, fp8):
    """fa_kvcache_append_varlen with rotary, seqlens_out = lens and Q rotated in place in a fused QKV buffer, then attend_varlen on the
    rotated Q view with cu_seqlens_q = cu_seqlens_new and cache_seqlens = lens; the float64 reference on what the append left"""
    torch = torch_cuda
    fmt, B, Hkv, G, Ncap, ps = 0, 4, av.HKV, av.G, 256, av.PAGE
    Hq = Hkv * G
    before, m = [100, 0, 37, 60], [1, 9, 4, 140]            # SHORT, LONG from an empty cache, SHORT at T, LONG across a row block
    cu = np.cumsum([2] + m)
    total = int(cu[-1]) + 3
    after = [L + x for L, x in zip(before, m)]
    rng = np.random.default_rng(9950 + d)
    kb, vb = (av.vi.encode16(rng.uniform(-1, 1, (B, Hkv, Ncap, d)).astype(np.float32), fmt) for _ in range(2))
    k, v = (av.vi.decode16(x, fmt) for x in (kb, vb))
    fused = torch.from_numpy(rng.uniform(-1, 1, (total, Hq + 2 * Hkv, d)).astype(np.float32)).cuda().to(torch.float16)
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    dcu, dl = _ints(torch, cu), _ints(torch, before)
    if fp8:
        ks, vs = _floats(torch, av.KS), _floats(torch, av.VS)
        kc = cm.dev8(torch, cm.poisoned(f8.encode(k), before, nan=f8.NAN_CODES[0]))
        vc = cm.dev8(torch, cm.poisoned(f8.encode(v), before, nan=f8.NAN_CODES[0]))
        table, tb = None, None
        fa.fa_kvcache_append_varlen_fp8(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, dcu, cache_seqlens=dl, seqlens_out=dl,
                                        k_scale=ks, v_scale=vs, q=fused[:, :Hq], rotary_cos=cos, rotary_sin=sin)
        o, lse = fa.fa_kvcache_attend_varlen_fp8(fused[:, :Hq], kc, vc, dcu, dl, k_scale=ks, v_scale=vs, split_rows=av.T, return_lse=True)
    else:
        kp, vp, tb = cm.scatter(kb, vb, after, ps, 9951)
        kc, vc, table = cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(tb).cuda()
        fa.fa_kvcache_append_varlen(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, dcu, cache_seqlens=dl, seqlens_out=dl,
                                    block_table=table, q=fused[:, :Hq], rotary_cos=cos, rotary_sin=sin)
        o, lse = fa.fa_kvcache_attend_varlen(fused[:, :Hq], kc, vc, dcu, dl, table, split_rows=av.T, return_lse=True)
    torch.cuda.synchronize()
    assert dl.tolist() == after
    qrot = fused[:, :Hq].float().cpu().numpy()
    if fp8:
        kf = f8.decode(kc.view(torch.uint8).cpu().numpy()) * np.array(av.KS, np.float32)[None, :, None, None]
        vf = f8.decode(vc.view(torch.uint8).cpu().numpy()) * np.array(av.VS, np.float32)[None, :, None, None]
        for b in range(B):
            kf[b, :, after[b]:], vf[b, :, after[b]:] = 0, 0
    else:
        kf, vf = (_gather_pages(x.float().cpu().numpy(), tb, after, ps, Ncap) for x in (kc, vc))
    assert np.isfinite(kf).all() and np.isfinite(vf).all()
    want = np.zeros((total, Hq, d), np.float64)
    want_lse = np.full((Hq, total), -np.inf, np.float64)
    own = np.zeros(total, bool)
    for b in range(B):
        s, n = int(cu[b]), m[b]
        ob, lb = cm.expected_f64(np.ascontiguousarray(qrot[s:s + n].transpose(1, 0, 2)), kf[b], vf[b], [after[b]], 1, Hkv, G, n, True)
        want[s:s + n], want_lse[:, s:s + n], own[s:s + n] = ob.transpose(1, 0, 2), lb, True
    # a fresh result: zeros and -inf in the tokens of no sequence (vi.problems' base)
    found = av.vi.problems(o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, own, fmt, base=(0.0, -np.inf))
    assert not found, found


# ---- 6. the captured step -------------------------------------------------------------------------------------------------------------
def test_captured_mixed_step(fa, torch_cuda):
    """append_varlen (paged, rotary, lengths and Q in place) -> attend_varlen with T = 4, captured once; replayed after cu_seqlens, the
    lengths, the table and the sinks are rewritten in place so that one sequence changes class in each direction (1 row -> 9 rows, 140
    rows -> 2 rows); each replay equals the eager call on the same data bit for bit"""
    torch = torch_cuda
    d, B, Hkv, G, Ncap, ps, T, total = 64, 2, 1, 2, 512, 16, av.T, 150
    Hq, max_pages = Hkv * G, Ncap // ps
    num_pages = B * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(9960)
    pool = lambda: (torch.rand((num_pages, Hkv, ps, d), device="cuda", generator=gen) * 2 - 1).to(torch.float16)
    kp0, vp0 = pool(), pool()
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, T, d, max_pages=max_pages, page_size=ps)
    assert need > 0                                       # S > 1: the merge is in the graph
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    fused = torch.zeros(total, Hq + 2 * Hkv, d, dtype=torch.float16, device="cuda")
    kp, vp = kp0.clone(), vp0.clone()
    cu, lens = _ints(torch, [0, 1, 2]), _ints(torch, [0, 0])
    table = torch.zeros(B, max_pages, dtype=torch.int32, device="cuda")
    sinks = torch.zeros(Hq, dtype=torch.float32, device="cuda")
    out = torch.zeros(total, Hq, d, dtype=torch.float32, device="cuda")
    lse = torch.zeros(Hq, total, dtype=torch.float32, device="cuda")

    def step(fz, ck, cv, cl, o, l):
        fa.fa_kvcache_append_varlen(fz[:, Hq:Hq + Hkv], fz[:, Hq + Hkv:], ck, cv, cu, cache_seqlens=cl, seqlens_out=cl, block_table=table,
                                    q=fz[:, :Hq], rotary_cos=cos, rotary_sin=sin)
        fa.fa_kvcache_attend_varlen(fz[:, :Hq], ck, cv, cu, cl, table, split_rows=T, out=o, lse=l, workspace=ws, sinks=sinks)

    def state(s):
        g = torch.Generator(device="cuda").manual_seed(9970 + s)
        tokens = (torch.rand((total, Hq + 2 * Hkv, d), device="cuda", generator=g) * 2 - 1).to(torch.float16)
        vec = ([2, 3, 143], [2, 11, 13], [5, 5, 9])[s]       # spans (1, 140); (9, 2); (0, 4)
        L = ([100, 50], [300, 7], [77, 500])[s]
        perm = torch.randperm(num_pages, device="cuda", generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
        return tokens, _ints(torch, vec), _ints(torch, L), perm, _floats(torch, [0.5 * s - 0.3 * h for h in range(Hq)])

    step(fused.clone(), kp.clone(), vp.clone(), lens.clone(), out.clone(), lse.clone())   # warm-up on scratch state (both halves run)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(fused, kp, vp, lens, out, lse)
    classes = []
    for s in range(3):
        tokens, vec, L, perm, sk = state(s)
        for dst, src in ((fused, tokens), (cu, vec), (lens, L), (table, perm), (sinks, sk), (kp, kp0), (vp, vp0)):
            dst.copy_(src)
        ws.fill_(0xFF), out.fill_(dv.SENTINEL_LSE), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in (out, lse, fused, kp, vp, lens)]
        ef, ek, ev, el = tokens.clone(), kp0.clone(), vp0.clone(), L.clone()
        eo, elz = torch.full_like(out, dv.SENTINEL_LSE), torch.full_like(lse, dv.SENTINEL_LSE)
        ws.fill_(0xFF)
        step(ef, ek, ev, el, eo, elz)
        torch.cuda.synchronize()
        for x, y, n in zip(got, (eo, elz, ef, ek, ev, el), ("O", "lse", "the fused buffer", "K pool", "V pool", "lengths")):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), f"step {s}: {n} of the replay differs from the eager call"
        lay = av.Layout(vec.tolist(), total)
        classes.append(tuple(lay.cls))
        live, free = _mask(torch, lay.rows(3)), _mask(torch, ~lay.rows(3))
        assert torch.isfinite(out[live]).all() and torch.isfinite(lse[:, live]).all(), s
        assert (out[free] == dv.SENTINEL_LSE).all() and (lse[:, free] == dv.SENTINEL_LSE).all(), s
    assert classes == [(av.SHORT, av.LONG), (av.LONG, av.SHORT), (0, av.SHORT)]


# ---- 7. the default threshold, on the real grid shapes --------------------------------------------------------------------------------
def test_default_threshold(fa, torch_cuda):
    """spans (1, 128, 129) over 300 keys, d = 64, paged fp16, split_rows left at its default of 128: 128 rows are the last SHORT span,
    129 the first LONG one"""
    torch = torch_cuda
    case = Case(torch, "default", 64, 0, av.PAGE)
    assert case.T == 128 and case.lay.cls == [av.SHORT, av.SHORT, av.LONG]
    got = _tied_to_both(fa, torch, case, False, torch.float32)
    o, lse = fa.fa_kvcache_attend_varlen(case.q, case.k, case.v, case.cu, case.lens, case.table, return_lse=True)   # the default
    torch.cuda.synchronize()
    live = _mask(torch, case.lay.rows(3))
    assert torch.equal(o[live], got[0][live]) and torch.equal(lse[:, live], got[1][:, live])
    assert (o[~live] == 0).all() and (lse[:, ~live] == float("-inf")).all()       # a fresh result
    found = av.problems("default", got[0].cpu().numpy(), got[1].cpu().numpy(), *av.model("default", 64, 0), 3, 0)
    assert not found, found


# ---- 8. the torch ops -----------------------------------------------------------------------------------------------------------------
def test_ops_are_the_front_ends(fa, torch_cuda):
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    d, fmt = 128, 1
    sc = 1.0 / np.sqrt(d)
    for ps, fp8 in ((0, False), (av.PAGE, True)):
        case = Case(torch, "mixed", d, fmt, ps, fp8)
        W, softcap, sinks = av.options(True, case.Hq)
        sk = _floats(torch, sinks)
        kw = dict(split_rows=av.T, scale=sc, window=W, sinks=sk, softcap=softcap, out_dtype=torch.float32, return_lse=True)
        for parts in (3, 1):
            if fp8:
                got = ops.attend_varlen_fp8(case.q, case.k, case.v, case.cu, case.lens, case.table, case.scales["k_scale"],
                                            case.scales["v_scale"], av.T, sc, W, sk, softcap, parts, True)
                want = fa.fa_kvcache_attend_varlen_fp8(case.q, case.k, case.v, case.cu, case.lens, case.table, parts=parts, **kw, **case.scales)
            else:
                got = ops.attend_varlen(case.q, case.k, case.v, case.cu, case.lens, case.table, av.T, sc, W, sk, softcap, parts, True)
                want = fa.fa_kvcache_attend_varlen(case.q, case.k, case.v, case.cu, case.lens, case.table, parts=parts, **kw)
            torch.cuda.synchronize()
            for x, y in zip(got, want):
                assert torch.equal(x, y) and not torch.isnan(x).any(), (ps, fp8, parts)
            free = _mask(torch, ~case.lay.rows(parts))
            assert (got[0][free] == 0).all() and (got[1][:, free] == float("-inf")).all()
