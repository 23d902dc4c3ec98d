"""GPU tier of the tree step: fa_kvcache_decode_varlen_ex with a tree mask (fa.fa_kvcache_decode_varlen(tree_mask=...), _fp8) and
fa_kvcache_append_varlen_ex with positions (fa.fa_kvcache_append_varlen(positions=...), _fp8).

Families, trees, the float64 reference with an explicit visibility and the numpy restatement of the append are tests/tree_inputs.py's;
its CPU tier shows that eleven wrong mask kernels and four wrong position rules fail the checks applied here.  Bounds are the
project's (dv.check: cm.MAX_ABS, cm.REL_L2, 2 * cm.P_EPS on lse; exact 0 / -inf on rows without a key); the census is decided between
neighbouring integers (ci.MARGIN); everything else is bit for bit.

Poison, as in the packed decode's tier: O and lse pre-filled with sentinels, the workspace with NaN bytes, cache rows past L_b and
unnamed pool pages NaN, table entries past the live pages garbage, Q rows of no sequence NaN and their mask words all-ones.
"""
import numpy as np
import pytest

import append_varlen_inputs as av
import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv
import fp8_inputs as f8
import logit_inputs as li
import ragged_inputs as ri
import rope_inputs as rp
import tree_inputs as ti

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
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


def _words(torch, words):
    """uint64 numpy words -> the int64 device tensor the front end takes (bit 63 is the sign bit)"""
    return torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64).copy()).cuda()


def _sentinel_out(torch, shape, out_dtype):
    if out_dtype == torch.float32:
        return torch.full(shape, dv.SENTINEL_O32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, dv.SENTINEL_O16, dtype=torch.int16, device="cuda").view(out_dtype)


def _bits(torch, t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Step:
    """The device tensors of one (family, d, fmt, cache form); bits: (q, k, v) encodings other than the family's own (the census)"""

    def __init__(self, oracle, torch, name, d, fmt, ps=0, fp8=False, seed=0, bits=None):
        self.f, self.lay, self.name, self.d, self.fmt, self.ps, self.fp8 = ti.family(name), ti.layout(name), name, d, fmt, ps, fp8
        B, Hkv, G, Nq, Ncap = ri.shape(self.f)
        (_, k, v), (qb, kb, vb) = ti.inputs(oracle, name, d, fmt)
        if bits is not None:
            assert not fp8
            qb, kb, vb = bits
        self.qb, lens = qb, self.f["lens"]
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
        assert di.splits_of(need, B * Hkv, G * Nq, self.d) == ri.want_S(self.f, W)
        return need

    def call(self, fa, torch, W, words, variant="none", out_dtype=None, poison=True, q=None, out=None, mask=None):
        """the packed entry, causal, with the tree words (numpy uint64; None: the plain entry) -> (O [total_q, Hq, d], lse [Hq, total_q]),
        both pre-filled with the sentinels unless given"""
        B, Hkv, G, Nq, Ncap = ri.shape(self.f)
        Hq, lay = Hkv * G, self.lay
        out_dtype = out_dtype or torch.float32
        if q is None:
            q = cm.dev16(torch, dv.pack_rows(lay, self.qb, cm.NAN16 if poison else 0), self.fmt)
        if out is None:
            out = _sentinel_out(torch, (lay.total_q, Hq, self.d), out_dtype)
        lse = torch.full((Hq, lay.total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
        sinks, softcap = li.options(variant, Hq)
        ws = torch.full((max(self.need(fa, W), 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN
        if mask is None and words is not None:
            mask = _words(torch, words)
        kw = dict(cache_seqlens=self.lens, block_table=self.table, causal=True, out=out, lse=lse, workspace=ws, window=W, softcap=softcap,
                  sinks=_floats(torch, sinks), tree_mask=mask)
        cu = _ints(torch, lay.cu)
        if self.fp8:
            o, l = fa.fa_kvcache_decode_varlen_fp8(q, self.k, self.v, cu, lay.max_q, k_scale=self.scales[0], v_scale=self.scales[1], **kw)
        else:
            o, l = fa.fa_kvcache_decode_varlen(q, self.k, self.v, cu, lay.max_q, **kw)
        torch.cuda.synchronize()
        assert o.data_ptr() == out.data_ptr() and o.dtype == out_dtype
        return o, l


def _free_tokens_hold_the_sentinel(torch, lay, o, lse, what):
    free = torch.from_numpy(~lay.owned).cuda()
    want = dv.SENTINEL_O32 if o.dtype == torch.float32 else dv.SENTINEL_O16
    assert (_bits(torch, o[free]) == want).all(), what + ": an O row of no sequence was written"
    assert (lse[:, free] == dv.SENTINEL_LSE).all(), what + ": an lse entry of no sequence was written"


def _fp8_reference(oracle, name, d, fmt, kind, W):
    f, lay = ti.family(name), ti.layout(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = ti.inputs(oracle, name, d, fmt)
    kd = f8.decode(f8.encode(k)) * np.tile(np.array(KS[:Hkv], np.float32), B)[:, None, None]
    vd = f8.decode(f8.encode(v)) * np.tile(np.array(VS[:Hkv], np.float32), B)[:, None, None]
    return ti.expected_f64(q, kd, vd, ti.visibility(lay, f["lens"], Ncap, G, ti.tree(name, kind)[0], W), B, Hkv, G, Nq)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", ti.WINDOWS)
@pytest.mark.parametrize("name", ti.NAMES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity(fa, oracle, torch_cuda, fmt, d, name, W):
    """every tree of the family on a contiguous cache and on pages of 16; the random tree on e4m3fn caches with per-head scales"""
    torch = torch_cuda
    if name == "split" and W == 0:
        assert ri.want_S(ti.family(name), W) > 1
    for ps in (0, 16):
        step = Step(oracle, torch, name, d, fmt, ps=ps, seed=ps + 1)
        for kind in ti.TREES:
            want, want_lse = ti.reference(oracle, name, d, fmt, kind, W)
            o, lse = step.call(fa, torch, W, ti.tree(name, kind)[0])
            dv.check(oracle, step.lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"{name} {kind} W={W} ps={ps}")
        want, want_lse = _fp8_reference(oracle, name, d, fmt, "random", W)
        o, lse = Step(oracle, torch, name, d, fmt, ps=ps, fp8=True, seed=ps + 2).call(fa, torch, W, ti.tree(name, "random")[0])
        dv.check(oracle, step.lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"{name} random W={W} ps={ps} fp8")


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity_with_sinks_and_softcap(fa, oracle, torch_cuda, fmt, d):
    torch = torch_cuda
    for name, kind, W in (("chain_and_fan", "random", 100), ("wide", "star", 0), ("split", "random", 0)):
        want, want_lse = ti.reference(oracle, name, d, fmt, kind, W, "both")
        o, lse = Step(oracle, torch, name, d, fmt).call(fa, torch, W, ti.tree(name, kind)[0], "both")
        dv.check(oracle, ti.layout(name), o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"{name} {kind} W={W} sinks + softcap")


# ---- 2. the exact census of the mask -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain_and_fan", "wide"])
def test_census_of_the_mask(fa, oracle, torch_cuda, name):
    """K = 0, V residue-coded (family Z), fp32 output, d = 64, fp16: O[row, col] * count_row is the number of visible keys of that
    residue -- the prefix keys of the residue plus the mask bit of the one tail key that has it -- decided between integers"""
    torch, d, fmt = torch_cuda, 64, 0
    f, lay = ti.family(name), ti.layout(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    assert lay.max_q <= d, "the tail's keys hit distinct columns"
    z = ci.z_decode(oracle, B, Hkv, G, Nq, Ncap, d, fmt, "residue")
    m_q = np.repeat(np.asarray(z["m"], np.float64), G)
    for ps in (0, 16):
        step = Step(oracle, torch, name, d, fmt, ps=ps, seed=7, bits=z["bits"])
        for kind in ti.TREES:
            for W in ti.WINDOWS:
                vis = ti.visibility(lay, f["lens"], Ncap, G, ti.tree(name, kind)[0], W)
                S, cnt = np.zeros((B * Hkv * G, Nq, d)), np.zeros((B * Hkv * G, Nq))
                for b in range(B):
                    for h in range(Hkv * G):
                        vv = z["v"][b * Hkv + h // G].astype(np.float64)
                        for i in range(lay.n[b]):
                            sel = vis[b][h % G, i]
                            S[b * Hkv * G + h, i] = vv[:sel.size][sel].sum(0)
                            cnt[b * Hkv * G + h, i] = sel.sum()
                assert ci.z_exact(fmt, float(S.max())), "the exactness rule of census_inputs"
                o, lse = step.call(fa, torch, W, ti.tree(name, kind)[0])
                got = dv.unpack_rows(lay, o.cpu().numpy(), B)
                worst = ci.census_check(got, S, cnt, m_q, what=f"{name} {kind} W={W} ps={ps}")
                print(f"{name} {kind} W={W} ps={ps}: census deviation {worst:.3e} (margin {ci.MARGIN})")
                gl = dv.unpack_rows(lay, np.ascontiguousarray(lse.cpu().numpy().T), B, fill=-np.inf)
                with np.errstate(over="ignore"):
                    assert (np.abs(np.exp(gl.astype(np.float64)) - cnt) <= ci.MARGIN).all(), "exp(lse) is the number of visible keys"


# ---- 3. the bits of the causal packed entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ti.NAMES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_triangle_gives_the_bits_of_the_causal_entry(fa, oracle, torch_cuda, fmt, d, name):
    torch = torch_cuda
    assert (ri.want_S(ti.family(name), 0) > 1) == (name == "split")
    tri = ti.triangle(ti.layout(name))
    for ps, fp8 in ((0, False), (16, False), (0, True), (16, True)):
        step = Step(oracle, torch, name, d, fmt, ps=ps, fp8=fp8, seed=ps + 3)
        for W, variant, out_dtype in ((0, "none", torch.float32), (100, "both", step.tdt), (0, "both", torch.float32), (100, "none", step.tdt)):
            what = f"{name} ps={ps} fp8={fp8} W={W} {variant} {out_dtype}"
            plain = step.call(fa, torch, W, None, variant, out_dtype)
            tree = step.call(fa, torch, W, tri, variant, out_dtype)
            for x, y, n in zip(tree, plain, ("O", "lse")):
                assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{what}: {n} differs from the causal entry's in " \
                    f"{int((_bits(torch, x) != _bits(torch, y)).sum())} places"
            _free_tokens_hold_the_sentinel(torch, step.lay, *tree, what)


# ---- 4. tokens of no sequence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain_and_fan", "wide", "split"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_tokens_of_no_sequence_are_neither_read_nor_written(fa, oracle, torch_cuda, fmt, d, name):
    """NaN in the Q rows of tokens that are no live row and other words in their mask entries change no bit of a live row; their O rows
    and lse entries keep the sentinel"""
    torch = torch_cuda
    lay = ti.layout(name)
    words = ti.tree(name, "random")[0]
    other = np.array(words)
    other[~lay.owned] = np.uint64(0)
    assert (words[~lay.owned] == ti.ALL).all() and (~lay.owned).sum() >= 5
    for ps in (0, 16):
        step = Step(oracle, torch, name, d, fmt, ps=ps, seed=5)
        for out_dtype in (torch.float32, step.tdt):
            clean = step.call(fa, torch, 0, other, "sinks", out_dtype, poison=False)
            dirty = step.call(fa, torch, 0, words, "sinks", out_dtype, poison=True)
            for x, y, n in zip(dirty, clean, ("O", "lse")):
                assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{name} ps={ps}: {n} moved under NaN rows and other words of no sequence"
            _free_tokens_hold_the_sentinel(torch, lay, *dirty, f"{name} ps={ps} {out_dtype}")
            t = torch.from_numpy(lay.tok[lay.tok >= 0]).cuda()
            assert torch.isfinite(dirty[0][t]).all() and not torch.isnan(dirty[1][:, t]).any()


# ---- 5. views ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain_and_fan", "split"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_strided_views(fa, oracle, torch_cuda, fmt, d, name):
    torch = torch_cuda
    step = Step(oracle, torch, name, d, fmt)
    B, Hkv, G, Nq, Ncap = ri.shape(step.f)
    Hq, T, tdt = Hkv * G, step.lay.total_q, step.tdt
    words = ti.tree(name, "random")[0]
    q = cm.dev16(torch, dv.pack_rows(step.lay, step.qb, cm.NAN16), fmt)
    base = step.call(fa, torch, 100, words, "both", tdt, q=q)
    fused = torch.full((T, Hq + 2 * Hkv, d), float("nan"), dtype=tdt, device="cuda")
    fused[:, :Hq] = q
    got = step.call(fa, torch, 100, words, "both", tdt, q=fused[:, :Hq])
    assert not fused[:, :Hq].is_contiguous()
    wide = _sentinel_out(torch, (T + 4, Hq + 3, d), tdt)
    before = _bits(torch, wide).clone()
    got_out = step.call(fa, torch, 100, words, "both", tdt, q=q, out=wide[3:3 + T, 2:2 + Hq])
    for g, what in ((got, "fused Q"), (got_out, "out= slice")):
        for x, y, n in zip(g, base, ("O", "lse")):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{what}: {n} differs from the contiguous call"
    after = _bits(torch, wide)
    inside = torch.zeros_like(after, dtype=torch.bool)
    inside[3:3 + T, 2:2 + Hq] = True
    assert torch.equal(after[~inside], before[~inside]), "bytes outside the out= slice changed"


# ---- 6. the append with positions ----------------------------------------------------------------------------------------------------------
def _np_bits(t):
    import torch
    if t.element_size() == 1:
        return t.contiguous().view(torch.uint8).cpu().numpy()
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _append(fa, torch, x, fmt, fp8, rope, pos, op=None):
    """one call on fresh device state, Q rotated into a q_out of its own -> dict of numpy bytes k, v, lens, qout"""
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    dk, dvv = dev(x["kc0"]), dev(x["vc0"])
    dq, dkn, dvn = (cm.dev16(torch, x[n], fmt) for n in ("qsrc", "knb", "vnb"))
    dqo = cm.dev16(torch, np.full(x["qsrc"].shape, av.QOUT_NAN, np.uint16), fmt)
    dl, dcu = _ints(torch, x["lens"]), _ints(torch, x["cu"])
    dt = torch.from_numpy(np.array(x["table"])).cuda() if x["table"] is not None else None
    dks, dvs = _floats(torch, x["ks"]), _floats(torch, x["vs"])
    dpos = None if pos is None else torch.from_numpy(np.array(pos, np.int32)).cuda()
    kw = dict(q=dq, q_out=dqo, rotary_cos=_floats(torch, x["cos"]), rotary_sin=_floats(torch, x["sin"]), rotary_interleaved=rope == 2)
    if op is not None:
        op(dkn, dvn, dk, dvv, dcu, dl, dl, dt, *((dks, dvs) if fp8 else ()), dpos, dq, dqo, kw["rotary_cos"], kw["rotary_sin"], rope == 2)
    elif fp8:
        fa.fa_kvcache_append_varlen_fp8(dkn, dvn, dk, dvv, dcu, dl, dl, dt, dks, dvs, positions=dpos, **kw)
    else:
        fa.fa_kvcache_append_varlen(dkn, dvn, dk, dvv, dcu, dl, dl, dt, positions=dpos, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(_np_bits(dq), x["qsrc"]), "the source Q was written"
    return dict(k=_np_bits(dk), v=_np_bits(dvv), lens=dl.cpu().numpy(), qout=_np_bits(dqo))


def _same(got, want, what):
    for n in ("k", "v", "lens", "qout"):
        assert np.array_equal(got[n], want[n]), f"{what}: {n} differs"


ROPE_FORMS = [pytest.param(p, q, r, id=av.form_id(p, q, r)) for p in (False, True) for q in (False, True) for r in (1, 2)]


@pytest.mark.parametrize("paged,fp8,rope", ROPE_FORMS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_append_with_positions(fa, torch_cuda, fmt, d, paged, fp8, rope):
    """all eight forms, both pair conventions: the bytes of the numpy restatement at the clamped table row -- positions just past
    max_pos and negative among them, NaN rows and unreadable positions in the rows of no sequence -- and the plain call's bytes with
    positions = L_b + i"""
    torch = torch_cuda
    x = av.inputs(fmt, d, paged, fp8, rope)
    pos = ti.append_positions(x)
    own = av.owned(x["cu"], x["total"])
    assert (pos[own] >= av.CASE["max_pos"]).any() and (pos[own] < 0).any() and (x["qsrc"][~own] == cm.NAN16).all()
    got = _append(fa, torch, x, fmt, fp8, rope, pos)
    _same(got, ti.append_model(fmt, d, paged, fp8, rope, pos), "positions")
    assert (got["qout"][~own] == av.QOUT_NAN).all() and not (got["qout"][own] == av.QOUT_NAN).any()
    plain = _append(fa, torch, x, fmt, fp8, rope, None)
    _same(plain, av.model(fmt, d, paged, fp8, rope), "no positions")
    _same(_append(fa, torch, x, fmt, fp8, rope, ti.append_positions(x, "slot")), plain, "positions = L_b + i")
    assert not np.array_equal(got["k"], plain["k"]) and np.array_equal(got["v"], plain["v"])


# ---- 7. end to end: the tree step ----------------------------------------------------------------------------------------------------------
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
def test_tree_step_end_to_end(fa, oracle, torch_cuda, d, fp8):
    """append_varlen(positions = L + depth, rotary) from a fused buffer, then the tree decode; the float64 reference on what the append
    left.  Second oracle: for one leaf per sequence the LINEAR sequence prefix + root-to-leaf path through the plain append_varlen
    and decode_varlen(causal=True): the leaf's O and lse agree within the sum of both sides' bounds against float64 (the key order
    differs, so not bit for bit)."""
    torch = torch_cuda
    fmt, B, Hkv, G, Ncap, ps, max_q = 0, 3, 2, 2, 256, 16, 64
    Hq = Hkv * G
    before, m = [130, 61, 0], [13, 64, 5]
    cu = np.cumsum([2] + m)
    T = int(cu[-1]) + 3
    after = [L + x for L, x in zip(before, m)]
    rng = np.random.default_rng(9600 + d)
    parents = np.full(T, -1, np.int32)
    for b in range(B):
        parents[cu[b]:cu[b + 1]] = ti.parents_of("random", m[b], rng)
    dcu = _ints(torch, cu)
    mask, depth = fa.tree_from_parents(torch.from_numpy(parents).cuda(), dcu)
    assert mask.is_cuda and mask.dtype == torch.int64 and depth.dtype == torch.int32
    pos = depth.clone()
    for b in range(B):
        pos[cu[b]:cu[b + 1]] += before[b]                 # positions = L_before[b] + depth
    (_, k, v), (_, kb, vb) = di.inputs(oracle, B, Hkv, G, 1, Ncap, d, fmt, 9601)
    tokens = torch.from_numpy(rng.uniform(-1, 1, (T, Hq + 2 * Hkv, d)).astype(np.float32)).cuda().to(torch.float16)
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    ks, vs = (_floats(torch, KS[:Hkv]), _floats(torch, VS[:Hkv])) if fp8 else (None, None)

    def caches(lens_after):
        if fp8:
            return (cm.dev8(torch, cm.poisoned(f8.encode(k).reshape(B, Hkv, Ncap, d), before, nan=f8.NAN_CODES[0])),
                    cm.dev8(torch, cm.poisoned(f8.encode(v).reshape(B, Hkv, Ncap, d), before, nan=f8.NAN_CODES[0])), None, None)
        kp, vp, tb = cm.scatter(kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), lens_after, ps, 9602)
        return cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(tb).cuda(), tb

    def step(fused, cu_dev, lens_after, nmax, positions, tree_mask):
        kc, vc, table, tb = caches(lens_after)
        dl = _ints(torch, before)
        kw = dict(cache_seqlens=dl, seqlens_out=dl, block_table=table, q=fused[:, :Hq], rotary_cos=cos, rotary_sin=sin, positions=positions)
        if fp8:
            fa.fa_kvcache_append_varlen_fp8(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, cu_dev, k_scale=ks, v_scale=vs, **kw)
            o, lse = fa.fa_kvcache_decode_varlen_fp8(fused[:, :Hq], kc, vc, cu_dev, nmax, dl, k_scale=ks, v_scale=vs, causal=True,
                                                     return_lse=True, tree_mask=tree_mask)
        else:
            fa.fa_kvcache_append_varlen(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, cu_dev, **kw)
            o, lse = fa.fa_kvcache_decode_varlen(fused[:, :Hq], kc, vc, cu_dev, nmax, dl, table, causal=True, return_lse=True,
                                                 tree_mask=tree_mask)
        torch.cuda.synchronize()
        assert dl.tolist() == list(lens_after)
        return o, lse, kc, vc, tb

    fused = tokens.clone()
    o, lse, kc, vc, tb = step(fused, dcu, after, max_q, pos, mask)
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
    words = mask.cpu().numpy().view(np.uint64)
    vis = ti.visibility(lay, after, Ncap, G, words, 0)
    want, want_lse = ti.expected_f64(qrot, kf.reshape(B * Hkv, Ncap, d), vf.reshape(B * Hkv, Ncap, d), vis, B, Hkv, G, max_q)
    free = torch.from_numpy(~lay.owned).cuda()
    assert (o[free] == 0).all() and (lse[:, free] == float("-inf")).all()
    dv.check(oracle, lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, "append_varlen(positions) -> tree decode", sentinel=False)
    # the linear sequences of one leaf each: the deepest token of every tree
    dep = depth.cpu().numpy()
    paths = []
    for b in range(B):
        i = int(np.argmax(dep[cu[b]:cu[b + 1]]))
        path = [j for j in range(m[b]) if (int(words[cu[b] + i]) >> j) & 1]
        assert path[-1] == i and len(path) == dep[cu[b] + i] + 1
        paths.append(path)
    cu2 = np.cumsum([0] + [len(p) for p in paths])
    rows = torch.tensor([int(cu[b]) + j for b in range(B) for j in paths[b]], device="cuda")
    lin = tokens[rows].clone()
    after2 = [L + len(p) for L, p in zip(before, paths)]
    o2, lse2, *_ = step(lin, _ints(torch, cu2), after2, max(len(p) for p in paths), None, None)
    leaf_tree = torch.tensor([int(cu[b]) + paths[b][-1] for b in range(B)], device="cuda")
    leaf_lin = torch.tensor([int(cu2[b + 1]) - 1 for b in range(B)], device="cuda")
    diff = float((o[leaf_tree] - o2[leaf_lin]).abs().max())
    ldiff = float((lse[:, leaf_tree] - lse2[:, leaf_lin]).abs().max())
    print(f"leaf rows, tree step against the linear sequence: max_abs={diff:.3e} lse_abs={ldiff:.3e} "
          f"(bounds {2 * cm.MAX_ABS:.1e} {4 * cm.P_EPS[fmt]:.2e})")
    assert torch.isfinite(o2[leaf_lin]).all() and diff <= 2 * cm.MAX_ABS and ldiff <= 4 * cm.P_EPS[fmt]


# ---- 8. the captured step ------------------------------------------------------------------------------------------------------------------
def test_captured_tree_step(fa, oracle, torch_cuda):
    """append_varlen(positions) -> tree decode behind a split, captured once; replayed on other trees with the masks, the positions, the
    vector, the lengths and the table rewritten in place; each replay equals the eager call bit for bit"""
    torch = torch_cuda
    d, B, Hkv, G, Ncap, ps, max_q, T = 64, 2, 1, 2, 8192, 16, 5, 12
    Hq, max_pages = Hkv * G, Ncap // ps
    num_pages = B * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(9650)
    pool = lambda: (torch.rand((num_pages, Hkv, ps, d), device="cuda", generator=gen) * 2 - 1).to(torch.float16)
    kp0, vp0 = pool(), pool()
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, max_q, d, max_pages=max_pages, page_size=ps)
    assert need > 0                                       # S > 1: the merge is in the graph
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    fused = torch.zeros(T, Hq + 2 * Hkv, d, dtype=torch.float16, device="cuda")
    kp, vp = kp0.clone(), vp0.clone()
    cu, lens = _ints(torch, [0, 1, 2]), _ints(torch, [0, 0])
    table = torch.zeros(B, max_pages, dtype=torch.int32, device="cuda")
    mask = torch.ones(T, dtype=torch.int64, device="cuda")
    pos = torch.zeros(T, dtype=torch.int32, device="cuda")
    out = torch.zeros(T, Hq, d, dtype=torch.float32, device="cuda")
    lse = torch.zeros(Hq, T, dtype=torch.float32, device="cuda")

    def step(fz, ck, cv, cl, o, l):
        fa.fa_kvcache_append_varlen(fz[:, Hq:Hq + Hkv], fz[:, Hq + Hkv:], ck, cv, cu, cache_seqlens=cl, seqlens_out=cl, block_table=table,
                                    q=fz[:, :Hq], rotary_cos=cos, rotary_sin=sin, positions=pos)
        fa.fa_kvcache_decode_varlen(fz[:, :Hq], ck, cv, cu, max_q, cl, table, causal=True, out=o, lse=l, workspace=ws, tree_mask=mask)

    def state(s):
        g = torch.Generator(device="cuda").manual_seed(9700 + s)
        tokens = (torch.rand((T, Hq + 2 * Hkv, d), device="cuda", generator=g) * 2 - 1).to(torch.float16)
        vec = ([1, 6, 10], [0, 3, 8], [2, 2, 9])[s]      # n = (5, 4); (3, 5); (0, 5 of 7: cut at max_q)
        L = ([8000, 4100], [37, 8100], [5000, 0])[s]
        par = np.full(T, -1, np.int32)
        rng = np.random.default_rng(9800 + s)
        for b in range(B):
            n = vec[b + 1] - vec[b]
            par[vec[b]:vec[b + 1]] = ti.parents_of(("random", "star", "chain")[s], n, rng) if n else []
        vec_dev = _ints(torch, vec)
        m, dep = fa.tree_from_parents(torch.from_numpy(par).cuda(), vec_dev)
        p = dep.clone()
        for b in range(B):
            p[vec[b]:vec[b + 1]] += L[b]
        perm = torch.randperm(num_pages, device="cuda", generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
        return tokens, vec_dev, _ints(torch, L), perm, m, p

    step(fused.clone(), kp.clone(), vp.clone(), lens.clone(), out.clone(), lse.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(fused, kp, vp, lens, out, lse)
    results = []
    for s in range(3):
        tokens, vec, L, perm, m, p = state(s)
        for dst, src in ((fused, tokens), (cu, vec), (lens, L), (table, perm), (mask, m), (pos, p), (kp, kp0), (vp, vp0)):
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
        lay = dv.Layout(vec.tolist(), T, max_q)
        t = torch.from_numpy(lay.tok[lay.tok >= 0]).cuda()
        assert torch.isfinite(out[t]).all() and torch.isfinite(lse[:, t]).all(), s
        free = torch.from_numpy(~lay.owned).cuda()
        assert (out[free] == dv.SENTINEL_LSE).all() and (lse[:, free] == dv.SENTINEL_LSE).all(), s
        results.append(out[t].clone())
    assert not torch.equal(results[0][:3], results[1][:3]), "the replays follow their inputs"


# ---- 9. the torch ops ----------------------------------------------------------------------------------------------------------------------
def test_ops_are_the_front_ends(fa, oracle, torch_cuda):
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    name, d, fmt = "chain_and_fan", 128, 1
    sc = 1.0 / np.sqrt(d)
    mask = _words(torch, ti.tree(name, "random")[0])
    for fp8, ps in ((False, 0), (False, 16), (True, 0)):
        step = Step(oracle, torch, name, d, fmt, ps=ps, fp8=fp8, seed=4)
        Hq = step.f["Hkv"] * step.f["G"]
        q = cm.dev16(torch, dv.pack_rows(step.lay, step.qb, 0), fmt)
        cu, sk = _ints(torch, step.lay.cu), _floats(torch, li.sinks_for(Hq))
        kw = dict(cache_seqlens=step.lens, block_table=step.table, causal=True, scale=sc, window=100, sinks=sk, softcap=li.SOFTCAP,
                  out_dtype=torch.float32, return_lse=True, tree_mask=mask)
        if fp8:
            got = ops.decode_varlen_tree_fp8(q, step.k, step.v, cu, step.lay.max_q, step.lens, step.table, mask, *step.scales, sc, True, 100,
                                             sk, li.SOFTCAP, True)
            want = fa.fa_kvcache_decode_varlen_fp8(q, step.k, step.v, cu, step.lay.max_q, k_scale=step.scales[0], v_scale=step.scales[1], **kw)
        else:
            got = ops.decode_varlen_tree(q, step.k, step.v, cu, step.lay.max_q, step.lens, step.table, mask, sc, True, 100, sk, li.SOFTCAP, True)
            want = fa.fa_kvcache_decode_varlen(q, step.k, step.v, cu, step.lay.max_q, **kw)
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y) and not torch.isnan(x).any(), (fp8, ps)
    for paged, fp8 in ((False, False), (True, True)):
        x = av.inputs(0, 64, paged, fp8, 1)
        pos = ti.append_positions(x)
        want = _append(fa, torch, x, 0, fp8, 1, pos)
        _same(_append(fa, torch, x, 0, fp8, 1, pos, op=ops.append_varlen_pos_fp8 if fp8 else ops.append_varlen_pos), want, "the op")
