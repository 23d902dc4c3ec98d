"""GPU tier of the packed append fa_kvcache_append_varlen (ops.fa_kvcache_append_varlen, _fp8).

Inputs and the numpy expectation are tests/append_varlen_inputs.py's; its CPU tier (tests/test_append_varlen_inputs.py) shows that the
byte comparison here tells the right kernel from six wrong ones.  Everything the append writes is compared bit for bit; the end-to-end
step is judged at the bounds of tests/test_gpu_varlen_cache.py (varlen_inputs.problems: cm.MAX_ABS, cm.REL_L2, 2 * cm.P_EPS).

Poison: every cache row and pool page holds a NaN pattern before a call, every source row of no sequence holds NaN, a q_out of its own
holds another NaN pattern, every table entry no kept token needs holds garbage.
"""
import numpy as np
import pytest

import append_inputs as ai
import append_varlen_inputs as av
import common_inputs as cm
import fp8_inputs as f8
import rope_inputs as rp
import varlen_cache_fp8_inputs as v8
import varlen_inputs as vi
import varlen_logit_inputs as li

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
FORMS = [pytest.param(*f, id=av.form_id(*f)) for f in av.FORMS]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ints(torch, values):
    return None if values is None else torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _floats(torch, values):
    return None if values is None else torch.tensor(np.asarray(values, np.float32), dtype=torch.float32, device="cuda")


def _bits(t):
    """a device tensor -> its bytes as numpy uint16 (16-bit types) or uint8 (fp8)"""
    import torch
    if t.element_size() == 1:
        return t.contiguous().view(torch.uint8).cpu().numpy()
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


LAYOUTS = ("packed", "fused", "head_major", "padded")


def _lay(torch, bits, fmt, layout, pad=64):
    """(total, H, d) encodings -> a device tensor with those rows in the given memory layout"""
    total, H, d = bits.shape
    if layout == "head_major":   # stride_t = d
        return cm.dev16(torch, np.ascontiguousarray(bits.transpose(1, 0, 2)), fmt).transpose(0, 1)
    if layout == "padded":       # stride_t = H * d + pad, the padding poisoned
        buf = cm.dev16(torch, np.full((total, H * d + pad), cm.NAN16, np.uint16), fmt)
        view = buf.as_strided((total, H, d), (H * d + pad, d, 1))
        view.copy_(cm.dev16(torch, bits, fmt))
        return view
    return cm.dev16(torch, bits, fmt)


def _launch(fa, torch, x, fmt, fp8, rope, layout="packed", in_place=False, lens_in_place=True, op=None):
    """one call on fresh device state -> dict of numpy bytes: k, v (whole cache or pool), lens, qout, and the sources after the call
    (knb, vnb, qsrc).  layout: how the sources lie (LAYOUTS; "fused": views of one (total, Hq + 2 Hkv, d) buffer).  in_place: Q is
    rotated where it lies, else into a q_out of its own that holds av.QOUT_NAN.  op: a torch op to call in the place of the front end."""
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    dk, dv = dev(x["kc0"]), dev(x["vc0"])
    Hkv, Hq = x["knb"].shape[1], x["qsrc"].shape[1]
    if layout == "fused":
        fused = cm.dev16(torch, np.concatenate([x["qsrc"], x["knb"], x["vnb"]], axis=1), fmt)
        dq, dkn, dvn = fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
    else:
        dq, dkn, dvn = (_lay(torch, x[n], fmt, layout) for n in ("qsrc", "knb", "vnb"))
    dqo = None
    if rope and not in_place:
        dqo = _lay(torch, np.full(x["qsrc"].shape, av.QOUT_NAN, np.uint16), fmt, "packed" if layout == "fused" else layout, pad=128)
    dl = _ints(torch, x["lens"])
    dout = dl if lens_in_place else torch.full_like(dl, -777)
    dcu, dt = _ints(torch, x["cu"]), (torch.from_numpy(np.array(x["table"])).cuda() if x["table"] is not None else None)
    dks, dvs = _floats(torch, x["ks"]), _floats(torch, x["vs"])
    dcos, dsin = (_floats(torch, x["cos"]), _floats(torch, x["sin"])) if rope else (None, None)
    rot = (dq if rope else None, dqo, dcos, dsin, rope == 2)
    if op is not None:
        op(dkn, dvn, dk, dv, dcu, dl, dout, dt, *((dks, dvs) if fp8 else ()), *rot)
    else:
        kw = dict(q=rot[0], q_out=rot[1], rotary_cos=rot[2], rotary_sin=rot[3], rotary_interleaved=rot[4])
        if fp8:
            fa.fa_kvcache_append_varlen_fp8(dkn, dvn, dk, dv, dcu, dl, dout, dt, dks, dvs, **kw)
        else:
            fa.fa_kvcache_append_varlen(dkn, dvn, dk, dv, dcu, dl, dout, dt, **kw)
    torch.cuda.synchronize()
    if not lens_in_place:
        assert dl.tolist() == [int(v) for v in x["lens"]], "seqlens_k was written although seqlens_out is a buffer of its own"
    return dict(k=_bits(dk), v=_bits(dv), lens=dout.cpu().numpy(), qout=_bits(dq if in_place else dqo) if rope else None,
                knb=_bits(dkn), vnb=_bits(dvn), qsrc=_bits(dq))


def _same(got, want, what, names=("k", "v", "lens", "qout")):
    for n in names:
        if want[n] is None:
            assert got[n] is None, (what, n)
        else:
            assert np.array_equal(got[n], want[n]), f"{what}: {n} differs"


# ---- 1. bytes against numpy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,rope", FORMS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bytes_against_numpy(fa, torch_cuda, fmt, d, paged, fp8, rope):
    """every byte of the caches or pools, of q_out and of seqlens_out is the numpy expectation's: what no kept token touches -- cache
    rows, pool pages, q_out rows of no sequence -- holds the NaN pattern it held, and the sources are as they were"""
    x = av.inputs(fmt, d, paged, fp8, rope)
    want = av.model(fmt, d, paged, fp8, rope)
    got = _launch(fa, torch_cuda, x, fmt, fp8, rope)
    _same(got, want, "a q_out of its own")
    for n in ("knb", "vnb", "qsrc"):
        assert np.array_equal(got[n], x[n]), f"the source {n} was written"
    nan = 0x7F if fp8 else cm.NAN16
    assert (got["k"] == nan).all(-1).sum() == (want["k"] == nan).all(-1).sum() > 0
    if rope:
        own = av.owned(x["cu"], x["total"])
        assert (got["qout"][~own] == av.QOUT_NAN).all() and not (got["qout"][own] == av.QOUT_NAN).any()
        inp = _launch(fa, torch_cuda, x, fmt, fp8, rope, in_place=True, lens_in_place=False)
        _same(inp, av.model(fmt, d, paged, fp8, rope, qout0=x["qsrc"]), "Q rotated in place, seqlens_out a buffer of its own")
        assert (inp["qout"][~own] == cm.NAN16).all()


# ---- 2. bytes against the padded entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,rope", FORMS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bytes_against_the_padded_entry(fa, torch_cuda, fmt, d, paged, fp8, rope):
    """the same call against fa_kvcache_append_ex(seqlens_new = m) on the padded head-major copy of the same rows: caches or pools,
    rotated Q rows and seqlens_out bit for bit"""
    torch = torch_cuda
    x = av.inputs(fmt, d, paged, fp8, rope)
    got = _launch(fa, torch, x, fmt, fp8, rope, in_place=True)
    rows = av.token_rows(x["cu"], x["total"])
    m = [len(r) for r in rows]
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    dk, dv, dl = dev(x["kc0"]), dev(x["vc0"]), _ints(torch, x["lens"])
    dkn, dvn, dq = (cm.dev16(torch, av.gather(x[n], rows), fmt) for n in ("knb", "vnb", "qsrc"))
    assert dkn.shape[2] == max(m)
    fn = getattr(fa, "fa_kvcache_append" + ("_paged" if paged else "") + ("_fp8" if fp8 else ""))
    args = [dkn, dvn, dk, dv] + ([torch.from_numpy(np.array(x["table"])).cuda()] if paged else [])
    kw = dict(cache_seqlens=dl, seqlens_out=dl, seqlens_new=_ints(torch, m))
    if fp8:
        kw.update(k_scale=_floats(torch, x["ks"]), v_scale=_floats(torch, x["vs"]))
    if rope:
        kw.update(q=dq, rotary_cos=_floats(torch, x["cos"]), rotary_sin=_floats(torch, x["sin"]), rotary_interleaved=rope == 2)
    fn(*args, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(got["k"], _bits(dk)) and np.array_equal(got["v"], _bits(dv)), "the caches differ from the padded entry's"
    assert got["lens"].tolist() == dl.tolist()
    if rope:
        qpad = _bits(dq)
        for b, r in enumerate(rows):
            if r:
                assert np.array_equal(got["qout"][r], qpad[b, :, :len(r)].transpose(1, 0, 2)), f"rotated Q rows of sequence {b}"


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,rope", [pytest.param(*f, id=av.form_id(*f)) for f in ((False, False, 1), (True, True, 2), (True, False, 0))])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_layouts_give_identical_bytes(fa, torch_cuda, fmt, d, paged, fp8, rope):
    """views of one fused (total, Hq + 2 Hkv, d) buffer with Q rotated in place inside it, head-major views (stride_t = d) and a
    padded stride_t: the bytes of the packed contiguous call"""
    x = av.inputs(fmt, d, paged, fp8, rope)
    want = av.model(fmt, d, paged, fp8, rope, qout0=x["qsrc"])
    for layout in LAYOUTS[1:]:
        got = _launch(fa, torch_cuda, x, fmt, fp8, rope, layout=layout, in_place=True)
        _same(got, want, layout + ", in place")
        assert np.array_equal(got["knb"], x["knb"]) and np.array_equal(got["vnb"], x["vnb"]), layout   # the neighbours in the buffer
        if rope and layout != "fused":
            _same(_launch(fa, torch_cuda, x, fmt, fp8, rope, layout=layout), av.model(fmt, d, paged, fp8, rope), layout + ", q_out")


# ---- 4. clamps with a defined result -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,rope", [pytest.param(*f, id=av.form_id(*f)) for f in ((False, False, 0), (True, False, 1), (False, True, 2))])
def test_clamped_vectors(fa, torch_cuda, paged, fp8, rope):
    """cu = [-5, 10, 10, 500] on total_new = 64 is (0, 10), (10, 10), (10, 64); seqlens_k = (-7, 1000, 20) is (0, Ncap, 20)"""
    fmt, d = 1, 64
    x = av.inputs(fmt, d, paged, fp8, rope, split=((-5, 10, 10, 500), 64, (-7, 1000, 20)))
    assert av.bounds(x["cu"], 64) == [(0, 10), (10, 10), (10, 64)]
    want = av.model(fmt, d, paged, fp8, rope, x=x)
    assert want["lens"].tolist() == [10, av.CASE["Ncap"], 74]
    _same(_launch(fa, torch_cuda, x, fmt, fp8, rope), want, "clamped cu_seqlens_new and seqlens_k")


# ---- 5. the mixed step, end to end -------------------------------------------------------------------------------------------------------
def _judge(fmt, o, lse, want, want_lse, cu_q, what):
    own = vi.owned(cu_q, o.shape[0])
    got, got_lse = o.float().cpu().numpy(), lse.float().cpu().numpy()
    ma, rl, le = vi.figures(got, got_lse, want, want_lse, own)
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    found = vi.problems(got, got_lse, want, want_lse, own, fmt)
    assert not found, f"{what}: {found}"


@pytest.mark.parametrize("fp8", (False, True), ids=("fp16_pages", "fp8_contiguous"))
def test_mixed_step_end_to_end(fa, torch_cuda, fp8):
    """two prompt chunks and one decode token packed in a fused buffer: append_varlen with rotary (lengths in place), then
    fa_forward_varlen_kvcache on the rotated Q view with cu_seqlens_q = cu_seqlens_new -- twice, so the second step starts at L_b > 0.
    Against varlen_logits_f64 on numpy-rotated data (fp8: the fp8 tier's reference on the decoded codes)."""
    torch = torch_cuda
    fmt, d, Hkv, G, ps, Ncap, B, tail = 0, 64, 2, 2, 16, 128, 3, 5
    Hq = Hkv * G
    steps = ((40, 25, 1), (33, 50, 1))
    cos, sin = rp.real_table(Ncap, d)
    ks, vs = (np.array([0.75, 1.5], np.float32), np.array([1.25, 0.5], np.float32)) if fp8 else (None, None)
    rng = np.random.default_rng(9200)
    max_pages = Ncap // ps
    table = None if fp8 else rng.permutation(B * max_pages + 3)[:B * max_pages].astype(np.int32).reshape(B, max_pages)
    if fp8:
        dk, dv = (cm.dev8(torch, np.full((B, Hkv, Ncap, d), v8.NAN8, np.uint8)) for _ in range(2))
    else:
        dk, dv = (cm.dev16(torch, np.full((B * max_pages + 3, Hkv, ps, d), cm.NAN16, np.uint16), fmt) for _ in range(2))
    dt = None if fp8 else torch.from_numpy(table).cuda()
    dl = _ints(torch, [0] * B)
    dcos, dsin = _floats(torch, cos), _floats(torch, sin)
    dks, dvs = _floats(torch, ks), _floats(torch, vs)
    hist_k, hist_v = [[] for _ in range(B)], [[] for _ in range(B)]   # what the cache holds, as values: per sequence (Hkv, d) rows
    lens = [0] * B
    for s, m in enumerate(steps):
        total = sum(m) + tail
        cu = vi.cu_of(m)
        bits = np.full((total, Hq + 2 * Hkv, d), cm.NAN16, np.uint16)
        bits[:sum(m)] = ai.round16_bits(rng.standard_normal((sum(m), Hq + 2 * Hkv, d)).astype(np.float32), fmt)
        pos = np.zeros(total, np.int64)
        for b in range(B):
            pos[cu[b]:cu[b + 1]] = lens[b] + np.arange(m[b])
        x = ai.widen16(bits[:sum(m)], fmt)
        c, sn = cos[pos[:sum(m)]][:, None], sin[pos[:sum(m)]][:, None]
        qrot = np.zeros((total, Hq, d), np.float32)
        qrot[:sum(m)] = ai.widen16(ai.round16_bits(rp.rotate_fp32(x[:, :Hq], c, sn, False), fmt), fmt)
        krot = rp.rotate_fp32(x[:, Hq:Hq + Hkv], c, sn, False)
        if fp8:
            kval = f8.decode(rp.fp8_codes(krot.transpose(1, 0, 2)[None], ks)[0]).transpose(1, 0, 2)
            vval = f8.decode(rp.fp8_codes(x[:, Hq + Hkv:].transpose(1, 0, 2)[None], vs)[0]).transpose(1, 0, 2)
        else:
            kval, vval = ai.widen16(ai.round16_bits(krot, fmt), fmt), x[:, Hq + Hkv:]
        for b in range(B):
            hist_k[b].extend(kval[cu[b]:cu[b + 1]]), hist_v[b].extend(vval[cu[b]:cu[b + 1]])
            lens[b] += m[b]
        fused = cm.dev16(torch, bits, fmt)
        q, kn, vn = fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
        dcu = _ints(torch, cu)
        out = torch.full((total, Hq, d), vi.POISON, dtype=torch.float32, device="cuda")
        lse = torch.full((Hq, total), vi.POISON, dtype=torch.float32, device="cuda")
        rot = dict(q=q, rotary_cos=dcos, rotary_sin=dsin)
        if fp8:
            fa.fa_kvcache_append_varlen_fp8(kn, vn, dk, dv, dcu, dl, dl, None, dks, dvs, **rot)
            fa.fa_forward_varlen_kvcache_fp8(q, dk, dv, dcu, dl, k_scale=dks, v_scale=dvs, causal=True, out=out, lse=lse)
        else:
            fa.fa_kvcache_append_varlen(kn, vn, dk, dv, dcu, dl, dl, dt, **rot)
            fa.fa_forward_varlen_kvcache(q, dk, dv, dcu, dl, block_table=dt, causal=True, out=out, lse=lse)
        torch.cuda.synchronize()
        assert dl.tolist() == lens, s
        kall, vall = (np.concatenate([np.stack(h[b]) for b in range(B)]).astype(np.float32) for h in (hist_k, hist_v))
        cu_k = vi.cu_of(lens)
        scale = 1.0 / np.sqrt(d)
        if fp8:
            ref = dict(q=qrot, k=kall, v=vall, cu_q=cu, cu_k=cu_k, Hkv=Hkv, G=G, causal=True, scale=scale, W=0, softcap=0.0, sinks=None,
                       k_scale=ks, v_scale=vs)
            want, want_lse = v8.reference_f64(ref)
        else:
            want, want_lse = li.varlen_logits_f64(qrot, kall, vall, cu, cu_k, Hkv, G, True, scale)
        _judge(fmt, out, lse, want, want_lse, cu, f"mixed step {s} ({'fp8 contiguous' if fp8 else 'fp16 pages of 16'}), lengths {lens}")


# ---- 6. the captured call ----------------------------------------------------------------------------------------------------------------
def test_captured_step_follows_rewritten_vectors(fa, torch_cuda):
    """append_varlen + fa_forward_varlen_kvcache captured once as a linear graph, replayed after cu_seqlens_new, the lengths and the
    table were rewritten in place to another split of the same total_new: the bytes of the eager calls"""
    torch = torch_cuda
    fmt, d, paged, fp8, rope = 0, 64, True, False, 1
    base = av.inputs(fmt, d, paged, fp8, rope)
    total, Hkv, Hq = base["total"], base["knb"].shape[1], base["qsrc"].shape[1]
    other = av.inputs(fmt, d, paged, fp8, rope, split=((0, 50, 51, 51, 90, 132), total, (30, 0, 7, 95, 60)))
    assert other["table"].shape == base["table"].shape and not np.array_equal(other["table"], base["table"])
    dcos, dsin = _floats(torch, base["cos"]), _floats(torch, base["sin"])

    def state(x):
        fused = cm.dev16(torch, np.concatenate([x["qsrc"], x["knb"], x["vnb"]], axis=1), fmt)
        return dict(fused=fused, k=cm.dev16(torch, x["kc0"], fmt), v=cm.dev16(torch, x["vc0"], fmt), cu=_ints(torch, x["cu"]),
                    lens=_ints(torch, x["lens"]), table=torch.from_numpy(np.array(x["table"])).cuda(),
                    o=torch.full((total, Hq, d), vi.POISON, dtype=torch.float32, device="cuda"),
                    lse=torch.full((Hq, total), vi.POISON, dtype=torch.float32, device="cuda"))

    def step(s):
        q, kn, vn = s["fused"][:, :Hq], s["fused"][:, Hq:Hq + Hkv], s["fused"][:, Hq + Hkv:]
        fa.fa_kvcache_append_varlen(kn, vn, s["k"], s["v"], s["cu"], s["lens"], s["lens"], s["table"], q=q, rotary_cos=dcos, rotary_sin=dsin)
        fa.fa_forward_varlen_kvcache(q, s["k"], s["v"], s["cu"], s["lens"], block_table=s["table"], causal=True, out=s["o"], lse=s["lse"])

    eager = {}
    for name, x in (("base", base), ("other", other)):
        eager[name] = state(x)
        step(eager[name])
    torch.cuda.synchronize()
    _same(dict(k=_bits(eager["other"]["k"]), v=_bits(eager["other"]["v"]), lens=eager["other"]["lens"].cpu().numpy(),
               qout=_bits(eager["other"]["fused"][:, :Hq])), av.model(fmt, d, paged, fp8, rope, qout0=other["qsrc"], x=other), "the other split, eager")
    g = state(base)
    fresh = {n: g[n].clone() for n in ("fused", "k", "v")}
    step({n: t.clone() for n, t in g.items()})   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(g)
    for name, x in (("base", base), ("other", other), ("base", base)):
        for n in ("fused", "k", "v"):
            g[n].copy_(fresh[n] if n != "fused" else cm.dev16(torch, np.concatenate([x["qsrc"], x["knb"], x["vnb"]], axis=1), fmt))
        g["cu"].copy_(_ints(torch, x["cu"])), g["lens"].copy_(_ints(torch, x["lens"])), g["table"].copy_(torch.from_numpy(np.array(x["table"])).cuda())
        g["o"].fill_(vi.POISON), g["lse"].fill_(vi.POISON)
        graph.replay()
        torch.cuda.synchronize()
        # bit for bit: the caches start as NaN patterns below the starting lengths, so O holds NaN where a row sees such a key
        for n in ("fused", "k", "v", "lens", "o", "lse"):
            as_int = torch.int16 if g[n].element_size() == 2 else torch.int32
            assert torch.equal(g[n].view(as_int), eager[name][n].view(as_int)), (name, n)
        assert not torch.equal(g["o"].view(torch.int32), torch.full_like(g["o"], vi.POISON).view(torch.int32))


# ---- 7. the torch ops --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,rope", [pytest.param(*f, id=av.form_id(*f)) for f in ((False, False, 0), (True, False, 1), (False, True, 1),
                                                                                         (True, True, 2))])
def test_torch_ops_return_the_front_ends_bytes(fa, torch_cuda, paged, fp8, rope):
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch_cuda.ops.fa_mi355
    fmt, d = 1, 128
    x = av.inputs(fmt, d, paged, fp8, rope)
    op = ops.append_varlen_fp8 if fp8 else ops.append_varlen
    for in_place in (True, False) if rope else (True,):
        for layout in ("fused", "packed"):
            got = _launch(fa, torch_cuda, x, fmt, fp8, rope, layout=layout, in_place=in_place, op=op)
            want = _launch(fa, torch_cuda, x, fmt, fp8, rope, layout=layout, in_place=in_place)
            _same(got, want, f"{layout}, in_place={in_place}", names=("k", "v", "lens", "qout", "knb", "vnb", "qsrc"))
            _same(got, av.model(fmt, d, paged, fp8, rope, qout0=None if not in_place else x["qsrc"]), "against numpy")
