"""GPU tier of fa_kvcache_commit (fa.fa_kvcache_commit, torch.ops.fa_mi355.commit) and fa.tree_accept_mask: the commit step of tree
speculation.

Inputs and the numpy model are tests/commit_inputs.py's; its CPU tier shows that ten wrong kernels fail the comparison made here.
Everything is bit for bit: the entry moves bytes, so there is no tolerance anywhere in this file.
"""
import numpy as np
import pytest

import commit_inputs as cmi
import common_inputs as cm
import decode_inputs as di
import fp8_inputs as f8
import rope_inputs as rp
import tree_inputs as ti

pytestmark = pytest.mark.gpu

FORM_FMT_D = [pytest.param(p, f, fmt, d, id=f"{cmi.form_id(p, f)}-{'e4m3' if f else cm.FMT_NAME[fmt]}-d{d}")
              for p, f in cmi.FORMS for fmt in ((0,) if f else (0, 1)) for d in (64, 128)]
KS, VS = (0.5, 0.75), (2.0, 1.5)   # per-head scales of the fp8 step


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


def _np_bits(torch, t):
    if t.element_size() == 1:
        return t.contiguous().view(torch.uint8).cpu().numpy()
    if t.element_size() == 4:
        return t.contiguous().view(torch.int32).cpu().numpy()
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _dev(torch, a, fp8, fmt):
    return cm.dev8(torch, a) if fp8 else cm.dev16(torch, a, fmt)


def _commit(fa, torch, x, fp8, fmt, mode, op=None):
    """one call on fresh device state -> (k, v, lens_out) as numpy bytes; mode: one of cmi.LENS_MODES"""
    dk, dvv = _dev(torch, x["k0"], fp8, fmt), _dev(torch, x["v0"], fp8, fmt)
    words = _words(torch, x["words"])
    table = None if x["table"] is None else torch.from_numpy(np.array(x["table"])).cuda()
    lens = _ints(torch, x["lens"])
    assert (lens is None) == (mode == "null")
    out = lens if mode == "in_place" else torch.full((len(x["words"]),), -77, dtype=torch.int32, device="cuda")
    if op is not None:
        assert op(dk, dvv, words, lens, out, table, x["max_new"]) is None
    else:
        fa.fa_kvcache_commit(dk, dvv, words, lens, out, table, max_new=x["max_new"])
    torch.cuda.synchronize()
    if mode == "disjoint":
        assert lens.tolist() == list(x["lens"]), "seqlens_k was written"
    assert np.array_equal(words.cpu().numpy().view(np.uint64), x["words"]), "the words were written"
    return _np_bits(torch, dk), _np_bits(torch, dvv), out.cpu().numpy()


# ---- 1. the bytes of the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,fmt,d", FORM_FMT_D)
def test_bytes_of_the_model(fa, torch_cuda, paged, fp8, fmt, d):
    """the whole cache or pool, K and V, guard pages included, and seqlens_out: both batches, lengths in place, disjoint and absent, and on
    pages the table with garbage in every entry the rule does not read"""
    torch = torch_cuda
    moved = 0
    for name, table, mode in cmi.gpu_cases(paged):
        x = cmi.inputs(name, d, paged, fp8, table, mode)
        want = cmi.expected(name, d, paged, fp8, table, mode)
        got = _commit(fa, torch, x, fp8, fmt, mode)
        for g, w, n in zip(got, want, ("K", "V", "seqlens_out")):
            assert g.shape == w.shape
            assert np.array_equal(g, w), f"{name} table={table} lengths={mode}: {n} differs from the model in {int((g != w).sum())} places"
        moved += int((want[0] != x["k0"]).any(-1).sum())
    assert moved >= 8 * cmi.HKV, "the runs move rows"


# ---- 2. prefix words ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fp8,fmt,d", FORM_FMT_D)
def test_prefix_words_touch_nothing(fa, torch_cuda, paged, fp8, fmt, d):
    """words that are low-bit prefixes once restricted -- to max_new, to the capacity -- leave every byte as it was and read no table
    entry: every entry holds -1.  The call is the length update alone."""
    torch = torch_cuda
    x = cmi.inputs("wide", d, paged, fp8)
    lens = (20, 40, 13, cmi.NCAP - 3, -9, 64)
    for max_new, words, pop in ((64, (0, 1, 0b111, (1 << 20) - 1, cmi.ALL, cmi.ALL), (0, 1, 3, 3, 64, 64)),
                                (8, (0xFF00, 0x1F | 1 << 9, cmi.ALL, 0b10111, 0b1111 | 1 << 63, 0xFF), (0, 5, 8, 3, 4, 8))):
        y = dict(x, words=np.array(words, np.uint64), lens=lens, max_new=max_new,
                 table=np.full((cmi.B, cmi.MAX_PAGES), -1, np.int32) if paged else None)
        k, v, out = _commit(fa, torch, y, fp8, fmt, "disjoint")
        assert np.array_equal(k, x["k0"]) and np.array_equal(v, x["v0"]), f"max_new={max_new}: a prefix word moved bytes"
        assert out.tolist() == [cm.clamp(L, cmi.NCAP) + p for L, p in zip(lens, pop)]


# ---- 3. end to end: append, tree decode, commit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["fp16_pages16", "fp8_contiguous"])
@pytest.mark.parametrize("d", [64, 128])
def test_step_end_to_end(fa, oracle, torch_cuda, d, fp8):
    """append_varlen(positions = L + depth) of three trees, the tree decode, then the commit of one node's path through tree_accept_mask.
    The live range [0, L_b + a_b) equals, byte for byte, that of a cache into which only the linear root-to-node sequence was appended
    (the path's token of rank j has depth j, so both appends rotate it at L_b + j), and a one-token causal decode over both caches
    returns the same bits."""
    torch = torch_cuda
    fmt, B, Hkv, G, Ncap, ps, max_q = 0, 3, 2, 2, 256, 16, 64
    Hq = Hkv * G
    before, m, kinds = [130, 61, 0], [13, 64, 5], ("random", "random", "star")
    cu = np.cumsum([2] + m)
    T = int(cu[-1]) + 3
    rng = np.random.default_rng(9970 + d)
    parents = np.full(T, -1, np.int32)
    for b in range(B):
        parents[cu[b]:cu[b + 1]] = ti.parents_of(kinds[b], m[b], rng)
    dcu = _ints(torch, cu)
    mask, depth = fa.tree_from_parents(torch.from_numpy(parents).cuda(), dcu)
    pos = depth.clone()
    for b in range(B):
        pos[cu[b]:cu[b + 1]] += before[b]
    dep = depth.cpu().numpy()
    last = [int(np.argmax(dep[cu[b]:cu[b + 1]])) for b in range(B)]
    last[2] = m[2] - 1                                        # the star's last leaf: the path {0, 4}
    accept = fa.tree_accept_mask(mask, dcu, _ints(torch, last))
    assert accept.is_cuda and accept.dtype == torch.int64 and accept.shape == (B,)
    words = accept.cpu().numpy().view(np.uint64)
    paths = [[j for j in range(m[b]) if (int(words[b]) >> j) & 1] for b in range(B)]
    assert all(p[-1] == i and len(p) == dep[cu[b] + i] + 1 for b, (p, i) in enumerate(zip(paths, last)))
    assert any(p != list(range(len(p))) for p in paths), "a path that is no prefix: rows move"
    after = [L + len(p) for L, p in zip(before, paths)]
    (_, k, v), (_, kb, vb) = di.inputs(oracle, B, Hkv, G, 1, Ncap, d, fmt, 9971)
    tokens = torch.from_numpy(rng.uniform(-1, 1, (T, Hq + 2 * Hkv, d)).astype(np.float32)).cuda().to(torch.float16)
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    ks, vs = (_floats(torch, KS), _floats(torch, VS)) if fp8 else (None, None)

    def caches():
        if fp8:
            return (cm.dev8(torch, cm.poisoned(f8.encode(k).reshape(B, Hkv, Ncap, d), before, nan=f8.NAN_CODES[0])),
                    cm.dev8(torch, cm.poisoned(f8.encode(v).reshape(B, Hkv, Ncap, d), before, nan=f8.NAN_CODES[0])), None, None)
        kp, vp, tb = cm.scatter(kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), [L + n for L, n in zip(before, m)], ps, 9972)
        return cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(tb).cuda(), tb

    def append(fused, cu_dev, kc, vc, table, lens_in, lens_out, positions):
        kw = dict(cache_seqlens=lens_in, seqlens_out=lens_out, block_table=table, q=fused[:, :Hq], rotary_cos=cos, rotary_sin=sin,
                  positions=positions)
        if fp8:
            fa.fa_kvcache_append_varlen_fp8(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, cu_dev, k_scale=ks, v_scale=vs, **kw)
        else:
            fa.fa_kvcache_append_varlen(fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], kc, vc, cu_dev, **kw)

    def decode(q, cu_dev, nmax, kc, vc, table, lens, tree_mask=None):
        kw = dict(cache_seqlens=lens, block_table=table, causal=True, return_lse=True, tree_mask=tree_mask)
        if fp8:
            return fa.fa_kvcache_decode_varlen_fp8(q, kc, vc, cu_dev, nmax, k_scale=ks, v_scale=vs, **kw)
        return fa.fa_kvcache_decode_varlen(q, kc, vc, cu_dev, nmax, **kw)

    # the tree step: three launches
    kc, vc, table, tb = caches()
    lens, lens_step = _ints(torch, before), torch.zeros(B, dtype=torch.int32, device="cuda")
    fused = tokens.clone()
    append(fused, dcu, kc, vc, table, lens, lens_step, pos)
    o, _ = decode(fused[:, :Hq], dcu, max_q, kc, vc, table, lens_step, mask)
    fa.fa_kvcache_commit(kc, vc, accept, lens, lens, table, max_new=max_q)
    torch.cuda.synchronize()
    assert lens_step.tolist() == [L + n for L, n in zip(before, m)] and lens.tolist() == after
    assert torch.isfinite(o[torch.from_numpy(np.arange(cu[0], cu[-1])).cuda()]).all()
    # the linear sequences through the plain append
    rows = torch.tensor([int(cu[b]) + j for b in range(B) for j in paths[b]], device="cuda")
    cu2 = _ints(torch, np.cumsum([0] + [len(p) for p in paths]))
    kc2, vc2, table2, tb2 = caches()
    lens2 = _ints(torch, before)
    append(tokens[rows].clone(), cu2, kc2, vc2, table2, lens2, lens2, None)
    torch.cuda.synchronize()
    assert lens2.tolist() == after and (tb is None or np.array_equal(tb, tb2))

    def live(cache):
        x = _np_bits(torch, cache)
        if tb is None:
            return [x[b, :, :after[b]] for b in range(B)]
        return [np.stack([x[tb[b, p // ps], :, p % ps] for p in range(after[b])], 1) if after[b] else x[:0] for b in range(B)]

    for got, want, n in ((live(kc), live(kc2), "K"), (live(vc), live(vc2), "V")):
        for b in range(B):
            assert np.array_equal(got[b], want[b]), f"{n} of sequence {b}: the committed range differs from the linear append's"
    q1 = torch.from_numpy(rng.uniform(-1, 1, (B, Hq, d)).astype(np.float32)).cuda().to(torch.float16)
    cu1 = _ints(torch, range(B + 1))
    (o1, l1), (o2, l2) = decode(q1, cu1, 1, kc, vc, table, lens), decode(q1, cu1, 1, kc2, vc2, table2, lens2)
    torch.cuda.synchronize()
    assert torch.isfinite(o1).all() and torch.isfinite(l1).all()
    assert torch.equal(_bits32(torch, o1), _bits32(torch, o2)) and torch.equal(_bits32(torch, l1), _bits32(torch, l2))


def _bits32(torch, t):
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32)


# ---- 4. the captured step -------------------------------------------------------------------------------------------------------------------
def test_captured_step(fa, oracle, torch_cuda):
    """append_varlen(positions) -> tree decode behind a split -> tree_accept_mask -> commit with the lengths in place, captured once and
    replayed three times on rewritten trees, tokens and accepted nodes.  Caches and lengths carry over from replay to replay; each
    replay equals the eager step on a second copy of the state bit for bit, and the lengths grow by a_b."""
    torch = torch_cuda
    d, B, Hkv, G, Ncap, ps, max_q, T = 64, 2, 1, 2, 8192, 16, 5, 12
    Hq, max_pages = Hkv * G, Ncap // ps
    num_pages = B * max_pages + 3
    gen = torch.Generator(device="cuda").manual_seed(9980)
    pool = lambda: (torch.rand((num_pages, Hkv, ps, d), device="cuda", generator=gen) * 2 - 1).to(torch.float16)
    cos, sin = (_floats(torch, x) for x in rp.real_table(Ncap, d))
    need = fa.kvcache_decode_varlen_workspace_bytes(B, Hkv, G, max_q, d, max_pages=max_pages, page_size=ps)
    assert need > 0                                       # S > 1: the merge is in the graph
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    start = [8000, 37]
    perm = torch.randperm(num_pages, device="cuda", generator=gen)[:B * max_pages].to(torch.int32).view(B, max_pages)
    # what a replay rewrites in place
    fused = torch.zeros(T, Hq + 2 * Hkv, d, dtype=torch.float16, device="cuda")
    cu, table = _ints(torch, [0, 1, 2]), torch.zeros(B, max_pages, dtype=torch.int32, device="cuda")
    mask, pos = torch.ones(T, dtype=torch.int64, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda")
    last = torch.zeros(B, dtype=torch.int32, device="cuda")

    class State:
        """what a step carries over and what it returns"""
        def __init__(self, kp, vp, lens):
            self.kp, self.vp, self.lens = kp, vp, lens
            self.lens_step = torch.zeros(B, dtype=torch.int32, device="cuda")
            self.accept = torch.zeros(B, dtype=torch.int64, device="cuda")
            self.fz = torch.zeros_like(fused)
            self.out = torch.zeros(T, Hq, d, dtype=torch.float32, device="cuda")
            self.lse = torch.zeros(Hq, T, dtype=torch.float32, device="cuda")

        def tensors(self):
            return self.out, self.lse, self.fz, self.kp, self.vp, self.lens, self.lens_step, self.accept

    def step(s):
        s.fz.copy_(fused)
        fa.fa_kvcache_append_varlen(s.fz[:, Hq:Hq + Hkv], s.fz[:, Hq + Hkv:], s.kp, s.vp, cu, cache_seqlens=s.lens, seqlens_out=s.lens_step,
                                    block_table=table, q=s.fz[:, :Hq], rotary_cos=cos, rotary_sin=sin, positions=pos)
        fa.fa_kvcache_decode_varlen(s.fz[:, :Hq], s.kp, s.vp, cu, max_q, s.lens_step, table, causal=True, out=s.out, lse=s.lse, workspace=ws,
                                    tree_mask=mask)
        s.accept.copy_(fa.tree_accept_mask(mask, cu, last))
        fa.fa_kvcache_commit(s.kp, s.vp, s.accept, s.lens, s.lens, table, max_new=max_q)

    kp0, vp0 = pool(), pool()
    scratch = State(kp0.clone(), vp0.clone(), _ints(torch, [0, 0]))
    step(scratch)                                         # warm-up on scratch state
    torch.cuda.synchronize()
    held = State(kp0.clone(), vp0.clone(), _ints(torch, start))
    eager = State(kp0.clone(), vp0.clone(), _ints(torch, start))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(held)
    table.copy_(perm)
    L = list(start)
    moved = 0
    for s in range(3):
        g = torch.Generator(device="cuda").manual_seed(9990 + s)
        vec = ([0, 5, 9], [0, 3, 8], [2, 2, 7])[s]          # n = (5, 4); (3, 5); (0, 5)
        kind = ("random", "star", "chain")[s]
        par = np.full(T, -1, np.int32)
        rng = np.random.default_rng(9985 + s)
        for b in range(B):
            n = vec[b + 1] - vec[b]
            par[vec[b]:vec[b + 1]] = ti.parents_of(kind, n, rng) if n else []
        m, dep = fa.tree_from_parents(torch.from_numpy(par).cuda(), _ints(torch, vec))
        p = dep.clone()
        for b in range(B):
            p[vec[b]:vec[b + 1]] += L[b]
        # the accepted node: the deepest of the random trees; the star's last leaf and nothing; nothing (no tokens) and the whole chain
        dn = dep.cpu().numpy()
        chosen = [int(np.argmax(dn[vec[b]:vec[b + 1]])) for b in range(B)] if s == 0 else ([2, -1], [-1, 4])[s - 1]
        wordv = [0 if c < 0 else int(m[vec[b] + c]) & cmi.ALL for b, c in enumerate(chosen)]
        a = [bin(w).count("1") for w in wordv]
        moved += sum(w & (w + 1) != 0 for w in wordv)
        tokens = (torch.rand((T, Hq + 2 * Hkv, d), device="cuda", generator=g) * 2 - 1).to(torch.float16)
        for dst, src in ((fused, tokens), (cu, _ints(torch, vec)), (mask, m), (pos, p), (last, _ints(torch, chosen))):
            dst.copy_(src)
        for st in (held, eager):
            st.out.fill_(-7.0), st.lse.fill_(-7.0)
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in held.tensors()]
        ws.fill_(0xFF)
        step(eager)
        torch.cuda.synchronize()
        names = ("O", "lse", "the fused buffer", "K pool", "V pool", "lengths", "the step's lengths", "the accept words")
        for x, y, n in zip(got, eager.tensors(), names):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"step {s}: {n} of the replay differs from the eager call"
        assert held.accept.tolist() == [w - (1 << 64) if w >> 63 else w for w in wordv]
        L = [x + y for x, y in zip(L, a)]
        assert held.lens.tolist() == L, f"step {s}: the lengths grow by a_b"
    assert moved >= 1 and L != start, "the replays moved rows"   # the star's path {0, 2} at the least


# ---- 5. the torch op ------------------------------------------------------------------------------------------------------------------------
def test_op_is_the_front_end(fa, torch_cuda):
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    for paged, fp8, fmt, d, mode in ((False, False, 1, 128, "in_place"), (True, True, 0, 64, "null"), (True, False, 0, 128, "disjoint")):
        x = cmi.inputs("narrow", d, paged, fp8, "good", mode)
        want = cmi.expected("narrow", d, paged, fp8, "good", mode)
        for g, w in zip(_commit(fa, torch, x, fp8, fmt, mode, op=torch.ops.fa_mi355.commit), want):
            assert np.array_equal(g, w), (paged, fp8, mode)
