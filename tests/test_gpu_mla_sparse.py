"""GPU tier of fa_mla_decode_sparse (fa.fa_mla_decode_sparse, torch.ops.fa_mi355.mla_decode_sparse): MLA decode over per-token key
index lists.

Inputs, layouts, packing, the page scatter and the check are tests/mla_inputs.py's, common_inputs' and decode_varlen_inputs' (Hq = 80
is the first 80 heads of the h128 family).  The float64 reference is mla_inputs.expected_f64 with cb[:lim] replaced by
cb[visible entries]: the softmax runs over the ENTRIES, so a key listed twice counts twice.  Bounds are the project's: cm.MAX_ABS and
cm.REL_L2 on O, 2 * cm.P_EPS on lse, exact 0 / -inf for a token without a visible entry -- the arithmetic is the dense kernel's.

Lists: a seeded, unsorted sample of [0, L_b) without repetition, padded with -1 where topk > L_b, then overwritten at fixed positions
with -1, L_b, INT_MAX, c_i (the first key the causal mask hides from the row) and one repeated key.
Poison: NaN in every cache row that no visible entry of its sequence names (paged: in every pool row besides), in Q rows of no
sequence and in the workspace; sentinels in O and lse; a plausible key (5) in the index rows of tokens of no sequence.  A wrong gather,
an address made from a masked entry or a write to a dead token shows as NaN or as a moved sentinel.
"""
import numpy as np
import pytest

import common_inputs as cm
import decode_varlen_inputs as dv
import mla_inputs as mi

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _lists(f, lay, topk, causal, special, seed):
    """-> int32 [total_q, topk]; special: None, "tile" (entries 0..31 of every list masked) or "token" (the first live token's whole
    list masked)"""
    rng = np.random.default_rng(seed)
    idx = np.full((lay.total_q, topk), 5, np.int32)
    first = True
    for b in range(f["B"]):
        L = cm.clamp(f["lens"][b], f["Ncap"])
        lim = cm.row_limits(L, lay.n[b], f["max_q"], causal)[1]
        for i in range(lay.n[b]):
            row = np.full(topk, -1, np.int64)
            row[:min(topk, L)] = rng.permutation(L)[:topk]
            if topk >= 6:
                row[0], row[1], row[2], row[3], row[4] = -1, L, INT_MAX, lim[i], row[5]
            if special == "tile":
                row[:32] = (-1, L, INT_MAX, -7) * 8
            if special == "token" and first:
                row[:] = np.where(np.arange(topk) % 2, INT_MAX, -1)
            first = False
            idx[lay.tok[b, i]] = row
    return idx


def _expected(q, c, idx, f, lay, Hq, causal):
    """mi.expected_f64 over the visible entries -> (O, lse) padded, and per sequence the set of keys some visible entry names"""
    B, Nq = f["B"], f["max_q"]
    out, lse, named = np.zeros((B * Hq, Nq, mi.DC)), np.full((B * Hq, Nq), -np.inf), []
    for b in range(B):
        lim = cm.row_limits(cm.clamp(f["lens"][b], f["Ncap"]), lay.n[b], Nq, causal)[1]
        cb, keys = c[b].astype(np.float64), set()
        for i in range(lay.n[b]):
            j = idx[lay.tok[b, i]].astype(np.int64)
            vis = j[(j >= 0) & (j < lim[i])]
            keys.update(vis.tolist())
            if len(vis):
                s = (cb[vis] @ q[b * Hq:(b + 1) * Hq, i].astype(np.float64).T) * mi.SCALE   # [entries, Hq]
                m = s.max(axis=0)
                p = np.exp(s - m)
                out[b * Hq:(b + 1) * Hq, i] = (p / p.sum(axis=0)).T @ cb[vis, :mi.DC]
                lse[b * Hq:(b + 1) * Hq, i] = m + np.log(p.sum(axis=0))
        named.append(np.array(sorted(keys), np.int64))
    return out, lse, named


class Case:
    """One state of one case on the host: the packed Q bits, the poisoned cache (or pool and table), the lists and the reference"""

    def __init__(self, oracle, name, Hq, topk, fmt, causal, ps, special=None, lens=None, seed=1, zero_page=None):
        self.f = f = dict(mi.family(name), **({} if lens is None else dict(lens=lens)))
        self.lay, self.Hq, self.topk, self.fmt, self.causal = mi.layout(name), Hq, topk, fmt, causal
        B, Nq = f["B"], f["max_q"]
        (q, c), (qb, cb) = mi.inputs(oracle, name, fmt)
        q, qb = (x.reshape(B, f["Hq"], Nq, mi.DQK)[:, :Hq].reshape(B * Hq, Nq, mi.DQK) for x in (q, qb))
        self.idx = _lists(f, self.lay, topk, causal, special, seed)
        if zero_page is not None:   # (b, page): the reference of a live table entry outside the pool
            c = c.copy()
            c[zero_page[0], zero_page[1] * ps:(zero_page[1] + 1) * ps] = 0.0
        self.want, self.want_lse, self.named = _expected(q, c, self.idx, f, self.lay, Hq, causal)
        self.q = dv.pack_rows(self.lay, qb, np.uint16(cm.NAN16))
        cache = np.full_like(cb, cm.NAN16)
        for b in range(B):
            cache[b, self.named[b]] = cb[b, self.named[b]]
        self.table = None
        if ps:
            pool, _, self.table = cm.scatter(cache[:, None], cache[:, None], f["lens"], ps, seed + 4)
            cache = np.ascontiguousarray(pool[:, 0])
        self.cache = cache

    def device(self, torch):
        ints = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
        return dict(q=cm.dev16(torch, self.q, self.fmt), c_cache=cm.dev16(torch, self.cache, self.fmt), indices=ints(self.idx),
                    cu_seqlens_q=ints(self.lay.cu), cache_seqlens=ints(self.f["lens"]), block_table=ints(self.table))

    def check(self, oracle, o, lse, what):
        dv.check(oracle, self.lay, o.float().cpu().numpy(), lse.cpu().numpy(), self.want, self.want_lse, self.fmt, what)


def _run(fa, torch, case, dev, S, out_dtype=None, table=None):
    """one call with sentinels in O and lse and NaN bytes in the workspace -> (O, lse)"""
    out_dtype = out_dtype or torch.float32
    T, Hq = case.lay.total_q, case.Hq
    if out_dtype == torch.float32:
        out = torch.full((T, Hq, mi.DC), dv.SENTINEL_O32, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        out = torch.full((T, Hq, mi.DC), dv.SENTINEL_O16, dtype=torch.int16, device="cuda").view(out_dtype)
    lse = torch.full((Hq, T), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    need = fa.mla_decode_sparse_workspace_bytes(case.f["B"], Hq, case.f["max_q"], case.topk, Ncap=case.f["Ncap"], num_splits=S)
    assert (need == 0) == (S == 1) or S == 0
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    kw = dict(dev, block_table=dev["block_table"] if table is None else table)
    o, l = fa.fa_mla_decode_sparse(max_seqlen_q=case.f["max_q"], causal=case.causal, num_splits=S, out=out, lse=lse, workspace=ws, **kw)
    torch.cuda.synchronize()
    return o, l


# family (Hq = the first heads of it), Hq, topk, num_splits, page size, fmt, causal, 16-bit output too, special list
CASES = [
    ("h5", 5, 200, 3, 0, 0, True, False, None),        # an idle slot, a sequence owning more tokens than max_q, n_b = 4, L = 3 < topk
    ("h5", 5, 33, 1, 16, 1, True, False, "tile"),      # one entry past a tile whose 32 entries are all masked: m_ref stays -inf
    ("h5", 5, 1, 0, 0, 1, False, False, None),         # one entry
    ("h16", 16, 64, 1, 16, 0, True, False, "token"),   # n_b = 2 under the causal mask; a token whose whole list is masked
    ("h128", 80, 200, 0, 16, 0, True, True, None),     # a partly live second head block; topk > L_b = 77
    ("h128", 128, 200, 3, 16, 1, False, False, None),  # two full head blocks, three splits
    ("h128", 128, 64, 1, 0, 0, True, False, None),
    ("h128", 80, 33, 1, 0, 1, False, True, None),
]


@pytest.mark.parametrize("name,Hq,topk,S,ps,fmt,causal,out16,special", CASES,
                         ids=[f"{c[0]}-Hq{c[1]}-k{c[2]}-S{c[3]}-p{c[4]}-{cm.FMT_NAME[c[5]]}{'-causal' if c[6] else ''}" for c in CASES])
def test_float64_reference(fa, oracle, torch_cuda, name, Hq, topk, S, ps, fmt, causal, out16, special):
    torch = torch_cuda
    case = Case(oracle, name, Hq, topk, fmt, causal, ps, special)
    dev = case.device(torch)
    if special == "token":
        assert not np.isfinite(case.want_lse[:Hq, 0]).any()
    o, lse = _run(fa, torch, case, dev, S)
    case.check(oracle, o, lse, f"sparse {name} Hq={Hq} topk={topk} S={S} page={ps}")
    if out16:   # the same call's fp32 result rounded once; tokens of no sequence keep the 16-bit sentinel
        o16, lse16 = _run(fa, torch, case, dev, S, out_dtype=dev["q"].dtype)
        owned = torch.from_numpy(case.lay.owned).cuda()
        assert torch.equal(o16[owned].view(torch.int16), o[owned].to(o16.dtype).view(torch.int16)) and torch.equal(lse16, lse)
        assert (o16[~owned].view(torch.int16) == dv.SENTINEL_O16).all()


@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_paged_returns_the_contiguous_bits(fa, oracle, torch_cuda, fmt):
    torch = torch_cuda
    res = []
    for ps in (0, 16):
        case = Case(oracle, "h5", 5, 200, fmt, True, ps)
        res.append(_run(fa, torch, case, case.device(torch), 3))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("ps", [0, 16], ids=["contiguous", "page16"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_the_full_list_returns_the_dense_bits(fa, oracle, torch_cuda, fmt, ps):
    """indices[t] = 0 .. L - 1 with L = 130, Hq = 5, no causal mask, one split and one token per sequence: tile contents, order and
    arithmetic are fa_mla_decode's, so the bits are.  One token per sequence, because the dense kernel folds a sequence's tokens into
    one wave and its lazy maximum moves on a wave-wide vote: with two tokens in a wave the other token's keys can move it."""
    torch = torch_cuda
    L, B, Hq = 130, 4, 5
    _, (qb, cb) = mi.inputs(oracle, "h5", fmt)
    q = cm.dev16(torch, np.ascontiguousarray(qb.reshape(B, Hq, -1, mi.DQK)[:, :, 0]), fmt)   # (B tokens, Hq, 576)
    cache, table = cm.poisoned(cb[:, None], [L] * B)[:, 0], None
    if ps:
        pool, _, tb = cm.scatter(cb[:, None], cb[:, None], [L] * B, ps, 9)
        cache, table = np.ascontiguousarray(pool[:, 0]), torch.from_numpy(tb).cuda()
    cache = cm.dev16(torch, cache, fmt)
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    idx = torch.arange(L, dtype=torch.int32, device="cuda").repeat(B, 1)
    kw = dict(cache_seqlens=lens, block_table=table, causal=False, num_splits=1, return_lse=True)
    o, lse = fa.fa_mla_decode_sparse(q, cache, idx, cu, 1, **kw)
    o_d, lse_d = fa.fa_mla_decode(q, cache, cu, 1, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all() and torch.equal(o.view(torch.int32), o_d.view(torch.int32)) and torch.equal(lse, lse_d)


def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda):
    """the table entry of a page some visible entry maps to is set to num_pages: its keys are rows of zeros with logit 0"""
    torch = torch_cuda
    b, ps = 1, 16
    page = Case(oracle, "h16", 16, 64, 0, True, ps).named[b][0] // ps
    case = Case(oracle, "h16", 16, 64, 0, True, ps, zero_page=(b, page))
    dev = case.device(torch)
    dev["block_table"][b, page] = case.cache.shape[0]
    o, lse = _run(fa, torch, case, dev, 1)
    case.check(oracle, o, lse, "sparse bad live page")


def test_a_captured_call_follows_its_vectors(fa, oracle, torch_cuda):
    """one call captured in a graph; the lists, the lengths, the block table and the pool are rewritten in place before each replay,
    and each replay is held against the reference of its own state"""
    torch = torch_cuda
    name, Hq, topk, S, ps = "h16", 16, 200, 2, 16
    states = [Case(oracle, name, Hq, topk, 0, True, ps, lens=lens, seed=seed) for lens, seed in (((600, 300, 65), 1), ((90, 512, 7), 2),
                                                                                                  ((333, 40, 200), 3))]
    dev = states[0].device(torch)
    T = states[0].lay.total_q
    out, lse = torch.zeros((T, Hq, mi.DC), dtype=torch.float32, device="cuda"), torch.zeros((Hq, T), dtype=torch.float32, device="cuda")
    ws = torch.full((fa.mla_decode_sparse_workspace_bytes(3, Hq, 2, topk, Ncap=512, num_splits=S),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0

    def step():
        fa.fa_mla_decode_sparse(max_seqlen_q=2, causal=True, num_splits=S, out=out, lse=lse, workspace=ws, **dev)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for n, case in reversed(list(enumerate(states))):
        for key, src in case.device(torch).items():
            dev[key].copy_(src)
        ws.fill_(0xFF)
        out.view(torch.int32).fill_(dv.SENTINEL_O32), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        case.check(oracle, out, lse, f"sparse replay of state {n}")


def test_torch_op(fa, oracle, torch_cuda):
    """torch.ops.fa_mi355.mla_decode_sparse is the front end's call: the same bits, and fresh outputs in the tokens of no sequence"""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    case = Case(oracle, "h16", 16, 64, 0, True, 16)
    dev = case.device(torch)
    o, lse = _run(fa, torch, case, dev, 1)
    o2, lse2 = torch.ops.fa_mi355.mla_decode_sparse(dev["q"], dev["c_cache"], dev["indices"], dev["cu_seqlens_q"], 2, dev["cache_seqlens"],
                                                    dev["block_table"], mi.SCALE, True, 1, True)
    torch.cuda.synchronize()
    owned = torch.from_numpy(case.lay.owned).cuda()
    assert torch.equal(o2[owned], o[owned]) and torch.equal(lse2[:, owned], lse[:, owned])
    assert (o2[~owned] == 0).all() and (lse2[:, ~owned] == -float("inf")).all()
