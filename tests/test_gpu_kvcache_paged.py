"""GPU tier of the paged KV-cache decode entry (fa_forward_kvcache_paged): a pool of pages and a block table read on the device.

Method of tests/test_gpu_kvcache.py: seeded inputs from oracle.make_qkv, expected outputs from the CPU oracle (oracle.forward_cross
on the keys a row sees; zeros for a row that sees none), expected log-sum-exps from float64 numpy on the same 16-bit-rounded
inputs.  The contiguous cache is scattered into a pool through a seeded permutation of pages; the pool has more pages than the
tables use.  Every page no table names, and every row at or past a sequence's length inside a live page, holds NaN bit patterns;
every table entry at or past ceil(L_b / page_size) holds garbage (-1, 2^30); the workspace is filled with NaN bytes.  A finite
result within tolerance shows that no such row, page or entry was used and that no stale partial was merged.

Tolerances: those of tests/test_gpu_kvcache.py -- the project's max-abs bar and relative-L2 bounds for O, 2 * P_EPS absolute for
the log-sum-exp (the kernel sums the weights after rounding them to the 16-bit input format).  Derived from the formats, not from
what the kernel gives.
"""
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _to_dev(torch, bits, fmt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(_tdtype(torch, fmt))


def _cache_to_dev(torch, bits, lens, B, Hkv, fmt):
    """[B*Hkv, Ncap, d] encodings -> device cache [B, Hkv, Ncap, d] with NaN in every row at and past the sequence's length."""
    bits = bits.reshape(B, Hkv, bits.shape[1], bits.shape[2]).copy()
    for b in range(B):
        bits[b, :, max(int(lens[b]), 0):] = cm.NAN16
    return _to_dev(torch, bits, fmt)


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _live_pages(L, ps):
    return (max(int(L), 0) + ps - 1) // ps


def _scatter(kb, vb, lens, B, Hkv, ps, seed, spare=3, shared=0):
    """K and V encodings [B*Hkv, Ncap, d] -> (K pool, V pool [num_pages, Hkv, ps, d] uint16, table [B, max_pages] int32).
    Pages are dealt out by a seeded permutation of a pool with `spare` pages more than B * max_pages.  shared: the first
    `shared` table entries of every sequence are sequence 0's (the caller made those keys equal)."""
    Ncap, d = kb.shape[1], kb.shape[2]
    max_pages = Ncap // ps
    assert max_pages * ps == Ncap
    num_pages = B * max_pages + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    pools = [np.full((num_pages, Hkv, ps, d), cm.NAN16, np.uint16) for _ in range(2)]
    table = np.empty((B, max_pages), np.int32)
    nxt = 0
    for b in range(B):
        L = min(max(int(lens[b]), 0), Ncap)
        for pi in range(max_pages):
            if pi >= _live_pages(L, ps):
                table[b, pi] = cm.GARBAGE[pi % 2]
                continue
            if b > 0 and pi < shared:
                assert pi < _live_pages(lens[0], ps) and (pi + 1) * ps <= min(L, int(lens[0])), "a shared page is full in both"
                table[b, pi] = table[0, pi]
                continue
            page = int(perm[nxt])
            nxt += 1
            table[b, pi] = page
            n = min(ps, L - pi * ps)   # rows of the page below the length; the rest stay NaN
            for pool, src in zip(pools, (kb, vb)):
                pool[page, :, :n] = src[b * Hkv:(b + 1) * Hkv, pi * ps:pi * ps + n]
    return pools[0], pools[1], table


def _expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal):
    """q [B*Hkv*G, Nq, d], k/v [B*Hkv, Ncap, d] fp32 (16-bit-rounded) -> (O [B*Hq, Nq, d] fp32, lse [B*Hq, Nq] float64)."""
    Hq, d = Hkv * G, q.shape[2]
    out = np.zeros(q.shape, np.float32)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    scale = 1.0 / np.sqrt(d)
    for b in range(B):
        qs = slice(b * Hq, (b + 1) * Hq)
        kb, vb = (np.repeat(x[b * Hkv:(b + 1) * Hkv], G, axis=0) for x in (k, v))   # K/V head of every query head
        lim = [int(c) for c in cm.row_limits(int(lens[b]), Nq, Nq, causal)[1]]
        for c in sorted(set(lim)):
            if c == 0:
                continue
            rows = [i for i in range(Nq) if lim[i] == c]
            out[qs, rows] = oracle.forward_cross(np.ascontiguousarray(q[qs][:, rows]), np.ascontiguousarray(kb[:, :c]),
                                                 np.ascontiguousarray(vb[:, :c]), nthreads=8)
            s = np.einsum("hid,hjd->hij", q[qs][:, rows].astype(np.float64), kb[:, :c].astype(np.float64)) * scale
            m = s.max(-1)
            lse[qs, rows] = m + np.log(np.exp(s - m[..., None]).sum(-1))
    return out, lse


@functools.lru_cache(maxsize=None)
def _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed, lens, causal):
    (q, k, v), _ = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed)
    out, lse = _expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def _run(fa, torch, qb, pools, table, lens, B, Hkv, G, Nq, fmt, causal=False, out_same=False):
    """pools: (K, V) [num_pages, Hkv, ps, d] uint16 numpy or device tensors.
    -> (O [B*Hq, Nq, d] fp32 numpy, lse [B*Hq, Nq] fp32 numpy, workspace bytes)"""
    dk, dv = (p if isinstance(p, torch.Tensor) else _to_dev(torch, p, fmt) for p in pools)
    ps, d = dk.shape[2], dk.shape[3]
    dq = _to_dev(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    dt = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
    need = fa.kvcache_paged_workspace_bytes(B, Hkv, G, Nq, dt.shape[1], ps, d)
    assert need == fa.kvcache_workspace_bytes(B, Hkv, G, Nq, dt.shape[1] * ps, d)
    dl = torch.tensor(list(lens), dtype=torch.int32, device="cuda")
    o, lse = fa.fa_forward_kvcache_paged(dq, dk, dv, dt, dl, causal=causal, out_dtype=_tdtype(torch, fmt) if out_same else torch.float32,
                                         return_lse=True, workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o.float().cpu().numpy().reshape(B * Hkv * G, Nq, d), lse.cpu().numpy().reshape(B * Hkv * G, Nq), need


FMT_D = [pytest.param(fmt, d, id=f"{'fp16' if fmt == 0 else 'bf16'}-d{d}") for d in (64, 128) for fmt in (0, 1)]


@pytest.mark.parametrize("ps,max_pages", [(16, 66), (64, 17), (256, 5)], ids=["p16", "p64", "p256"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_oracle_parity(fa, oracle, torch_cuda, fmt, d, ps, max_pages):
    """Split over the keys (S > 1) with lengths 1, 3 pages + 5 and the capacity; both output types.  Pages of 16 keys put four
    pages into every tile; with pages of 256 the 773-key sequence has its split boundaries (192 keys apart) inside pages."""
    B, Hkv, G, Nq, Ncap = 3, 2, 2, 1, ps * max_pages
    lens = (1, 3 * ps + 5, Ncap)
    _, (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1101)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1101, lens, False)
    kp, vp, table = _scatter(kb, vb, lens, B, Hkv, ps, seed=ps + d)
    pools = tuple(_to_dev(torch_cuda, p, fmt) for p in (kp, vp))
    for out_same in (False, True):
        got, lse, need = _run(fa, torch_cuda, qb, pools, table, lens, B, Hkv, G, Nq, fmt, out_same=out_same)
        assert need > 0
        cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"paged parity d={d} fmt={fmt} page={ps} out_same={out_same}")


@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_single_pass(fa, oracle, torch_cuda, fmt, d, ps):
    """S = 1 (no workspace, the kernel writes O and the log-sum-exp itself).  A sequence of one key returns its V row."""
    B, Hkv, G, Nq, Ncap, lens = 3, 2, 1, 1, 192, (1, 64, 190)
    (q, k, v), (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1201)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1201, lens, False)
    kp, vp, table = _scatter(kb, vb, lens, B, Hkv, ps, seed=ps + d + 1)
    for out_same in (False, True):
        got, lse, need = _run(fa, torch_cuda, qb, (kp, vp), table, lens, B, Hkv, G, Nq, fmt, out_same=out_same)
        assert need == 0
        cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"paged single pass d={d} fmt={fmt} page={ps} out_same={out_same}")
        assert np.array_equal(got[:Hkv, 0], v[:Hkv, 0]), "a sequence of one key must return v[0]"


@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_mask_and_degenerate_rows(fa, oracle, torch_cuda, fmt, d, causal, ps):
    """Lengths 0, 2, 66 and the capacity with five query rows in two folded heads.  Under the mask: length 66 puts keys 64-65 in a
    tile only rows 3 and 4 see, length 2 leaves rows 0-2 without a key, length 0 leaves every row (and the whole table row: all
    garbage) without one."""
    B, Hkv, G, Nq, Ncap, lens = 4, 1, 2, 5, 1024, (0, 2, 66, 1024)
    _, (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1301)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1301, lens, causal)
    dead = np.isinf(want_lse).reshape(B, Hkv * G, Nq)
    assert dead[0].all() and (dead[1].all(0).tolist() == [causal] * 3 + [False] * 2) and not dead[2:].any()
    kp, vp, table = _scatter(kb, vb, lens, B, Hkv, ps, seed=ps + d + 2)
    got, lse, need = _run(fa, torch_cuda, qb, (kp, vp), table, lens, B, Hkv, G, Nq, fmt, causal=causal)
    assert need > 0
    cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"paged mask + degenerate rows d={d} fmt={fmt} page={ps} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("ps", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("fmt,d", [pytest.param(0, 64, id="fp16-d64"), pytest.param(1, 128, id="bf16-d128")])
def test_bit_equal_to_contiguous_entry(fa, oracle, torch_cuda, fmt, d, ps, causal):
    """Same splits, same tile order, same arithmetic, other addresses: O and the log-sum-exp equal fa_forward_kvcache's on the
    unscattered cache bit for bit -- behind a split (1280 keys) and in one pass (256 keys)."""
    torch = torch_cuda
    B, Hkv, G, Nq = 3, 2, 2, 3
    for Ncap, lens, split in ((1280, (1, 773, 1280), True), (256, (5, 200, 256), False)):
        _, (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1401)
        dq = _to_dev(torch, qb, fmt).view(B, Hkv * G, Nq, d)
        dk, dv = (_cache_to_dev(torch, x, lens, B, Hkv, fmt) for x in (kb, vb))
        dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
        assert (need > 0) == split
        base, base_lse = fa.fa_forward_kvcache(dq, dk, dv, dl, causal=causal, return_lse=True, workspace=_nan_workspace(torch, need))
        kp, vp, table = _scatter(kb, vb, lens, B, Hkv, ps, seed=ps + d + 3)
        dt = torch.from_numpy(table).cuda()
        got, got_lse = fa.fa_forward_kvcache_paged(dq, _to_dev(torch, kp, fmt), _to_dev(torch, vp, fmt), dt, dl, causal=causal,
                                                   return_lse=True, workspace=_nan_workspace(torch, need))
        torch.cuda.synchronize()
        assert torch.isfinite(base).all() and torch.isfinite(got).all() and not torch.isnan(got_lse).any()
        diff = (got - base).abs().max().item()
        print(f"page={ps} Ncap={Ncap} causal={causal}: max |paged - contiguous| = {diff:.3e}")
        assert torch.equal(got, base) and torch.equal(got_lse, base_lse), (ps, Ncap, causal, diff)


@pytest.mark.parametrize("fmt,d,ps,shared", [pytest.param(0, 64, 16, 5, id="fp16-d64-p16"), pytest.param(1, 128, 64, 3, id="bf16-d128-p64")])
def test_shared_prefix(fa, oracle, torch_cuda, fmt, d, ps, shared):
    """Two sequences whose tables name the SAME physical pages for their first `shared` pages and differ afterwards."""
    B, Hkv, G, Nq, Ncap = 2, 2, 2, 1, 1088
    lens = (shared * ps + 7, Ncap - 9)
    (q, k, v), (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1501)
    k, v, kb, vb = (x.copy() for x in (k, v, kb, vb))
    for x in (k, v, kb, vb):
        x[Hkv:, :shared * ps] = x[:Hkv, :shared * ps]   # sequence 1 starts with sequence 0's prefix
    want, want_lse = _expected(oracle, q, k, v, lens, B, Hkv, G, Nq, False)
    kp, vp, table = _scatter(kb, vb, lens, B, Hkv, ps, seed=ps + d + 4, shared=shared)
    assert (table[0, :shared] == table[1, :shared]).all() and table[0, shared] != table[1, shared]
    got, lse, need = _run(fa, torch_cuda, qb, (kp, vp), table, lens, B, Hkv, G, Nq, fmt)
    assert need > 0
    cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"paged shared prefix d={d} fmt={fmt} page={ps}")


@pytest.mark.parametrize("fmt,d,ps", [pytest.param(0, 64, 16, id="fp16-d64-p16"), pytest.param(0, 64, 64, id="fp16-d64-p64"),
                                      pytest.param(1, 128, 64, id="bf16-d128-p64")])
def test_bad_live_entries_read_zeros(fa, oracle, torch_cuda, fmt, d, ps):
    """Live table slots holding -1, -2, 4 and 5 against a pool of 4 pages: each reads as a page of zero K and V rows.  The pool is
    the contiguous view [2:6] of an allocation of 8 pages whose other 4 pages hold NaN, so every one of those numbers lands inside
    the allocation even with the guard missing: a missing guard shows as NaN, not as a fault."""
    torch = torch_cuda
    B, Hkv, G, Nq, max_pages = 1, 2, 2, 1, 8
    Ncap = max_pages * ps
    L = Ncap - 3
    slots = [0, -1, 1, 4, 2, -2, 5, 3]   # page number of each table slot; the last page (a good one) is live up to row ps - 3
    (q, k, v), (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 1601)
    k, v = k.copy(), v.copy()
    alloc = [np.full((8, Hkv, ps, d), cm.NAN16, np.uint16) for _ in range(2)]
    for pi, page in enumerate(slots):
        n = min(ps, L - pi * ps)
        if 0 <= page < 4:
            for a, src in zip(alloc, (kb, vb)):
                a[2 + page, :, :n] = src[:, pi * ps:pi * ps + n]
        else:
            k[:, pi * ps:(pi + 1) * ps] = 0.0
            v[:, pi * ps:(pi + 1) * ps] = 0.0
    want, want_lse = _expected(oracle, q, k, v, (L,), B, Hkv, G, Nq, False)
    views = tuple(_to_dev(torch, a, fmt)[2:6] for a in alloc)
    assert all(p.is_contiguous() and p.shape[0] == 4 and p.storage_offset() > 0 for p in views)
    got, lse, need = _run(fa, torch, qb, views, np.array([slots], np.int32), (L,), B, Hkv, G, Nq, fmt)
    assert (need > 0) == (ps == 64)
    cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"paged bad live entries d={d} fmt={fmt} page={ps}")


def test_graph_replay_follows_table_and_lengths(fa, torch_cuda):
    """One captured call; the table and the lengths are overwritten in place between replays, with another permutation of the pages.
    Nothing on the host read either at capture time, so every replay equals the eager call bit for bit."""
    torch = torch_cuda
    B, Hkv, G, Nq, ps, max_pages, d = 2, 2, 1, 1, 16, 44, 64
    Ncap, num_pages = ps * max_pages, 2 * max_pages + 5
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.randn(B, Hkv * G, Nq, d, generator=g, device="cuda").half()
    k0, v0 = (torch.randn(B, Hkv, Ncap, d, generator=g, device="cuda").half() for _ in range(2))
    kp, vp = (torch.empty(num_pages, Hkv, ps, d, dtype=torch.float16, device="cuda") for _ in range(2))
    table = torch.empty(B, max_pages, dtype=torch.int32, device="cuda")
    lens = torch.empty(B, dtype=torch.int32, device="cuda")
    steps = (((704, 5), 1), ((64, 699), 2))

    def place(lengths, seed):
        """pools, table and lengths rewritten IN PLACE: NaN everywhere but the live rows, garbage past the live table entries"""
        perm = np.random.default_rng(seed).permutation(num_pages)
        kp.fill_(float("nan")), vp.fill_(float("nan"))
        tb = np.empty((B, max_pages), np.int32)
        nxt = 0
        for b, L in enumerate(lengths):
            for pi in range(max_pages):
                if pi >= _live_pages(L, ps):
                    tb[b, pi] = cm.GARBAGE[pi % 2]
                    continue
                page, n = int(perm[nxt]), min(ps, L - pi * ps)
                nxt += 1
                tb[b, pi] = page
                kp[page, :, :n] = k0[b, :, pi * ps:pi * ps + n]
                vp[page, :, :n] = v0[b, :, pi * ps:pi * ps + n]
        table.copy_(torch.from_numpy(tb).cuda())
        lens.copy_(torch.tensor(lengths, dtype=torch.int32, device="cuda"))

    need = fa.kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, ps, d)
    assert need > 0
    ws = _nan_workspace(torch, need)
    eager = []
    for lengths, seed in steps:
        place(lengths, seed)
        ws.fill_(0xFF)
        o, lse = fa.fa_forward_kvcache_paged(q, kp, vp, table, lens, return_lse=True, workspace=ws)
        eager.append((o.clone(), lse.clone()))
    place((300, 300), 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = fa.fa_forward_kvcache_paged(q, kp, vp, table, lens, return_lse=True, workspace=ws)
    for (lengths, seed), (eo, el) in zip(steps, eager):
        place(lengths, seed)
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), lengths
        assert torch.equal(o, eo) and torch.equal(lse, el), lengths
