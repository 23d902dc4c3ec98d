"""GPU tier of the KV-cache decode entry (fa_forward_kvcache): per-sequence key counts read on the device, the causal
mask aligned to the end of the cache, rows and splits without a key, the log-sum-exp output, graph replay.

Expected outputs come from the CPU oracle (oracle.forward_cross on the keys a row sees; zeros for a row that sees none),
expected log-sum-exps from float64 numpy on the same 16-bit-rounded inputs.  In every case the cache rows at and past a
sequence's length hold NaN bit patterns and the workspace is filled with NaN bytes before the call: a finite result within
tolerance shows that no key past the length was used and that no stale partial was merged.

Tolerances: the project's max-abs bar and relative-L2 bounds for O.  For the log-sum-exp 2 * P_EPS absolute: the kernel
sums the weights after rounding them to the 16-bit input format, so l is off by a factor within 1 +- P_EPS and ln l by about
P_EPS; the factor 2 covers the fp32 terms (the logits, exp2, log2).  Derived from the formats, not from what the kernel gives.
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
            out[qs, rows] = oracle.forward_cross(q[qs][:, rows], kb[:, :c], vb[:, :c], nthreads=8)
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


def _run(fa, torch, bits, lens, B, Hkv, G, Nq, fmt, causal=False, out_same=False, pass_lens=True):
    """-> (O [B*Hq, Nq, d] fp32 numpy, lse [B*Hq, Nq] fp32 numpy, workspace bytes)"""
    qb, kb, vb = bits
    Ncap, d = kb.shape[1], kb.shape[2]
    dq = _to_dev(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    dk, dv = (_cache_to_dev(torch, x, lens, B, Hkv, fmt) for x in (kb, vb))
    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    dl = torch.tensor(list(lens), dtype=torch.int32, device="cuda") if pass_lens else None
    o, lse = fa.fa_forward_kvcache(dq, dk, dv, dl, causal=causal, out_dtype=_tdtype(torch, fmt) if out_same else torch.float32,
                                   return_lse=True, workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o.float().cpu().numpy().reshape(B * Hkv * G, Nq, d), lse.cpu().numpy().reshape(B * Hkv * G, Nq), need


FMT_D = [pytest.param(fmt, d, id=f"{'fp16' if fmt == 0 else 'bf16'}-d{d}") for d in (64, 128) for fmt in (0, 1)]


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_single_pass(fa, oracle, torch_cuda, fmt, d):
    """S = 1 (no workspace): lengths 1, one full tile, and the ragged capacity; both output types.  One key returns its V row."""
    B, Hkv, G, Nq, Ncap, lens = 3, 2, 1, 1, 200, (1, 64, 200)
    (q, k, v), bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 101)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 101, lens, False)
    for out_same in (False, True):
        got, lse, need = _run(fa, torch_cuda, bits, lens, B, Hkv, G, Nq, fmt, out_same=out_same)
        assert need == 0
        cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"single pass d={d} fmt={fmt} out_same={out_same}")
        assert np.array_equal(got[:Hkv, 0], v[:Hkv, 0]), "a sequence of one key must return v[0]"


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_split_with_empty_splits_gqa(fa, oracle, torch_cuda, fmt, d):
    """A full cache beside one filled to 77 keys (two tiles: every later split is empty), four query heads per K/V head."""
    B, Hkv, G, Nq, Ncap, lens = 2, 2, 4, 1, 8229, (8229, 77)
    _, bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 201)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 201, lens, False)
    got, lse, need = _run(fa, torch_cuda, bits, lens, B, Hkv, G, Nq, fmt)
    assert need > 0
    cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"split + empty splits d={d} fmt={fmt}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_mask_and_degenerate_rows(fa, oracle, torch_cuda, fmt, d, causal):
    """Lengths 0, 2, 66 and the capacity with five query rows in two folded heads.  Under the mask: length 66 puts keys 64-65 in a
    tile only rows 3 and 4 see, length 2 leaves rows 0-2 without a key, length 0 leaves every row without one."""
    B, Hkv, G, Nq, Ncap, lens = 4, 1, 2, 5, 4096, (0, 2, 66, 4096)
    _, bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 301)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 301, lens, causal)
    dead = np.isinf(want_lse).reshape(B, Hkv * G, Nq)
    assert dead[0].all() and (dead[1].all(0).tolist() == [causal] * 3 + [False] * 2) and not dead[2:].any()
    got, lse, need = _run(fa, torch_cuda, bits, lens, B, Hkv, G, Nq, fmt, causal=causal)
    assert need > 0
    cm.check_decode(oracle, got, lse, want, want_lse, fmt, f"mask + degenerate rows d={d} fmt={fmt} causal={causal}")


def test_mask_across_query_blocks(fa, oracle, torch_cuda):
    """Nq = Ncap = 130 without lengths is causal self-attention over two query blocks: the oracle's causal forward and fa_forward."""
    B, Hkv, G, Nq, Ncap, d, fmt = 1, 2, 1, 130, 130, 64, 0
    (q, k, v), bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 401)
    want = oracle.forward(q, k, v, nthreads=8, causal=True)
    _, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 401, (Ncap,), True)
    got, lse, _ = _run(fa, torch_cuda, bits, (Ncap,), B, Hkv, G, Nq, fmt, causal=True, pass_lens=False)
    cm.check_decode(oracle, got, lse, want, want_lse, fmt, "mask across query blocks")
    dq, dk, dv = (_to_dev(torch_cuda, x, fmt) for x in bits)
    plain = fa.fa_forward(dq, dk, dv, causal=True)
    torch_cuda.cuda.synchronize()
    diff = float(np.abs(got - plain.cpu().numpy()).max())
    print(f"against fa_forward(causal=True): {diff:.3e}")
    assert diff <= 2e-3   # the bound of test_splitkv_equals_plain_forward_on_square_shapes


def test_same_answer_as_splitkv(fa, oracle, torch_cuda):
    """Without a mask and with every length at the capacity (given, or by default) the entry computes what fa_forward_splitkv
    computes: the grouped-query shape of test_splitkv_grouped_query_heads."""
    torch = torch_cuda
    b, hq, hkv, nk, d = 2, 8, 2, 3000, 128
    for nq, seed in ((1, 61), (5, 63)):
        (_, _, _), (qb, _, _) = oracle.make_qkv(b * hq, nq, d, fmt=0, seed=seed)
        (_, _, _), (_, kb, vb) = oracle.make_qkv(b * hkv, nk, d, fmt=0, seed=62)
        dq = _to_dev(torch, qb, 0).view(b, hq, nq, d)
        dk, dv = (_to_dev(torch, x, 0).view(b, hkv, nk, d) for x in (kb, vb))
        base = fa.fa_forward_splitkv(dq, dk, dv)
        need = fa.kvcache_workspace_bytes(b, hkv, hq // hkv, nq, nk, d)
        for lens in (None, torch.full((b,), nk, dtype=torch.int32, device="cuda")):
            got = fa.fa_forward_kvcache(dq, dk, dv, lens, workspace=_nan_workspace(torch, need))
            torch.cuda.synchronize()
            diff = (got - base).abs().max().item()
            print(f"nq={nq} lens={'None' if lens is None else 'Ncap'}: max |kvcache - splitkv| = {diff:.3e}, "
                  f"bit-equal: {torch.equal(got, base)}")
            assert torch.isfinite(got).all() and diff <= 2e-3


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_lse_merges_key_ranges(fa, oracle, torch_cuda, fmt, d):
    """The inputs of test_split_with_empty_splits_gqa with the key axis cut at 4000: two calls on contiguous copies of the ranges,
    merged in numpy through their log-sum-exps, give the result over the whole range.  The 77-key sequence has nothing in the
    second range: lse = -inf there, weight 0 in the merge."""
    B, Hkv, G, Nq, Ncap, lens, a = 2, 2, 4, 1, 8229, (8229, 77), 4000
    _, (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 201)
    want, want_lse = _reference(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 201, lens, False)
    o1, l1, _ = _run(fa, torch_cuda, (qb, kb[:, :a], vb[:, :a]), tuple(min(n, a) for n in lens), B, Hkv, G, Nq, fmt)
    o2, l2, _ = _run(fa, torch_cuda, (qb, kb[:, a:], vb[:, a:]), tuple(max(n - a, 0) for n in lens), B, Hkv, G, Nq, fmt)
    assert np.isfinite(l1).all() and np.isfinite(l2[:Hkv * G]).all() and (l2[Hkv * G:] == -np.inf).all()
    assert (o2[Hkv * G:] == 0.0).all()
    l1, l2 = l1.astype(np.float64), l2.astype(np.float64)
    lse = np.logaddexp(l1, l2)
    merged = o1 * np.exp(l1 - lse)[..., None] + o2 * np.exp(l2 - lse)[..., None]
    ma, le = oracle.max_abs(merged.astype(np.float32), want), float(np.abs(lse - want_lse).max())
    print(f"merged over two key ranges d={d} fmt={fmt}: max_abs={ma:.3e} lse_abs={le:.3e}")
    assert np.isfinite(merged).all()
    assert ma <= cm.MAX_ABS
    assert le <= 2 * cm.P_EPS[fmt]


def test_graph_replay_follows_lengths(fa, torch_cuda):
    """One captured call; the lengths tensor is overwritten in place between replays.  Nothing on the host read it at capture
    time, so every replay equals the eager call with those lengths bit for bit."""
    torch = torch_cuda
    B, Hkv, G, Nq, Ncap, d = 2, 4, 1, 1, 700, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(B, Hkv * G, Nq, d, generator=g, device="cuda").half()
    k, v = (torch.randn(B, Hkv, Ncap, d, generator=g, device="cuda").half() for _ in range(2))
    steps = ((700, 5), (64, 699))
    k0, v0 = k.clone(), v.clone()

    def poison(lengths):
        """the clean cache with NaN in every row at and past each sequence's CURRENT length"""
        k.copy_(k0), v.copy_(v0)
        for b, n in enumerate(lengths):
            k[b, :, n:] = float("nan")
            v[b, :, n:] = float("nan")

    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    ws = _nan_workspace(torch, need)
    eager = []
    for s in steps:
        poison(s)
        ws.fill_(0xFF)
        o, lse = fa.fa_forward_kvcache(q, k, v, torch.tensor(s, dtype=torch.int32, device="cuda"), return_lse=True, workspace=ws)
        eager.append((o.clone(), lse.clone()))
    lens = torch.tensor((300, 300), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = fa.fa_forward_kvcache(q, k, v, lens, return_lse=True, workspace=ws)
    for s, (eo, el) in zip(steps, eager):
        poison(s)
        lens.copy_(torch.tensor(s, dtype=torch.int32, device="cuda"))
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), s
        assert torch.equal(o, eo) and torch.equal(lse, el), s
