"""GPU tier of the in-launch running-max pass (fa_fwd_rp16_kernel.hpp, kInLaunch): algo 24 at d = 64 is ONE kernel per call.  A
workgroup collects the row blocks its fast passes refuse in a list of kTailCap entries in LDS and computes their two half-blocks
on half-width waves when its items are done -- or at once when the list is full, after which it goes on with its items.

  flush      more refused blocks per workgroup than the list holds: the list is emptied in between and the workgroup comes back
  edges      a half-block missing / partial / whole at the end of the sequence, next to blocks a fast pass keeps in the SAME
             workgroup, plain and under the mask, fp32 and 16-bit output, whatever the output buffer held
  graph      captured on benign data, replayed on hostile data
  streams    two forwards with refused blocks at the same time

Inputs, references and tolerances are those of tests/test_gpu_fallback_paths.py (fallback_inputs.py; the CPU oracle with float64
accumulators on the 16-bit-rounded inputs; fp16: max-abs 1e-2, rel-L2 2e-3, x 1.5 with 16-bit output).  Two calls of our kernels
are compared bit for bit."""
import functools
import os
import re

import numpy as np
import pytest

import fallback_inputs as fi
import test_gpu_fallback_paths as fb

pytestmark = pytest.mark.gpu

F16 = 0
D = 64
ROWS = fi.ROWS_PER_BLOCK[D]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def tail_cap():
    """rp16::kTailCap, from the one place that defines it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "flashattention_kernel_project_amd", "csrc", "fa_fwd_rp16_kernel.hpp")).read()
    (cap,) = re.findall(r"constexpr int kTailCap = (\d+);", src)
    return int(cap)


def owners(nwg, nqb, grid):
    """A copy of locate() in flashattention_kernel_project_amd/csrc/fa_fwd_rp16_body.inc (which points back here): if the remap
    changes there, change it here, or the "mixed workgroups" assertion below checks another map than the kernel's.
    item -> (workgroup, head): item `bid` of the persistent grid belongs to workgroup bid % grid and,
    through the XCD-aware remap, is row block wgid % nqb (in one direction or the other) of head wgid // nqb"""
    xq, xr = nwg >> 3, nwg & 7
    out = []
    for bid in range(nwg):
        xcd = bid & 7
        wgid = (xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3)
        out.append((bid % grid, wgid // nqb))
    return out


# ---- flush ---------------------------------------------------------------------------------------------------------------------
def test_list_flush(fa, oracle, torch_cuda):
    """(kTailCap + 1) x CUs + 3 heads of one row block each, Q and K spread x 3: every block is refused (asserted: id 3 for at
    least 99 % of them; every block holds rows more than 20 log2 units above their tile-0 maximum, measured with
    fallback_inputs.lifts on the sampled heads and with the same float64 arithmetic on the GPU for all of them), so every workgroup
    fills its list, empties it, comes back for its last one or two items and empties it again.  Eight heads against the oracle,
    two calls bit for bit, the experimental library's output bit for bit."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = tail_cap()
    bh, n = (cap + 1) * cus + 3, ROWS
    g = torch.Generator().manual_seed(4242)
    q = (torch.randn(bh, n, D, generator=g) * 3.0).half()
    k = (torch.randn(bh, n, D, generator=g) * 3.0).half()
    v = torch.randn(bh, n, D, generator=g).half()
    dev = tuple(x.cuda() for x in (q, k, v))
    assert -(-bh // cus) > cap, "more items per workgroup than the list holds"
    # lifts: float64 on the GPU for every head ...
    s = torch.empty(0)
    lift_all = torch.empty(bh, n, dtype=torch.float64, device="cuda")
    for b0 in range(0, bh, 256):
        s = (dev[0][b0:b0 + 256].double() @ dev[1][b0:b0 + 256].double().transpose(1, 2)) * (fi.LOG2E / np.sqrt(D))
        lift_all[b0:b0 + 256] = s.amax(-1) - s[:, :, :64].amax(-1)
    del s
    per_block = lift_all.amax(-1).cpu().numpy()
    print(f"flush: bh={bh} cap={cap} cus={cus}; smallest per-block maximum lift {per_block.min():.1f}")
    assert (per_block > 20.0).all(), per_block.min()
    # ... which is fallback_inputs.lifts on the sampled heads
    sample = [0, 1, cus - 1, cus, cap * cus - 1, cap * cus, bh - 2, bh - 1]
    qn, kn, vn = (x.float().numpy() for x in (q, k, v))
    for b in sample:
        want_l = fi.lifts(qn, kn, b, False)
        np.testing.assert_allclose(lift_all[b].cpu().numpy(), want_l, atol=1e-9)
        assert want_l.max() > 20.0 and any(fi.fails(x, F16) for x in want_l)
    ids, o_exp = fb._pass_ids(torch, dev, 24, ROWS, False)
    frac = float((ids == 3).mean())
    print(f"flush: blocks with pass id 3: {frac:.4f}")
    assert frac >= 0.99, frac
    a = fb._forward(fa, torch, dev, F16, 24, False, False)
    b2 = fb._forward(fa, torch, dev, F16, 24, False, False)
    assert torch.equal(fb._raw(torch, a), fb._raw(torch, b2)), "not reproducible"
    assert torch.equal(fb._raw(torch, a), fb._raw(torch, o_exp)), "product and experimental library differ"
    assert bool(torch.isfinite(a).all())
    idx = np.array(sample)
    want = oracle.forward(qn[idx], kn[idx], vn[idx], accum=1, nthreads=8)
    fb._check(oracle, a[torch.from_numpy(idx).cuda()].cpu().numpy(), want, F16, "flush, sampled heads", np.abs(vn[idx]).max())


# ---- half-block edges ----------------------------------------------------------------------------------------------------------
TILE = 128   # copies of the three-head case: 384 heads x 2 row blocks = 768 items, three per workgroup on 256 CUs


@functools.lru_cache(maxsize=None)
def _plain_edges(oracle, n):
    """Three heads without a mask: head 0 benign N(0, 1); heads 1 and 2 with every key behind tile 0 x 6 (head 2 of
    fallback_inputs.plain_case: beyond fp16's overflow point in every row block)."""
    (q, k, v), _ = oracle.make_qkv(3, n, D, F16, seed=3100 + n)
    k = k.copy()
    k[1:, 64:] *= 6.0
    (q, k, v), bits = fi._round(oracle, F16, q, k, v)
    want = oracle.forward(q, k, v, accum=1, nthreads=8)
    want.setflags(write=False)
    return dict(q=q, k=k, v=v, bits=bits, rows=ROWS, causal=False), want


def _assert_plain_edges(case):
    q, k = case["q"], case["k"]
    n = q.shape[1]
    assert fi.lifts(q, k, 0, False, width=32).max() <= 19.5, "head 0 can stay in a fast pass"
    for b in (1, 2):
        lb = fi.lifts(q, k, b, False)
        for blk in range((n + ROWS - 1) // ROWS):
            assert any(fi.fails(x, F16) for x in lb[blk * ROWS:(blk + 1) * ROWS]), (b, blk)


EDGES = [pytest.param(n, causal, out_same, id=f"n{n}-{'causal' if causal else 'plain'}-{'out16' if out_same else 'out32'}")
         for n in fi.CHAIN_N[D] for causal in (False, True) for out_same in (False, True)]


@pytest.mark.parametrize("n,causal,out_same", EDGES)
def test_half_block_edges(fa, oracle, torch_cuda, n, causal, out_same):
    """The second half of row block 1 lies behind the sequence (n = 600: skipped), partly inside it (800) or inside it (1024).
    The three-head case 128 times over: every workgroup owns three items, and workgroups own blocks a fast pass keeps (head 0)
    next to refused ones (asserted from the pass ids and the kernel's item map).  The output buffer holds NaNs in one call and the
    former marker word in the other: same bits, finite, and the oracle's values."""
    torch = torch_cuda
    if causal:
        case, want = fi.chain_case(oracle, D, n, F16), fb._chain_ref(oracle, D, n, F16)
        fi.assert_chain_case(case, F16)
    else:
        case, want = _plain_edges(oracle, n)
        _assert_plain_edges(case)
    dev = tuple(fb._to_dev(torch, x, F16).repeat(TILE, 1, 1) for x in case["bits"])
    bh, nqb = 3 * TILE, (n + ROWS - 1) // ROWS
    ids, _ = fb._pass_ids(torch, dev, 24, ROWS, causal, out_same)
    benign = (np.arange(bh) % 3 == 0)
    assert (ids[benign] <= 1).all() and (ids[~benign] == 3).all(), ids[:3].tolist()
    grid = min(bh * nqb, torch.cuda.get_device_properties(0).multi_processor_count)
    own = {}
    for wg, head in owners(bh * nqb, nqb, grid):
        own.setdefault(wg, set()).add(bool(benign[head]))
    mixed = sum(1 for kinds in own.values() if len(kinds) == 2)
    print(f"edges n={n} causal={causal} out_same={out_same}: {mixed} of {len(own)} workgroups own kept and refused blocks")
    assert mixed > 0
    odt = torch.float16 if out_same else torch.float32
    nan_buf = torch.full(dev[0].shape, float("nan"), dtype=odt, device="cuda")
    mark_buf = torch.empty(dev[0].shape, dtype=odt, device="cuda")
    mark_buf.view(torch.int32).fill_(fb.MARKER)
    a = fb._forward(fa, torch, dev, F16, 24, out_same, causal, out=nan_buf)
    b = fb._forward(fa, torch, dev, F16, 24, out_same, causal, out=mark_buf)
    assert a.data_ptr() == nan_buf.data_ptr() and b.data_ptr() == mark_buf.data_ptr()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(fb._raw(torch, a), fb._raw(torch, b)), "the result depends on what the output buffer held"
    got = a.float().cpu().numpy()
    assert np.array_equal(got, np.tile(got[:3], (TILE, 1, 1))), "copies of a head differ"
    fb._check(oracle, got[:3], want, F16, f"edges n={n} causal={causal}", np.abs(case["v"]).max(), out_same, peaked=causal)


# ---- graph ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_on_hostile_data(fa, oracle, torch_cuda):
    """One call captured on benign data (no block refused, asserted); Q and K rewritten in place with the x 6 heads of the edges
    case (blocks refused, asserted); the replay computes the hostile data's result: what the in-launch pass does is decided on
    the device from the data, nothing of it by the host at capture time."""
    torch = torch_cuda
    n = 800
    case, want = _plain_edges(oracle, n)
    _assert_plain_edges(case)
    hostile = tuple(fb._to_dev(torch, x, F16).repeat(TILE, 1, 1) for x in case["bits"])
    (bq, bk, _), bbits = oracle.make_qkv(3, n, D, F16, seed=3100 + n)   # the same heads before the x 6
    q, k, v = (fb._to_dev(torch, x, F16).repeat(TILE, 1, 1) for x in (bbits[0], bbits[1], case["bits"][2]))
    ids, _ = fb._pass_ids(torch, (q, k, v), 24, ROWS, False)
    assert (ids <= 1).all(), "the captured call refuses nothing"
    ids, _ = fb._pass_ids(torch, hostile, 24, ROWS, False)
    assert (ids[1::3] == 3).all() and (ids[2::3] == 3).all()
    o = torch.empty(q.shape, dtype=torch.float32, device="cuda")
    fa.fa_forward(q, k, v, algo=24, out=o)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.fa_forward(q, k, v, algo=24, out=o)
    q.copy_(hostile[0])
    k.copy_(hostile[1])
    o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    eager = fb._forward(fa, torch, hostile, F16, 24, False, False)
    assert torch.equal(fb._raw(torch, o), fb._raw(torch, eager)), "replay and eager call differ"
    fb._check(oracle, o[:3].cpu().numpy(), want, F16, "graph replay on hostile data", np.abs(case["v"]).max(), peaked=False)


# ---- two streams ---------------------------------------------------------------------------------------------------------------
def test_two_streams(fa, oracle, torch_cuda):
    """Two forwards with refused blocks enqueued on two streams, into separate outputs, three rounds: each gives the bits of
    its serial call and the oracle's values (the list and everything else of the in-launch pass is per workgroup, in LDS)."""
    torch = torch_cuda
    cases = [_plain_edges(oracle, 800), _plain_edges(oracle, 1024)]
    devs = [tuple(fb._to_dev(torch, x, F16).repeat(TILE, 1, 1) for x in c["bits"]) for c, _ in cases]
    serial = [fb._forward(fa, torch, dv, F16, 24, False, False).clone() for dv in devs]
    outs = [torch.empty_like(s) for s in serial]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for o in outs:
            o.fill_(float("nan"))
        torch.cuda.synchronize()
        for st, dv, o in zip(streams, devs, outs):
            with torch.cuda.stream(st):
                fa.fa_forward(*dv, algo=24, out=o)
        torch.cuda.synchronize()
        for i, (o, s) in enumerate(zip(outs, serial)):
            assert torch.equal(fb._raw(torch, o), fb._raw(torch, s)), f"stream {i} differs from its serial call"
    for (c, want), o in zip(cases, outs):
        fb._check(oracle, o[:3].cpu().numpy(), want, F16, f"two streams n={c['q'].shape[1]}", np.abs(c["v"]).max(), peaked=False)
