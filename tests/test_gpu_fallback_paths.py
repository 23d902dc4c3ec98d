"""GPU tier of the data-dependent fallback paths on HOSTILE inputs, where the rest of the suite only has benign ones:

A. the softmax chain of the rolling-pipeline kernels (folded fast pass -> exact optimistic pass -> running-max pass, which the
   full-width families leave to a REDO kernel through a marker word in the output) under the causal mask, with 16-bit output,
   and at ragged N around the redo kernel's half-block edges; the tiled and generic kernels under the mask on the same inputs;
B. the lazy running maximum and the 2^(m_s - M) merge of the split-KV and KV-cache kernels.

Inputs come from tests/fallback_inputs.py (seeded; tests/test_fallback_inputs.py shows without a GPU that each forces what it is
named for, and every test here repeats that assertion before it trusts a result).  The reference is the CPU oracle with float64
accumulators on the 16-bit-rounded inputs (oracle.forward / forward_cross, accum=1), float64 numpy for the log-sum-exp.

Tolerances are the project's, fixed before any run (tests/test_gpu_parity.py, tests/test_gpu_kvcache.py):
  fp16   max-abs MAX_ABS (1e-2), rel-L2 REL_L2[fp16]
  bf16   part A (peaked rows: near-one-hot rows, the first rows under the mask, logits spread x 6): max-abs cm.peaked_tol(bf16, vmax),
         rel-L2 3e-2 as test_redo_kernel_takes_the_blocks_the_fast_passes_refuse; the plain-forward inputs of
         test_optimistic_pass_overflow_fallback and part B keep MAX_ABS and REL_L2[bf16] as there
  16-bit output: the same max-abs bound and rel-L2 x 1.5, as test_golden_general and test_causal_vs_oracle
  lse    2 * P_EPS absolute, derived at the head of tests/test_gpu_kvcache.py
Two of our kernels (or two calls of one) are compared bit for bit, never to a tolerance.
Every case prints its max_abs / rel_l2 / lse_abs next to the bounds (pytest -s).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import common_inputs as cm
import fallback_inputs as fi

pytestmark = pytest.mark.gpu

MARKER = 0x7FA5C0DE                     # kMarker of fa_fwd_rp16_kernel.hpp
FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]


def _bounds(fmt, vmax, out_same, peaked):
    """(max-abs, rel-L2) of the module docstring."""
    ma = cm.MAX_ABS if (fmt == 0 or not peaked) else cm.peaked_tol(fmt, vmax)
    rl = cm.REL_L2[fmt] if (fmt == 0 or not peaked) else 3e-2
    return ma, rl * (1.5 if out_same else 1.0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _to_dev(torch, bits, fmt):
    return torch.from_numpy(np.array(bits, order="C").view(np.int16)).cuda().view(_tdtype(torch, fmt))   # (a copy: the builders' arrays are read-only)


def _forward(fa, torch, dev, fmt, algo, out_same, causal, out=None):
    """-> the device tensor (fp32 or 16-bit), synchronised"""
    q, k, v = dev
    o = fa.fa_forward(q, k, v, out_dtype=_tdtype(torch, fmt) if out_same else torch.float32, algo=algo, causal=causal, out=out)
    torch.cuda.synchronize()
    return o


def _raw(torch, t):
    """the tensor's bits, for NaN-proof equality"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check(oracle, got, want, fmt, what, vmax, out_same=False, peaked=True):
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    tol_ma, tol_rl = _bounds(fmt, vmax, out_same, peaked)
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} (bounds {tol_ma:.2e} {tol_rl:.1e})")
    assert np.isfinite(got).all(), what + ": not finite"
    assert ma <= tol_ma and rl <= tol_rl, f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} (bounds {tol_ma:.2e} {tol_rl:.1e})"


@functools.lru_cache(maxsize=None)
def _chain_ref(oracle, d, n, fmt):
    c = fi.chain_case(oracle, d, n, fmt)
    want = oracle.forward(c["q"], c["k"], c["v"], causal=True, accum=1, nthreads=8)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _plain_ref(oracle, d, n, fmt):
    c = fi.plain_case(oracle, d, n, fmt)
    want = oracle.forward(c["q"], c["k"], c["v"], accum=1, nthreads=8)
    want.setflags(write=False)
    return want


def _causal_algos(d):
    return (0, 24, 6, 2, 1) if d == 64 else (0, 24, 28, 2, 1)


CHAIN = [pytest.param(fmt, d, n, id=f"{cm.FMT_NAME[fmt]}-d{d}-n{n}") for d in (64, 128) for n in fi.CHAIN_N[d] for fmt in (0, 1)]


# ---- A. the fallback chain under the mask ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d,n", CHAIN)
def test_causal_chain_vs_oracle(fa, oracle, torch_cuda, fmt, d, n):
    """fallback_inputs.chain_case -- a benign head with a must-stay row, a head with spikes on the diagonal, on the last key of
    the last row and in the first half of a block only, a head spread x 6 with a huge future key -- through every kernel that
    implements the mask, fp32 and 16-bit output.  n puts the second half of row block 1 (the redo kernel's last half-block) out of
    the sequence, partly inside it, and wholly inside it.  Row 0 sees one key: O[:, 0] == V[:, 0], also where block 0 was redone
    (to 1e-6 in fp32; bit for bit with 16-bit output, V being representable there: the redo kernel's 16-bit store checked exactly).
    Rows in front of the huge key are compared on their own as well: the key lies in their future."""
    torch = torch_cuda
    case, want = fi.chain_case(oracle, d, n, fmt), _chain_ref(oracle, d, n, fmt)
    fi.assert_chain_case(case, fmt)
    assert np.isfinite(want).all()
    dev = tuple(_to_dev(torch, x, fmt) for x in case["bits"])
    vmax, fk = np.abs(case["v"]).max(), case["future_key"]
    for out_same in (False, True):
        for algo in _causal_algos(d):
            got = _forward(fa, torch, dev, fmt, algo, out_same, True).float().cpu().numpy()
            what = f"causal chain d={d} n={n} {cm.FMT_NAME[fmt]} algo={algo} out={'same' if out_same else 'fp32'}"
            _check(oracle, got, want, fmt, what, vmax, out_same)
            _check(oracle, got[2, :fk], want[2, :fk], fmt, what + " rows before the huge key", vmax, out_same)
            if out_same:
                assert np.array_equal(got[:, 0], case["v"][:, 0]), what + ": row 0 is not V[0]"
            else:
                np.testing.assert_allclose(got[:, 0], case["v"][:, 0], atol=1e-6, err_msg=what)


_exp_lib = None


def _exp():
    """libfa_mi355_exp.so (build() makes it): the product's kernels plus fa_lab_rp16_pass_ids."""
    global _exp_lib
    if _exp_lib is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        path = os.path.join(root, "flashattention_kernel_project_amd", "libfa_mi355_exp.so")
        assert os.path.exists(path), "make -C flashattention_kernel_project_amd/csrc experimental (build() does it)"
        from flashattention_kernel_project_amd import capi
        capi._share_torch_hip_runtime()
        L = C.CDLL(path)
        sig = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] + [C.c_int] * 3 + [C.c_void_p]
        L.fa_forward_ex.argtypes = sig
        L.fa_forward_causal.argtypes = sig
        L.fa_lab_rp16_pass_ids.argtypes = [C.c_void_p]
        _exp_lib = L
    return _exp_lib


def _pass_ids(torch, dev, algo, rows, causal, out_same=False):
    """tests/test_gpu_parity.py::_pass_ids for either forward and any row-block size (512 rows at d = 64, 256 at d = 128): which
    pass produced each row block -- 0 folded fast pass, 1 exact optimistic pass, 2 running-max pass in the kernel, 3 left to the
    redo kernel.  -> (ids [BH, blocks], the experimental library's output)"""
    L = _exp()
    q, k, v = dev
    BH, N, d = q.shape
    nblk = (N + rows - 1) // rows
    ids = torch.full((BH * nblk,), 255, dtype=torch.int32, device="cuda")
    out = torch.empty(q.shape, dtype=q.dtype if out_same else torch.float32, device="cuda")
    assert L.fa_lab_rp16_pass_ids(ids.data_ptr()) == 0
    try:
        fn = L.fa_forward_causal if causal else L.fa_forward_ex
        rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, BH, N, d, 1.0 / d ** 0.5,
                0 if q.dtype == torch.float16 else 1, 1 if out_same else 0, algo, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
    finally:
        assert L.fa_lab_rp16_pass_ids(None) == 0
    return ids.cpu().numpy().reshape(BH, nblk), out


@pytest.mark.parametrize("fmt,d,n", CHAIN)
def test_causal_chain_pass_identity(fa, oracle, torch_cuda, fmt, d, n):
    """The chain case really takes the path it was built for: under the mask, algo 24 (and 28 at d = 128) leaves every row block
    that holds a lift-40 / 150 / 110 row or belongs to the x 6 head to the redo kernel (id 3) and produces every block of the
    benign head -- the must-stay row's block included -- in a fast pass (id <= 1).  So the causal redo kernel ran on marked
    blocks, and the fast passes were not simply refused everywhere.  The product library computes what the experimental one
    does, bit for bit, for both output types."""
    torch = torch_cuda
    case = fi.chain_case(oracle, d, n, fmt)
    fi.assert_chain_case(case, fmt)
    dev = tuple(_to_dev(torch, x, fmt) for x in case["bits"])
    for algo in ((24,) if d == 64 else (24, 28)):
        for out_same in (False, True):
            ids, o_exp = _pass_ids(torch, dev, algo, case["rows"], True, out_same)
            print(f"pass ids d={d} n={n} {cm.FMT_NAME[fmt]} algo={algo} out_same={out_same}: {ids.tolist()}")
            assert ids.shape == case["fail"].shape
            assert (ids[case["fail"]] == 3).all() and (ids[~case["fail"]] <= 1).all(), (algo, ids.tolist())
            o = _forward(fa, torch, dev, fmt, algo, out_same, True)
            assert torch.equal(_raw(torch, o), _raw(torch, o_exp)), (algo, out_same)


@pytest.mark.parametrize("fmt", [0, 1])
def test_causal_large_grid_marked_blocks(fa, oracle, torch_cuda, fmt):
    """test_causal_large_grid_item_order with work for the redo kernel: 300 heads, every third with a lift-40 / 150 row in each of
    its row blocks.  The redo kernel has a persistent grid of its own, its own block lookup with the same direction alternation,
    and half-size blocks: 900 (d = 64) / 900 (d = 128) half-blocks on 256 CUs, marked and unmarked ones interleaved, every marked
    one to be computed exactly once.  All rows against fp32 torch ops on the GPU (the softmax subtracts the row maximum), three
    heads -- a spiked one among them -- against the oracle."""
    torch = torch_cuda
    for (bh, n, d) in ((300, 600, 64), (300, 300, 128)):
        case = fi.large_grid_case(oracle, bh, n, d, fmt)
        fi.assert_large_grid_case(case, fmt)
        q, k, v = (_to_dev(torch, x, fmt) for x in case["bits"])
        vmax = float(np.abs(case["v"]).max())
        s = (q.float() @ k.float().transpose(1, 2)) * (1.0 / d ** 0.5)
        s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device="cuda").tril_(), float("-inf"))
        want = torch.softmax(s, dim=-1) @ v.float()
        del s
        sample = (0, 151, 299)
        assert any(b == 151 for (b, _, _, _) in case["spikes"])
        want_cpu = {b: oracle.forward(case["q"][b:b + 1], case["k"][b:b + 1], case["v"][b:b + 1], causal=True, accum=1, nthreads=8)
                    for b in sample}
        for algo in (0, 24):
            o = fa.fa_forward(q, k, v, algo=algo, causal=True)
            torch.cuda.synchronize()
            err = float((o - want).abs().max())
            # (bf16 under the mask: the first rows have two or three keys -- peaked by construction)
            tol = cm.MAX_ABS if fmt == 0 else cm.peaked_tol(fmt, vmax)
            print(f"large grid bh={bh} n={n} d={d} {cm.FMT_NAME[fmt]} algo={algo}: max_abs={err:.3e} (bound {tol:.2e})")
            assert bool(torch.isfinite(o).all()) and err <= tol, (bh, n, d, algo, err)
            for b in sample:
                _check(oracle, o[b:b + 1].cpu().numpy(), want_cpu[b], fmt, f"large grid d={d} algo={algo} head {b}", vmax)
            del o
        del q, k, v, want
        torch.cuda.empty_cache()


PLAIN = [pytest.param(fmt, d, n, id=f"{cm.FMT_NAME[fmt]}-d{d}-n{n}") for (d, n) in ((64, 640), (64, 333), (128, 300), (128, 400)) for fmt in (0, 1)]


@pytest.mark.parametrize("fmt,d,n", PLAIN)
def test_plain_fallback_16bit_output(fa, oracle, torch_cuda, fmt, d, n):
    """Marker store -> redo kernel -> 16-bit store without a mask: the inputs of test_optimistic_pass_overflow_fallback (n = 640 and
    the ragged n = 333) and their d = 128 counterpart with out_dtype = the input type, where the marker word covers TWO output
    elements and the redo kernel looks for it at byte row * D * 2.  fp32 output alongside, on the same bounds as the parity test."""
    torch = torch_cuda
    case, want = fi.plain_case(oracle, d, n, fmt), _plain_ref(oracle, d, n, fmt)
    fi.assert_plain_case(case, fmt)
    dev = tuple(_to_dev(torch, x, fmt) for x in case["bits"])
    vmax = np.abs(case["v"]).max()
    for algo in (0, 23, 24, 26) + ((28,) if d == 128 else ()):
        for out_same in (True, False):
            got = _forward(fa, torch, dev, fmt, algo, out_same, False).float().cpu().numpy()
            _check(oracle, got, want, fmt, f"plain fallback d={d} n={n} {cm.FMT_NAME[fmt]} algo={algo} out={'same' if out_same else 'fp32'}",
                   vmax, out_same, peaked=False)
    if case["spikes"]:
        # the full-width kernel did leave the blocks of the rows that must fail to the redo kernel, with 16-bit output (the other
        # blocks see the spiked keys as well, without a mask: they are not asserted on); x 6 is beyond fp16's overflow point only
        ids, _ = _pass_ids(torch, dev, 24, case["rows"], False, True)
        print(f"pass ids plain d={d} n={n} {cm.FMT_NAME[fmt]}: {ids.tolist()}")
        must = sorted({(b, row // case["rows"]) for (b, row, _, lift) in case["spikes"] if fi.fails(lift, fmt)})
        assert must and all(ids[b, blk] == 3 for (b, blk) in must), (must, ids.tolist())
        assert fmt == 1 or (ids[2] == 3).all()


HYGIENE = [pytest.param(fmt, d, causal, out_same, id=f"{cm.FMT_NAME[fmt]}-d{d}-{'causal' if causal else 'plain'}-{'out16' if out_same else 'out32'}")
           for d in (64, 128) for causal in (False, True) for out_same in (False, True) for fmt in (0, 1)]


@pytest.mark.parametrize("fmt,d,causal,out_same", HYGIENE)
def test_marker_hygiene(fa, oracle, torch_cuda, fmt, d, causal, out_same):
    """The marker is a word in the caller's output buffer.  A hostile call (blocks marked and redone next to blocks that are not)
    into a buffer pre-filled with the marker pattern in every 32-bit word gives the bits it gives into a zeroed buffer (no stale
    word is taken for a marker that matters, no marker survives), finite wherever the oracle is; called twice it gives the same
    bits; and a (b, h) slice of it gives the bits of the full call.  The slice is compared bit for bit, not against the oracle,
    because the algo is explicit (24, and 28 at d = 128): the kernel is the same for both calls and every decision of the chain is
    taken per row block from that block's own rows and the head's keys -- the grid only changes which workgroup computes it."""
    torch = torch_cuda
    n = 800 if d == 64 else 400   # second half of block 1 partial (plain: n = 640 / 400)
    if causal:
        case, want = fi.chain_case(oracle, d, n, fmt), _chain_ref(oracle, d, n, fmt)
        fi.assert_chain_case(case, fmt)
    else:
        n = 640 if d == 64 else 400
        case, want = fi.plain_case(oracle, d, n, fmt), _plain_ref(oracle, d, n, fmt)
        fi.assert_plain_case(case, fmt)
    assert np.isfinite(want).all()
    dev = tuple(_to_dev(torch, x, fmt) for x in case["bits"])
    sub = tuple(x[1:3].contiguous() for x in dev)
    vmax = np.abs(case["v"]).max()
    for algo in ((24,) if d == 64 else (24, 28)):
        what = f"marker hygiene d={d} n={n} {cm.FMT_NAME[fmt]} algo={algo} causal={causal} out_same={out_same}"
        ids, _ = _pass_ids(torch, dev, algo, case["rows"], causal, out_same)
        # marked blocks in the launch; under the mask the benign head's unmarked ones beside them (without a mask every row
        # sees every spiked key, so no block is promised to a fast pass)
        assert (ids == 3).any() and (not causal or (ids <= 1).any()), (what, ids.tolist())
        dirty = torch.empty(dev[0].shape, dtype=_tdtype(torch, fmt) if out_same else torch.float32, device="cuda")
        dirty.view(torch.int32).fill_(MARKER)
        assert int(dirty.view(torch.int32)[0, 0, 0]) == MARKER
        a = _forward(fa, torch, dev, fmt, algo, out_same, causal, out=dirty)
        assert a.data_ptr() == dirty.data_ptr()
        b = _forward(fa, torch, dev, fmt, algo, out_same, causal, out=torch.zeros_like(dirty))
        assert bool(torch.isfinite(a).all()), what
        assert torch.equal(_raw(torch, a), _raw(torch, b)), what + ": the result depends on what the output buffer held"
        c = _forward(fa, torch, dev, fmt, algo, out_same, causal)
        assert torch.equal(_raw(torch, c), _raw(torch, b)), what + ": not reproducible"
        s = _forward(fa, torch, sub, fmt, algo, out_same, causal)
        assert torch.equal(_raw(torch, s), _raw(torch, b[1:3])), what + ": a (b, h) slice differs from the full call"
        _check(oracle, a.float().cpu().numpy(), want, fmt, what, vmax, out_same, peaked=causal)


# ---- B. split-KV and KV-cache under hostile logits ---------------------------------------------------------------------------
def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_splitkv_hostile_rows(fa, oracle, torch_cuda, fmt, d):
    """fallback_inputs.splitkv_case: five query rows per head against 8229 keys (26 splits and the merge) and against 200 (one
    pass), NaN-filled workspace, both output types.  Row 0's maximum climbs 7 log2 units per tile in key order.  The kernel votes
    against its REFERENCE (tmax - m_ref > kThr = 8), not against the tile before, and visits the tiles of a split in a rotated
    order: where it walks up the staircase, one step stays under the threshold and the second refreshes the reference, so weights
    reach about 2^7 before each refresh; where the rotation starts high (head 1 of the one-pass shape starts at tile 3) it walks
    down and the early weights are tiny instead.  Rows 1 and 2 jump by 40 and by 150 in the LAST split (every other split's
    partial has to vanish in the merge); row 3's tile 0 lies 210 above everything else (every split but the first vanishes; inside
    the first the rotated tile order meets tile 0 late); row 4 spikes on the last key, in the partial last tile."""
    torch = torch_cuda
    bh, nq = 2, 5
    for nk in (8229, 200):
        case = fi.splitkv_case(oracle, d, fmt, nk)
        fi.assert_splitkv_case(case)
        need = fa.splitkv_workspace_bytes(1, bh, nq, nk, d)
        if nk == 200:
            assert need == 0
        else:
            splits = need // (bh * nq * (d + 2) * 4)
            chunk = -(-((nk + 63) // 64) // splits) * 64
            assert splits > 1 and all(case["keys"][b, r][0] >= (splits - 1) * chunk for b in range(bh) for r in (1, 2, 4)), (splits, chunk)
        want = oracle.forward_cross(case["q"], case["k"], case["v"], accum=1, nthreads=8)
        assert np.isfinite(want).all()
        dq, dk, dv = (_to_dev(torch, x[None], fmt) for x in case["bits"])   # B = 1, H = bh
        vmax = np.abs(case["v"]).max()
        for out_same in (False, True):
            o = fa.fa_forward_splitkv(dq, dk, dv, out_dtype=_tdtype(torch, fmt) if out_same else torch.float32,
                                      workspace=_nan_workspace(torch, need))
            torch.cuda.synchronize()
            _check(oracle, o[0].float().cpu().numpy(), want, fmt, f"splitkv hostile d={d} nk={nk} {cm.FMT_NAME[fmt]} out_same={out_same}",
                   vmax, out_same, peaked=False)


def _kv_expected(oracle, case, lens, causal):
    """tests/test_gpu_kvcache.py::_expected on the case's arrays: -> (O [B*Hq, Nq, d] fp32, lse [B*Hq, Nq] float64)"""
    q, k, v = case["q"], case["k"], case["v"]
    B, G, Nq = fi.KV_SHAPE["B"], fi.KV_SHAPE["G"], fi.KV_SHAPE["Nq"]
    d = q.shape[2]
    out = np.zeros(q.shape, np.float32)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    scale = 1.0 / np.sqrt(d)
    for b in range(B):
        qs = slice(b * G, (b + 1) * G)
        kb, vb = (np.repeat(x[b:b + 1], G, axis=0) for x in (k, v))
        lim = cm.row_limits(int(lens[b]), Nq, Nq, causal)[1]
        for c in sorted(set(lim)):
            if c == 0:
                continue
            rows = [i for i in range(Nq) if lim[i] == c]
            out[qs, rows] = oracle.forward_cross(q[qs][:, rows], kb[:, :c], vb[:, :c], accum=1, nthreads=8)
            s = np.einsum("hid,hjd->hij", q[qs][:, rows].astype(np.float64), kb[:, :c].astype(np.float64)) * scale
            m = s.max(-1)
            lse[qs, rows] = m + np.log(np.exp(s - m[..., None]).sum(-1))
    return out, lse


def _kv_run(fa, torch, case, lens, fmt, causal=False, out_same=False, key0=0):
    """-> (O [B*Hq, Nq, d] fp32 numpy, lse [B*Hq, Nq] fp32 numpy); NaN bit patterns at and past each length, NaN-filled workspace"""
    B, Hkv, G, Nq = (fi.KV_SHAPE[x] for x in ("B", "Hkv", "G", "Nq"))
    qb, kb, vb = case["bits"]
    kb, vb = kb[:, key0:], vb[:, key0:]
    Ncap, d = kb.shape[1], kb.shape[2]

    def cache(bits):
        bits = bits.reshape(B, Hkv, Ncap, d).copy()
        for b in range(B):
            bits[b, :, max(int(lens[b]), 0):] = cm.NAN16
        return _to_dev(torch, bits, fmt)

    dq = _to_dev(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    assert need > 0
    o, lse = fa.fa_forward_kvcache(dq, cache(kb), cache(vb), torch.tensor(list(lens), dtype=torch.int32, device="cuda"), causal=causal,
                                   out_dtype=_tdtype(torch, fmt) if out_same else torch.float32, return_lse=True,
                                   workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o.float().cpu().numpy().reshape(B * Hkv * G, Nq, d), lse.cpu().numpy().reshape(B * Hkv * G, Nq)


def _kv_check(oracle, got, got_lse, want, want_lse, fmt, what, vmax, out_same=False):
    """tests/test_gpu_kvcache.py::_check"""
    live = np.isfinite(want_lse)
    le = float(np.abs(got_lse[live] - want_lse[live]).max()) if live.any() else 0.0
    print(f"{what}: lse_abs={le:.3e} (bound {2 * cm.P_EPS[fmt]:.2e})")
    assert not np.isnan(got_lse).any(), what + ": NaN in lse"
    _check(oracle, got, want, fmt, what, vmax, out_same, peaked=False)
    assert (got[~live] == 0.0).all(), what + ": a row without a key is not exactly zero"
    assert (got_lse[~live] == -np.inf).all(), what + ": a row without a key has lse != -inf"
    assert np.isfinite(got_lse[live]).all(), what
    assert le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_kvcache_hostile_logits(fa, oracle, torch_cuda, fmt, d, causal):
    """fallback_inputs.kvcache_case, lengths (66, 4096, 130), five query rows in two folded heads: spikes of +40 / +150 on keys 65
    and 64 of the 66-key sequence (under the end-aligned mask only the last rows see them: the row's reference stays at -inf, or
    at tile 0's level, until then), +40 on key 4000 of the full sequence (a late split), and one sequence whose two heads sit at
    -300 and +300 log2 units: the lse (about -208 and +208) must be finite and within the bound.  Both output types.
    (With these lengths every row has a key, so the zero / -inf branch of _kv_check is idle here; test_lse_merges_spiked_ranges has
    a sequence without keys, and tests/test_gpu_kvcache.py covers such rows under the mask.)"""
    case = fi.kvcache_case(oracle, d, fmt)
    fi.assert_kvcache_case(case, causal)
    want, want_lse = _kv_expected(oracle, case, fi.KV_LENS, causal)
    assert np.isfinite(want).all() and np.isfinite(want_lse).all()
    assert abs(want_lse[4].mean() + 300 * fi.LN2) < 10 and abs(want_lse[5].mean() - 300 * fi.LN2) < 10
    vmax = np.abs(case["v"]).max()
    for out_same in (False, True):
        got, lse = _kv_run(fa, torch_cuda, case, fi.KV_LENS, fmt, causal=causal, out_same=out_same)
        _kv_check(oracle, got, lse, want, want_lse, fmt, f"kvcache hostile d={d} {cm.FMT_NAME[fmt]} causal={causal} out_same={out_same}",
                  vmax, out_same)


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_lse_merges_spiked_ranges(fa, oracle, torch_cuda, fmt, d):
    """test_lse_merges_key_ranges on the hostile case, the key axis cut at 100: the dominant key of the full sequence's spiked row
    (key 4000) lies in the second range only, the 66-key sequence has nothing there (lse = -inf, weight 0), the +-300 sequence
    has 100 and 30 keys.  Two calls, merged in numpy through their log-sum-exps, give the result over the whole range."""
    case, a = fi.kvcache_case(oracle, d, fmt), fi.KV_CUT
    fi.assert_kvcache_case(case, False)
    want, want_lse = _kv_expected(oracle, case, fi.KV_LENS, False)
    o1, l1 = _kv_run(fa, torch_cuda, case, tuple(min(n, a) for n in fi.KV_LENS), fmt)
    o2, l2 = _kv_run(fa, torch_cuda, case, tuple(max(n - a, 0) for n in fi.KV_LENS), fmt, key0=a)
    G = fi.KV_SHAPE["G"]
    assert np.isfinite(l1).all() and (l2[:G] == -np.inf).all() and np.isfinite(l2[G:]).all()
    assert (o2[:G] == 0.0).all()
    h, row = case["spikes"][2][:2]
    assert l2[h, row] - l1[h, row] > 20.0, "the second range dominates the spiked row"
    l1, l2 = l1.astype(np.float64), l2.astype(np.float64)
    lse = np.logaddexp(l1, l2)
    merged = o1 * np.exp(l1 - lse)[..., None] + o2 * np.exp(l2 - lse)[..., None]
    ma, le = oracle.max_abs(merged.astype(np.float32), want), float(np.abs(lse - want_lse).max())
    print(f"merged over two key ranges, hostile, d={d} {cm.FMT_NAME[fmt]}: max_abs={ma:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert np.isfinite(merged).all()
    assert ma <= cm.MAX_ABS
    assert le <= 2 * cm.P_EPS[fmt]
