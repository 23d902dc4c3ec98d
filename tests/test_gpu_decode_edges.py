"""GPU tier of the decode family -- fa_forward_splitkv, fa_forward_kvcache, fa_forward_kvcache_paged and the merge kernel behind
them -- in the regimes the hand-picked shapes of the other files leave out:

A. more than 64 splits (S = 129): the second trip of the merge's max loop and the remainder of its unrolled accumulation;
B. the causal mask on folded heads whose edges fall inside waves and across query blocks, rows that are dead in one live split
   and live in the others, more query rows than keys, 16-bit output behind a split;
C. 48 lengths in one launch: on and next to every tile, chunk and page edge, and the clamp of lengths outside [0, Ncap];
D. the scale argument: 0.3, negative, and 0 (uniform weights) -- also on fa_forward_splitkv and fa_forward;
E. K/V heads and pages past 2^31 and 2^32 elements.

Inputs and expected outputs come from tests/decode_inputs.py (tests/test_decode_inputs.py shows without a GPU that each reaches
its regime).  The hygiene of tests/test_gpu_kvcache_paged.py holds in every case: NaN bit patterns in every cache row at or past
a sequence's length and in every page no table names, garbage in the dead table entries, a NaN-filled workspace; a row without a
key must be exactly 0 with lse = -inf.

Tolerances are the project's, fixed before any run: max-abs 1e-2, relative L2 2e-3 (fp16) / 1.2e-2 (bf16), x 1.5 with 16-bit
output, lse within 2 * P_EPS.  Where the input makes peaked rows (the spikes of case A, scale 0.3) the max-abs bound is
peaked_tol of tests/common_inputs.py.  Wherever the paged and the contiguous entry run on the same keys, O and lse are also
compared bit for bit.  Every case prints its figures next to the bounds (pytest -s).

That the cases bite was measured on scratch builds of the library (one edit each, never committed; all give wrong numbers inside
the allocations), 102 cases per run on an MI355X:
  merge accumulates the first 64 splits only      16 fail: every test_many_splits_kvcache and _splitkv case
  merge takes M over the first 64 splits only      8 fail: the spiked cases of both (O not finite: the sequence with the +150 key alone)
  `q_row % Nq1` -> `q_row`                         24 fail: test_folded_causal_mask 8, test_length_sweep 4, test_scale_kvcache 12 (causal)
  `lim` -> `lim_lo` in the element mask            24 fail: the same cases
  q_flip dropped                                   12 fail: scale -0.2 in test_scale_kvcache 8 and test_scale_splitkv 4
  floor for ceil in the per-sequence tile count    41 fail: folded mask 8, length sweep 8, scale_kvcache 24, heads_past_4g 1
  page block offset truncated to 32 bits            1 fails: test_pages_past_4g_elements_paged
  head offset truncated to 32 bits                  1 fails: test_heads_past_4g_elements_contiguous
  kCache clamp of c dropped                        not detectable since host_scale_log2e() hands the kernels +-FLT_MIN: with that
                                                   host rule dropped as well, 12 fail (scale 0 in test_scale_kvcache 8, test_scale_splitkv 4)
"""
import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
GIB = 1 << 30


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _to_dev(torch, bits, fmt):
    return torch.from_numpy(np.array(bits, order="C").view(np.int16)).cuda().view(_tdtype(torch, fmt))   # (a copy: the builders' arrays are read-only)


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _shape(s):
    return tuple(s[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))


def _lens_dev(torch, lens):
    return torch.tensor(list(lens), dtype=torch.int32, device="cuda")


def _contig(fa, torch, bits, lens, shape, fmt, causal=False, out_same=False, scale=None, splits=None):
    """fa_forward_kvcache on the poisoned cache -> (O, lse) device tensors"""
    B, Hkv, G, Nq, Ncap = shape
    qb, kb, vb = bits
    d = qb.shape[2]
    dq = _to_dev(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    dk, dv = (_to_dev(torch, cm.poisoned(x.reshape(B, Hkv, Ncap, d), lens), fmt) for x in (kb, vb))
    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    assert splits is None or di.splits_of(need, B * Hkv, G * Nq, d) == splits
    o, lse = fa.fa_forward_kvcache(dq, dk, dv, _lens_dev(torch, lens), causal=causal, scale=scale,
                                   out_dtype=_tdtype(torch, fmt) if out_same else torch.float32, return_lse=True,
                                   workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o, lse


def _paged(fa, torch, bits, lens, shape, fmt, ps, seed, causal=False, out_same=False, scale=None):
    """fa_forward_kvcache_paged on the same keys scattered into a pool -> (O, lse) device tensors"""
    B, Hkv, G, Nq, Ncap = shape
    qb, kb, vb = bits
    d = qb.shape[2]
    kp, vp, table = cm.scatter(kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), lens, ps, seed)
    dq = _to_dev(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    need = fa.kvcache_paged_workspace_bytes(B, Hkv, G, Nq, Ncap // ps, ps, d)
    assert need == fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    o, lse = fa.fa_forward_kvcache_paged(dq, _to_dev(torch, kp, fmt), _to_dev(torch, vp, fmt), torch.from_numpy(table).cuda(),
                                         _lens_dev(torch, lens), causal=causal, scale=scale,
                                         out_dtype=_tdtype(torch, fmt) if out_same else torch.float32, return_lse=True,
                                         workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o, lse


def _host(t, shape):
    return t.float().cpu().numpy().reshape(shape)


def _check(oracle, res, want, want_lse, fmt, what, out_same=False, max_abs=cm.MAX_ABS):
    """the checks of tests/test_gpu_kvcache.py::_check; res = (O, lse) device tensors, or O alone (want_lse None)"""
    o, lse = res if isinstance(res, tuple) else (res, None)
    got = _host(o, want.shape)
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    tol_rl = cm.REL_L2[fmt] * (1.5 if out_same else 1.0)
    assert np.isfinite(got).all(), what + ": O is not finite"
    if lse is None:
        print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} (bounds {max_abs:.2e} {tol_rl:.1e})")
        assert ma <= max_abs and rl <= tol_rl, f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
        return
    got_lse = _host(lse, want_lse.shape)
    live = np.isfinite(want_lse)
    le = float(np.abs(got_lse[live] - want_lse[live]).max()) if live.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {max_abs:.2e} {tol_rl:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert not np.isnan(got_lse).any(), what + ": NaN in lse"
    assert ma <= max_abs and rl <= tol_rl, f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert (got[~live] == 0.0).all(), what + ": a row without a key is not exactly zero"
    assert (got_lse[~live] == -np.inf).all(), what + ": a row without a key has lse != -inf"
    assert np.isfinite(got_lse[live]).all(), what
    assert le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"


def _same_bits(torch, a, b, what):
    """O and lse of the paged entry equal the contiguous entry's bit for bit"""
    for x, y, name in zip(a, b, ("O", "lse")):
        assert not torch.isnan(x).any() and torch.equal(x, y), f"{what}: {name} of the paged entry differs from the contiguous entry's"


_REF = {}


def _reference(oracle, key, q, k, v, lens, shape, causal, scale=None):
    """cm.expected, computed once per case and shared (read-only)"""
    if key not in _REF:
        B, Hkv, G, Nq, _ = shape
        out, lse = cm.expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal, scale=scale)
        out.setflags(write=False), lse.setflags(write=False)
        _REF[key] = (out, lse)
    return _REF[key]


# ---- A. more than 64 splits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spiked", [False, True], ids=["benign", "spiked"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_many_splits_kvcache(fa, oracle, torch_cuda, fmt, d, spiked):
    """S = 129 in both cache entries, one query row per sequence: 33024 keys (every split live) beside 20001 (105 live splits of
    three tiles, 24 empty).  Benign weights do not notice a wrong reference maximum (M cancels in the merge), so the rows also run
    with their maximum 150 log2 units up in a split of index >= 64 -- beside a second peak at +40 in split 10 (sequence 0), and
    alone (sequence 1).  Both output types; the paged entry (pages of 256) equals the contiguous one bit for bit."""
    torch, shape = torch_cuda, _shape(di.A_SHAPE)
    case = di.case_a(oracle, d, fmt, "kvcache", spiked)
    di.assert_case_a(case, di.A_SPLITS)
    want, want_lse = _reference(oracle, ("A", d, fmt, spiked), case["q"], case["k"], case["v"], case["lens"], shape, False)
    tol = cm.peaked_tol(fmt, np.abs(case["v"]).max()) if spiked else cm.MAX_ABS
    for out_same in (False, True):
        what = f"A kvcache d={d} {cm.FMT_NAME[fmt]} spiked={spiked} out_same={out_same}"
        base = _contig(fa, torch, case["bits"], case["lens"], shape, fmt, out_same=out_same, splits=di.A_SPLITS)
        _check(oracle, base, want, want_lse, fmt, what, out_same, tol)
        got = _paged(fa, torch, case["bits"], case["lens"], shape, fmt, di.A_PAGE, seed=d + fmt, out_same=out_same)
        _check(oracle, got, want, want_lse, fmt, what + " paged", out_same, tol)
        _same_bits(torch, got, base, what)


@pytest.mark.parametrize("spiked", [False, True], ids=["benign", "spiked"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_many_splits_splitkv(fa, oracle, torch_cuda, fmt, d, spiked):
    """The plain merge instantiation at S = 129: two heads of one query row against 33000 keys (a ragged last split), benign and
    with the spikes of case A (head 1's lies in the last split, index 128)."""
    torch, s = torch_cuda, di.A_SPLITKV
    case = di.case_a(oracle, d, fmt, "splitkv", spiked)
    di.assert_case_a(case, di.A_SPLITS)
    need = fa.splitkv_workspace_bytes(1, s["bh"], s["nq"], s["nk"], d)
    assert di.splits_of(need, s["bh"], s["nq"], d) == di.A_SPLITS
    want = oracle.forward_cross(case["q"], case["k"], case["v"], accum=1, nthreads=8)
    assert np.isfinite(want).all()
    dq, dk, dv = (_to_dev(torch, x[None], fmt) for x in case["bits"])   # B = 1, H = bh
    tol = cm.peaked_tol(fmt, np.abs(case["v"]).max()) if spiked else cm.MAX_ABS
    for out_same in (False, True):
        o = fa.fa_forward_splitkv(dq, dk, dv, out_dtype=_tdtype(torch, fmt) if out_same else torch.float32,
                                  workspace=_nan_workspace(torch, need))
        torch.cuda.synchronize()
        _check(oracle, o, want, None, fmt, f"A splitkv d={d} {cm.FMT_NAME[fmt]} spiked={spiked} out_same={out_same}", out_same, tol)


# ---- B. the causal mask on folded heads -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", di.B_PAGES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_folded_causal_mask(fa, oracle, torch_cuda, fmt, d, ps):
    """Eight folded heads of 20 rows per K/V head (160 rows: head edges inside waves, two query blocks), S = 5, causal.  1030 keys:
    keys 1024-1029 sit alone in split 4, where rows 0-13 of every folded head are dead while rows 14-19 -- in the same waves --
    are live; those rows' partials there must be (m = -inf, l = 0, O = 0) and weigh 0 in the merge.  7 keys: rows 0-12 of every
    folded head see nothing.  Both cache entries (bit-equal), and the contiguous one with 16-bit output behind the split."""
    torch, shape = torch_cuda, _shape(di.B_SHAPE)
    B, Hkv, G, Nq, Ncap = shape
    (q, k, v), bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 3300)
    want, want_lse = _reference(oracle, ("B", d, fmt), q, k, v, di.B_LENS, shape, True)
    dead = np.isinf(want_lse).reshape(B, Hkv * G, Nq)
    assert not dead[0].any() and (dead[1] == (np.arange(Nq) < 13)[None, :]).all()
    what = f"B folded causal d={d} {cm.FMT_NAME[fmt]} page={ps}"
    base = _contig(fa, torch, bits, di.B_LENS, shape, fmt, causal=True, splits=di.B_SPLITS)
    _check(oracle, base, want, want_lse, fmt, what)
    got = _paged(fa, torch, bits, di.B_LENS, shape, fmt, ps, seed=ps + d + fmt, causal=True)
    _check(oracle, got, want, want_lse, fmt, what + " paged")
    _same_bits(torch, got, base, what)
    low = _contig(fa, torch, bits, di.B_LENS, shape, fmt, causal=True, out_same=True)
    _check(oracle, low, want, want_lse, fmt, what + " out_same", out_same=True)


# ---- C. a sweep of lengths in one launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_length_sweep(fa, oracle, torch_cuda, fmt, d, causal):
    """48 sequences, one length each (decode_inputs.C_FIXED and seeded random ones), S = 4: every sequence has its own chunk, so
    tile, chunk and page edges fall differently in each.  Lengths -1, INT_MIN, 1025 and INT_MAX are clamped into [0, 1024] by the
    kernel; their reference is the clamped length's (a too-long sequence has a fully valid cache row and table row).  The
    contiguous entry and the paged one with pages of 16 and 256 keys, bit-equal."""
    torch, shape = torch_cuda, _shape(di.C_SHAPE)
    B, Hkv, G, Nq, Ncap = shape
    lens = di.c_lens()
    assert di.length_categories(lens, Ncap, di.C_SPLITS, di.C_PAGES) >= di.c_categories_wanted(di.C_PAGES)
    (q, k, v), bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 3400)
    want, want_lse = _reference(oracle, ("C", d, fmt, causal), q, k, v, lens, shape, causal)
    what = f"C length sweep d={d} {cm.FMT_NAME[fmt]} causal={causal}"
    base = _contig(fa, torch, bits, lens, shape, fmt, causal=causal, splits=di.C_SPLITS)
    _check(oracle, base, want, want_lse, fmt, what)
    for ps in di.C_PAGES:
        got = _paged(fa, torch, bits, lens, shape, fmt, ps, seed=ps + d + fmt, causal=causal)
        _check(oracle, got, want, want_lse, fmt, f"{what} page={ps}")
        _same_bits(torch, got, base, f"{what} page={ps}")


# ---- D. scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", di.D_SCALES)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_scale_kvcache(fa, oracle, torch_cuda, fmt, d, causal, scale):
    """The scale argument in both cache entries, lengths (0, 2, 66, 200, 1024, 1, 513, 777), S = 4: 0.3 (peaked rows), -0.2 (the
    kernels flip the sign of Q and keep |scale|), and 0: every visible key weighs the same, O is the mean of the visible V rows
    and lse = ln(their number) -- a masked key must not turn into 0 * -inf."""
    torch, shape = torch_cuda, _shape(di.D_SHAPE)
    B, Hkv, G, Nq, Ncap = shape
    (q, k, v), bits = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, 3500)
    want, want_lse = _reference(oracle, ("D", d, fmt, causal, scale), q, k, v, di.D_LENS, shape, causal, scale)
    if scale == 0.0:
        uo, ul = cm.uniform_expected(v, di.D_LENS, B, Hkv, G, Nq, causal)
        assert np.abs(want - uo).max() < 1e-6 and np.array_equal(np.isfinite(ul), np.isfinite(want_lse))
    tol = cm.peaked_tol(fmt, np.abs(v).max()) if scale == 0.3 else cm.MAX_ABS
    what = f"D scale={scale} d={d} {cm.FMT_NAME[fmt]} causal={causal}"
    base = _contig(fa, torch, bits, di.D_LENS, shape, fmt, causal=causal, scale=scale, splits=4)
    _check(oracle, base, want, want_lse, fmt, what, max_abs=tol)
    got = _paged(fa, torch, bits, di.D_LENS, shape, fmt, di.D_PAGE, seed=d + fmt, causal=causal, scale=scale)
    _check(oracle, got, want, want_lse, fmt, what + " paged", max_abs=tol)
    _same_bits(torch, got, base, what)


@pytest.mark.parametrize("scale", [-0.2, 0.0])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_scale_splitkv(fa, oracle, torch_cuda, fmt, d, scale):
    """fa_forward_splitkv at a negative scale and at 0, in one pass (5 rows x 100 keys) and behind the merge (3 rows x 8229 keys).
    Both key counts end in a ragged tile: the keys past Nk are masked to -inf there, and scale 0 must not turn them into NaN."""
    torch = torch_cuda
    for (nq, nk) in di.D_SPLITKV:
        (q, _, _), (qb, _, _) = oracle.make_qkv(2, nq, d, fmt=fmt, seed=3700 + nk)
        (_, k, v), (_, kb, vb) = oracle.make_qkv(2, nk, d, fmt=fmt, seed=3701 + nk)
        want = oracle.forward_cross(q, k, v, scale=scale, accum=1, nthreads=8)
        if scale == 0.0:
            assert np.abs(want - v.astype(np.float64).mean(1)[:, None, :]).max() < 1e-6
        need = fa.splitkv_workspace_bytes(1, 2, nq, nk, d)
        assert (need > 0) == (nk > 1000)
        o = fa.fa_forward_splitkv(*(_to_dev(torch, x[None], fmt) for x in (qb, kb, vb)), scale=scale, workspace=_nan_workspace(torch, need))
        torch.cuda.synchronize()
        _check(oracle, o, want, None, fmt, f"D splitkv scale={scale} d={d} {cm.FMT_NAME[fmt]} nq={nq} nk={nk}")


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("algo", [0, 1, 2], ids=["auto", "generic", "tiled"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_scale_zero_forward(fa, oracle, torch_cuda, fmt, algo, causal):
    """fa_forward at scale 0 with a ragged N (100 rows, d = 64), with and without the mask: row i is the mean of the V rows it sees."""
    torch, f = torch_cuda, di.D_FORWARD
    (q, k, v), bits = oracle.make_qkv(f["bh"], f["n"], f["d"], fmt=fmt, seed=3600)
    want = oracle.forward(q, k, v, scale=0.0, accum=1, nthreads=4, causal=causal)
    o = fa.fa_forward(*(_to_dev(torch, x, fmt) for x in bits), scale=0.0, algo=algo, causal=causal)
    torch.cuda.synchronize()
    _check(oracle, o, want, None, fmt, f"D fa_forward scale=0 {cm.FMT_NAME[fmt]} algo={algo} causal={causal}")


# the kernels behind fa_forward that the N = 100 case above does not reach: (d, n, algo, causal); n is ragged and spans two row blocks
PIPELINE = [(64, 600, 5, False), (64, 600, 6, False), (64, 600, 23, False), (64, 600, 24, False), (64, 600, 26, False),
            (64, 600, 27, False), (64, 600, 24, True), (64, 600, 6, True), (128, 300, 24, False), (128, 300, 28, False),
            (128, 300, 24, True), (128, 300, 28, True)]


@pytest.mark.parametrize("d,n,algo,causal", PIPELINE, ids=[f"d{d}-n{n}-algo{a}-{'causal' if c else 'full'}" for (d, n, a, c) in PIPELINE])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_scale_zero_forward_pipeline(fa, oracle, torch_cuda, fmt, d, n, algo, causal):
    """Scale 0 through the interleaved kernels (5, 6), the rolling pipeline on every wave width (23, 24, 26, 27, 28; the fold is
    off at scale 0, the exact passes run) and the 128-row tiled kernel under the mask (6, causal), at a ragged N over two row
    blocks: uniform weights, never NaN."""
    torch = torch_cuda
    (q, k, v), bits = oracle.make_qkv(2, n, d, fmt=fmt, seed=3650 + d)
    want = oracle.forward(q, k, v, scale=0.0, accum=1, nthreads=4, causal=causal)
    mean = np.cumsum(v.astype(np.float64), 1) / np.arange(1, n + 1)[None, :, None] if causal else v.astype(np.float64).mean(1, keepdims=True)
    assert np.abs(want - mean).max() < 1e-6
    o = fa.fa_forward(*(_to_dev(torch, x, fmt) for x in bits), scale=0.0, algo=algo, causal=causal)
    torch.cuda.synchronize()
    _check(oracle, o, want, None, fmt, f"D fa_forward scale=0 d={d} n={n} {cm.FMT_NAME[fmt]} algo={algo} causal={causal}")


# ---- E. addresses past 2^32 elements --------------------------------------------------------------------------------------------
def _need_memory(torch, nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{free / GIB:.1f} GiB of device memory free, the case needs {nbytes / GIB:.1f}")


def _live_reference(oracle, d, fmt, lens, seed, ncap):
    """the live sequences of a case E shape as a small problem of their own: Hkv = G = Nq = 1"""
    n = len(lens)
    (q, k, v), bits = di.inputs(oracle, n, 1, 1, 1, ncap, d, fmt, seed)
    want, want_lse = _reference(oracle, ("E", seed), q, k, v, lens, (n, 1, 1, 1, ncap), False)
    return bits, want, want_lse


def test_heads_past_4g_elements_contiguous(fa, oracle, torch_cuda):
    """A cache of 8200 sequences x 4096 keys x 128 (2^32 + 2^22 elements per tensor, 8.6 GB each), uninitialised; every length is
    0 but those of sequences 0, 4097, 8193 and 8199, whose heads start at 0, just past 2^31 and just past 2^32 elements and hold
    real keys (NaN past their lengths).  Heads 1 and 7 -- where a head offset wrapped at 2^31 or 2^32 bytes or elements would
    land -- hold NaN.  The live sequences match the oracle, every other output row is exactly 0 with lse = -inf."""
    torch, e, fmt = torch_cuda, di.E_CONTIG, 0
    B, Ncap, d = e["B"], e["Ncap"], e["d"]
    _need_memory(torch, 2 * B * Ncap * d * 2 + GIB // 2)
    live = [b for (b, _) in di.E_CONTIG_LIVE]
    lens_live = tuple(L for (_, L) in di.E_CONTIG_LIVE)
    (qb, kb, vb), want, want_lse = _live_reference(oracle, d, fmt, lens_live, 3800, Ncap)
    dk, dv = (torch.empty((B, 1, Ncap, d), dtype=torch.float16, device="cuda") for _ in range(2))
    assert dk.numel() > 2 ** 32
    for t, src in ((dk, kb), (dv, vb)):
        for b in di.wrap_aliases(live, Ncap * d, B):
            t[b].fill_(float("nan"))
        rows = _to_dev(torch, cm.poisoned(src[:, None], lens_live), fmt)
        for i, b in enumerate(live):
            t[b].copy_(rows[i])
    dq = torch.randn((B, 1, 1, d), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda").half()
    dq[live] = _to_dev(torch, qb, fmt).view(len(live), 1, 1, d)
    lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    lens[live] = _lens_dev(torch, lens_live)
    assert fa.kvcache_workspace_bytes(B, 1, 1, 1, Ncap, d) == 0
    o, lse = fa.fa_forward_kvcache(dq, dk, dv, lens, return_lse=True)
    torch.cuda.synchronize()
    del dk, dv
    _check(oracle, (o[live], lse[live]), want, want_lse, fmt, "E contiguous, live sequences")
    rest = torch.ones(B, dtype=torch.bool, device="cuda")
    rest[live] = False
    assert bool((o[rest] == 0.0).all()) and bool((lse[rest] == -np.inf).all()), "a sequence of length 0 is not exactly zero"
    torch.cuda.empty_cache()


def test_pages_past_4g_elements_paged(fa, oracle, torch_cuda):
    """Pools of 131100 pages x 256 keys x 128 (2^32 + 28 pages of elements, 8.6 GB each), uninitialised; two sequences (S = 8)
    whose tables name pages next to 5, 65543 (past 2^31 elements), 131081 and 131099 (past 2^32).  The pages a wrapped page
    offset would land in (7-11, 25-27) hold NaN, the dead table entries garbage."""
    torch, p, fmt = torch_cuda, di.E_PAGED, 0
    B, ps, max_pages, num_pages, d = p["B"], p["ps"], p["max_pages"], p["num_pages"], p["d"]
    _need_memory(torch, 2 * num_pages * ps * d * 2 + GIB // 2)
    Ncap = ps * max_pages
    (qb, kb, vb), want, want_lse = _live_reference(oracle, d, fmt, di.E_PAGED_LENS, 3900, Ncap)
    kp, vp = (torch.empty((num_pages, 1, ps, d), dtype=torch.float16, device="cuda") for _ in range(2))
    assert kp.numel() > 2 ** 32
    table = np.array([[cm.GARBAGE[i % 2] for i in range(max_pages)] for _ in range(B)], np.int32)
    named = [x for row in di.E_PAGED_TABLE for x in row]
    for pool, src in ((kp, kb), (vp, vb)):
        for page in di.wrap_aliases(named, ps * d, num_pages):
            pool[page].fill_(float("nan"))
        rows = _to_dev(torch, cm.poisoned(src[:, None], di.E_PAGED_LENS), fmt)   # [B, 1, Ncap, d], NaN past the lengths
        for b, entries in enumerate(di.E_PAGED_TABLE):
            for pi, page in enumerate(entries):
                table[b, pi] = page
                pool[page].copy_(rows[b, :, pi * ps:(pi + 1) * ps])
    need = fa.kvcache_paged_workspace_bytes(B, 1, 1, 1, max_pages, ps, d)
    assert di.splits_of(need, B, 1, d) == 8
    dq = _to_dev(torch, qb, fmt).view(B, 1, 1, d)
    got = fa.fa_forward_kvcache_paged(dq, kp, vp, torch.from_numpy(table).cuda(), _lens_dev(torch, di.E_PAGED_LENS), return_lse=True,
                                      workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    del kp, vp
    _check(oracle, got, want, want_lse, fmt, "E paged")
    torch.cuda.empty_cache()
