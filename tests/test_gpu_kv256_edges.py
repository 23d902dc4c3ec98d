"""GPU tier of fa_kvcache_decode_d256 at the edges tests/test_gpu_kv256.py (Ncap = 256, N(0,1) logits) cannot reach; inputs, limits
and the model from tests/kv256_inputs.py, whose CPU tier (tests/test_kv256_inputs.py) shows that they force what they are named for.

A. key census (K = 0, coded V): every visible key counted exactly once over 16 tiles, S in {1, 3, 5, 7, 16, 0}, windows 3, 70 and
   300, pages of 16 up to 1024 keys (a page of several tiles), 40 rows in two blocks, lengths 0, 1, 3 below n_b.  ci.census_check
   (margin 0.25) and lse = ln(count) within 2 * P_EPS; every paged launch returns the contiguous launch's bits
B. softmax range: staircases, jumps of 40 and 150, a fall of 210, masked spikes and logits near -300 / +300 -- the rescale of O and
   l, the vote of two blocks and the merge by 2^(m_s - M) do work here.  sr.check_packed at sr.bounds, against float64
C. random inputs against cm.expected_f64: 48 lengths in one launch, 128 / 35 / 3 rows, Ncap = 1000, scales 0.3, -0.2 and 0, and
   num_splits = 0 where the rule gives four splits
D. K/V heads and pages whose byte offsets lie past 2^32 and 2^33 (8.6 GB per tensor; skipped where the memory is missing)

Every call: packed Q with NaN in the tokens of no sequence, sentinel-filled O and lse whose tokens of no sequence must keep the
sentinel, caches with NaN past each length and below each window start, pools with NaN pages no table names and garbage in the dead
table entries, and behind a split a workspace of exactly kvcache_decode_d256_workspace_bytes(...) filled with 0xFF.  No bound is
new: cm.MAX_ABS, cm.REL_L2, 2 * cm.P_EPS, cm.peaked_tol, sr.bounds, ci.MARGIN.  profiles/kv256_edges.txt holds one run's CENSUS| and
RANGE| lines, the wall times, and the eight scratch edits of the kernel each of which fails a test here.
"""
import numpy as np
import pytest

import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv
import kv256_inputs as kv
import test_gpu_decode_edges as tde

pytestmark = pytest.mark.gpu

FMTS = [pytest.param(fmt, id=cm.FMT_NAME[fmt]) for fmt in (0, 1)]
MASKS = [pytest.param(True, id="causal"), pytest.param(False, id="full")]
ENTRY = "fa_kvcache_decode_d256"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ints(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.int64).clip(cm.INT_MIN, cm.INT_MAX).astype(np.int32)).cuda()


def _launch(fa, torch, p, causal, W=0, S=1, ps=0, out16=False, softcap=0.0, scale=None, dev=None):
    """one call on a kv.Problem under the module docstring's conditions -> (O, lse) device tensors.  dev: a dict that keeps the device
    caches of (W, page size) between the launches of one test"""
    fmt = p.fmt
    if dev is None or (W, ps) not in (dev or {}):
        if ps:
            kp, vp, tb = p.pools(ps, W)
            entry = (cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(tb).cuda())
        else:
            entry = tuple(cm.dev16(torch, x, fmt) for x in p.caches(W)) + (None,)
        if dev is not None:
            dev[W, ps] = entry
    else:
        entry = dev[W, ps]
    kc, vc, table = entry
    q = cm.dev16(torch, p.packed_q(), fmt)
    free = torch.from_numpy(~p.lay.owned).cuda()
    assert torch.isnan(q[free]).all()
    out = torch.empty((p.lay.total_q, p.Hq, kv.D), dtype=q.dtype if out16 else torch.float32, device="cuda")
    out.view(torch.int16 if out16 else torch.int32).fill_(dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)
    lse = torch.full((p.Hq, p.lay.total_q), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    need = fa.kvcache_decode_d256_workspace_bytes(p.B, p.Hkv, p.G, p.max_q, Ncap=0 if ps else p.Ncap, max_pages=p.Ncap // ps if ps else 0,
                                                  page_size=ps, window=W, num_splits=S)
    assert need == kv.workspace_bytes(p.B, p.Hkv, p.G, p.max_q, S or p.split_count(W)), (need, S, W)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda") if need else None   # fp32 0xFFFFFFFF is a NaN
    o = fa.fa_kvcache_decode_d256(q, kc, vc, _ints(torch, p.lay.cu), p.max_q, cache_seqlens=_ints(torch, p.lens), block_table=table,
                                  causal=bool(causal), scale=scale, window=W, softcap=softcap, out=out, lse=lse, workspace=ws, num_splits=S)
    torch.cuda.synchronize()
    assert o[0] is out and o[1] is lse
    assert (out[free].contiguous().view(torch.int16 if out16 else torch.int32) == (dv.SENTINEL_O16 if out16 else dv.SENTINEL_O32)).all(), \
        "an O row of no sequence was written"
    assert (lse[:, free] == dv.SENTINEL_LSE).all(), "an lse entry of no sequence was written"
    return out, lse


def _host(p, res):
    """-> packed fp32 numpy O (a 16-bit result widened, the 32-bit sentinel in the tokens _launch found untouched) and lse"""
    o = res[0].float().cpu().numpy()
    if res[0].dtype.itemsize == 2:
        o[~p.lay.owned] = np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0]
    return o, res[1].cpu().numpy()


def _same(torch, a, b, what):
    for x, y, n in zip(a, b, ("O", "lse")):
        assert torch.equal(x.view(torch.int16 if x.dtype.itemsize == 2 else torch.int32), y.view(torch.int16 if y.dtype.itemsize == 2 else torch.int32)), \
            f"{what}: {n} differs from the contiguous launch's bits"


def _check(oracle, p, res, want, what, max_abs=None):
    """dv.check's conditions (cm.MAX_ABS, cm.REL_L2, 2 * cm.P_EPS, rows without a key exactly 0 / -inf); max_abs: cm.peaked_tol in the
    place of cm.MAX_ABS, where tests/test_gpu_decode_edges.py::test_scale_kvcache uses it"""
    o, lse = _host(p, res)
    if max_abs is None:
        return dv.check(oracle, p.lay, o, lse, want[0], want[1], p.fmt, what)
    B, fin = p.B, np.isfinite(want[1])
    got, gl = dv.unpack_rows(p.lay, o, B), dv.unpack_rows(p.lay, np.ascontiguousarray(lse.T), B, fill=-np.inf)
    w = np.asarray(want[0], np.float32)
    ma, rl = oracle.max_abs(got, w), oracle.rel_l2(got, w)
    le = float(np.abs(gl[fin] - want[1][fin]).max()) if fin.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {max_abs:.2e} {cm.REL_L2[p.fmt]:.1e} {2 * cm.P_EPS[p.fmt]:.2e})")
    assert np.isfinite(got).all() and not np.isnan(gl).any(), what + ": NaN"
    nokey = dv.live_mask(p.lay, p.Hq) & ~fin
    assert (got[nokey] == 0.0).all() and (gl[nokey] == -np.inf).all(), what + ": a row without a key is not exactly 0 / -inf"
    assert ma <= max_abs and rl <= cm.REL_L2[p.fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert np.isfinite(gl[fin]).all() and le <= 2 * cm.P_EPS[p.fmt], f"{what}: lse off by {le:.3e}"


# ---- A. the key census ------------------------------------------------------------------------------------------------------------------
def _census(p, m, coding, res, causal, W, what):
    """ci.census_check on the padded rows and lse = ln(count) within 2 * P_EPS -> (largest deviation, largest lse error)"""
    S, cnt, m_q = kv.census_expected(p, m, coding, causal, W)
    o, lse = _host(p, res)
    got = dv.unpack_rows(p.lay, o, p.B)
    gl = dv.unpack_rows(p.lay, np.ascontiguousarray(lse.T), p.B, fill=-np.inf)
    dev = ci.census_check(got, S, cnt, m_q, what=what)
    live = cnt > 0
    assert (gl[~live] == -np.inf).all(), what + ": a row without a key has lse != -inf"
    le = float(np.abs(gl[live] - kv.census_lse(cnt)[live]).max())
    assert le <= 2 * cm.P_EPS[p.fmt], f"{what}: lse off ln(count) by {le:.3e}"
    return dev, le


@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("fmt", FMTS)
def test_census(fa, oracle, torch_cuda, fmt, coding):
    """kv.census_launches(): the contiguous launch of every (S, W) against the closed-form sums, the paged launch beside it bit for
    bit; then, for every S, the soft-cap (every score is 0: the weights stay uniform) and the 16-bit output where ci.out16_exact holds"""
    torch = torch_cuda
    p, m = kv.census_problem(oracle, fmt, coding)
    dev, base, worst, worst_lse = {}, {}, 0.0, 0.0
    for S, W, ps, causal in kv.census_launches():
        what = f"census {cm.FMT_NAME[fmt]} {coding} S={S} W={W} pages={ps} causal={causal}"
        res = _launch(fa, torch, p, causal, W, S, ps, dev=dev)
        if ps:
            _same(torch, res, base[S, W, causal], what)
            continue
        base[S, W, causal] = res
        d, le = _census(p, m, coding, res, causal, W, what)
        worst, worst_lse = max(worst, d), max(worst_lse, le)
    count_max = 4 if coding == "residue" else 64
    for i, S in enumerate(kv.CENSUS_S):
        W, causal, ps = kv.CENSUS_W[i % 4], i & 1, kv.CENSUS_PAGES[i % 5]
        what = f"census {cm.FMT_NAME[fmt]} {coding} S={S} W={W} pages={ps} causal={causal}"
        d, le = _census(p, m, coding, _launch(fa, torch, p, causal, W, S, ps, softcap=kv.CENSUS_SOFTCAP, dev=dev), causal, W, what + " softcap")
        worst, worst_lse = max(worst, d), max(worst_lse, le)
        if ci.out16_exact(fmt, count_max):
            d, le = _census(p, m, coding, _launch(fa, torch, p, causal, W, S, ps, out16=True, dev=dev), causal, W, what + " out16")
            worst, worst_lse = max(worst, d), max(worst_lse, le)
    print(f"CENSUS|{ENTRY}|Z {cm.FMT_NAME[fmt]} {coding}|{worst:.3e}|lse {worst_lse:.3e}")


# ---- B. the softmax range ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", MASKS)
@pytest.mark.parametrize("variant", kv.RANGE_VARIANTS)
@pytest.mark.parametrize("fmt", FMTS)
def test_softmax_range(fa, oracle, torch_cuda, fmt, variant, causal):
    """every split count: fp32 and 16-bit output against float64 at sr.bounds, pages of 16 and 256 the contiguous launch's bits"""
    torch = torch_cuda
    p, _ = kv.range_case(oracle, fmt, variant)
    W, softcap = kv.range_options(variant)
    want = kv.range_reference(oracle, fmt, variant, causal)
    dev = {}
    for S in kv.RANGE_SPLITS:
        case = f"{cm.FMT_NAME[fmt]} {variant} causal={int(causal)} S={S}"
        res = _launch(fa, torch, p, causal, W, S, softcap=softcap, scale=kv.SCALE, dev=dev)
        kv.range_check(oracle, p, *_host(p, res), *want, case)
        low = _launch(fa, torch, p, causal, W, S, out16=True, softcap=softcap, scale=kv.SCALE, dev=dev)
        kv.range_check(oracle, p, *_host(p, low), *want, case + " o16", out16=True)
        for ps in kv.RANGE_PAGES:
            _same(torch, _launch(fa, torch, p, causal, W, S, ps, softcap=softcap, scale=kv.SCALE, dev=dev), res, f"{case} pages={ps}")


# ---- C. lengths, rows, scale, the library's split count ---------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", MASKS)
@pytest.mark.parametrize("fmt", FMTS)
def test_length_sweep(fa, oracle, torch_cuda, fmt, causal):
    """di.c_lens() -- 48 lengths on and next to every tile, chunk and page edge, and -1, INT_MIN, 1025, INT_MAX -- with 0 .. max_q + 2
    tokens per sequence, W in {0, 100}, S in {4, 0}; pages of 16 and 256 bit for bit"""
    torch = torch_cuda
    p = kv.sweep_problem(oracle, fmt)
    assert di.length_categories(p.lens, p.Ncap, di.C_SPLITS, di.C_PAGES) >= di.c_categories_wanted(di.C_PAGES)
    dev = {}
    for W in kv.SWEEP_W:
        want = p.reference(causal, W)
        for S in kv.SWEEP_S:
            what = f"length sweep {cm.FMT_NAME[fmt]} causal={int(causal)} W={W} S={S}"
            res = _launch(fa, torch, p, causal, W, S, dev=dev)
            _check(oracle, p, res, want, what)
            for ps in di.C_PAGES:
                _same(torch, _launch(fa, torch, p, causal, W, S, ps, dev=dev), res, f"{what} pages={ps}")


@pytest.mark.parametrize("G,max_q", kv.ROW_CASES)
@pytest.mark.parametrize("fmt", FMTS)
def test_rows(fa, oracle, torch_cuda, fmt, G, max_q):
    """128 rows in four blocks, 35 rows with three in the last block, three rows; lengths 1, 2, 3 below n_b; Ncap = 1000"""
    p = kv.rows_problem(oracle, fmt, G, max_q)
    dev = {}
    for causal in (True, False):
        for W in (0, 70):
            want = p.reference(causal, W)
            for S in (1, 3):
                _check(oracle, p, _launch(fa, torch_cuda, p, causal, W, S, dev=dev), want,
                       f"rows {cm.FMT_NAME[fmt]} G={G} max_q={max_q} causal={int(causal)} W={W} S={S}")


@pytest.mark.parametrize("scale", di.D_SCALES)
@pytest.mark.parametrize("fmt", FMTS)
def test_scale(fa, oracle, torch_cuda, fmt, scale):
    """0.3 (peaked rows: cm.peaked_tol), -0.2 (the sign goes into Q) and 0: every visible key weighs the same -- also under the
    soft-cap and a window, where a masked key must not turn into 0 * -inf"""
    torch = torch_cuda
    p = kv.scale_problem(oracle, fmt)
    tol = cm.peaked_tol(fmt, np.abs(p.v).max()) if scale == 0.3 else None
    options = [(0, 0.0)] + ([(0, kv.SCALE_SOFTCAP), (kv.SCALE_W, 0.0)] if scale == 0.0 else [])
    dev = {}
    for causal in (True, False):
        for W, softcap in options:
            want = p.reference(causal, W, scale, softcap)
            if scale == 0.0:
                uo, ul = cm.uniform_expected(p.v, p.lens, p.B, p.Hkv, p.G, p.max_q, causal, W)
                assert np.abs(want[0] - uo).max() < 1e-6 and np.array_equal(np.isfinite(ul), np.isfinite(want[1]))
            for S in (1, 4):
                what = f"scale={scale} {cm.FMT_NAME[fmt]} causal={int(causal)} W={W} softcap={softcap} S={S}"
                res = _launch(fa, torch, p, causal, W, S, softcap=softcap, scale=scale, dev=dev)
                _check(oracle, p, res, want, what, tol)
                _same(torch, _launch(fa, torch, p, causal, W, S, di.D_PAGE, softcap=softcap, scale=scale, dev=dev), res, what + " pages=16")


@pytest.mark.parametrize("B,lens,W,S_rule", kv.AUTO_CASES, ids=[f"B{B}-W{W}" for B, _, W, _ in kv.AUTO_CASES])
@pytest.mark.parametrize("fmt", FMTS)
def test_automatic_split(fa, oracle, torch_cuda, fmt, B, lens, W, S_rule):
    """num_splits = 0 where the rule gives four splits (and one under a window of 70): the workspace is B * Hkv * S * nqb * 32 * 260 * 4
    bytes, the result matches float64, and its bits are those of the call with that S given"""
    torch = torch_cuda
    p = kv.auto_problem(oracle, fmt, lens)
    need = fa.kvcache_decode_d256_workspace_bytes(p.B, p.Hkv, p.G, p.max_q, Ncap=p.Ncap, window=W, num_splits=0)
    assert need == kv.workspace_bytes(p.B, p.Hkv, p.G, p.max_q, S_rule) and p.split_count(W) == S_rule
    for causal in (True, False):
        auto = _launch(fa, torch, p, causal, W, 0)
        _check(oracle, p, auto, p.reference(causal, W), f"automatic split {cm.FMT_NAME[fmt]} B={B} W={W} causal={int(causal)}")
        _same(torch, _launch(fa, torch, p, causal, W, S_rule), auto, f"num_splits={S_rule}")


# ---- D. base offsets past 2^32 bytes ----------------------------------------------------------------------------------------------------
def _far_check(oracle, torch, o, lse, rows, want, want_lse, fmt, what):
    """the live tokens against float64 (tde._check), every other token exactly 0 / -inf"""
    tde._check(oracle, (o[rows, 0], lse[0, rows]), want, want_lse, fmt, what)
    rest = torch.ones(o.shape[0], dtype=torch.bool, device="cuda")
    rest[rows] = False
    assert bool((o[rest] == 0.0).all()) and bool((lse[0, rest] == -np.inf).all()), what + ": a sequence of length 0 is not exactly 0 / -inf"


def test_heads_past_4g_bytes_contiguous(fa, oracle, torch_cuda):
    """4104 sequences x 4096 keys x 256 (8.6 GB per tensor), uninitialised; heads 2049 and 4097 start just past 2^32 and 2^33 bytes.
    The heads a wrapped offset would land in hold NaN; every other sequence has length 0"""
    torch, f, fmt = torch_cuda, kv.FAR_CONTIG, 0
    B, Ncap = f["B"], f["Ncap"]
    tde._need_memory(torch, 2 * B * Ncap * kv.D * 2 + tde.GIB // 2)
    live, lens_live = [b for b, _ in kv.FAR_CONTIG_LIVE], tuple(L for _, L in kv.FAR_CONTIG_LIVE)
    (q, k, v), (qb, kb, vb) = di.inputs(oracle, len(live), 1, 1, 1, Ncap, kv.D, fmt, 9900)
    want, want_lse = cm.expected_f64(q, k, v, lens_live, len(live), 1, 1, 1, False)
    dk, dv_ = (torch.empty((B, 1, Ncap, kv.D), dtype=torch.float16, device="cuda") for _ in range(2))
    assert dk.numel() * 2 > 2 ** 33
    for t, src in ((dk, kb), (dv_, vb)):
        for b in di.wrap_aliases(live, Ncap * kv.D, B):
            t[b].fill_(float("nan"))
        rows = cm.dev16(torch, cm.poisoned(src[:, None], lens_live), fmt)
        for i, b in enumerate(live):
            t[b].copy_(rows[i])
    dq = torch.randn((B, 1, kv.D), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda").half()
    dq[live] = cm.dev16(torch, qb, fmt).view(len(live), 1, kv.D)
    lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    lens[live] = _ints(torch, lens_live)
    assert fa.kvcache_decode_d256_workspace_bytes(B, 1, 1, 1, Ncap=Ncap) == 0
    o, lse = fa.fa_kvcache_decode_d256(dq, dk, dv_, torch.arange(B + 1, dtype=torch.int32, device="cuda"), 1, cache_seqlens=lens, return_lse=True)
    torch.cuda.synchronize()
    del dk, dv_
    _far_check(oracle, torch, o, lse, live, want, want_lse, fmt, "far heads, contiguous")
    torch.cuda.empty_cache()


def test_pages_past_4g_bytes_paged(fa, oracle, torch_cuda):
    """pools of 32800 pages x 2 heads x 256 keys x 256 (8.6 GB per tensor), uninitialised; two sequences behind four splits whose
    tables name pages just past 2^32 and 2^33 bytes.  The (page, head) units a wrapped offset would land in hold NaN, the dead table
    entries garbage"""
    torch, g, fmt = torch_cuda, kv.FAR_PAGED, 0
    B, Hkv, ps, max_pages, num_pages = g["B"], g["Hkv"], g["ps"], g["max_pages"], g["num_pages"]
    tde._need_memory(torch, 2 * num_pages * Hkv * ps * kv.D * 2 + tde.GIB // 2)
    Ncap = ps * max_pages
    (q, k, v), (qb, kb, vb) = di.inputs(oracle, B, Hkv, 1, 1, Ncap, kv.D, fmt, 9910)
    want, want_lse = cm.expected_f64(q, k, v, kv.FAR_PAGED_LENS, B, Hkv, 1, 1, False)
    kp, vp = (torch.empty((num_pages, Hkv, ps, kv.D), dtype=torch.float16, device="cuda") for _ in range(2))
    assert kp.numel() * 2 > 2 ** 33
    table = np.array([[cm.GARBAGE[i % 2] for i in range(max_pages)] for _ in range(B)], np.int32)
    named = [x for row in kv.FAR_PAGED_TABLE for x in row]
    for pool, src in ((kp, kb), (vp, vb)):
        units = pool.view(num_pages * Hkv, ps, kv.D)
        for u in di.wrap_aliases(kv.far_units(named, Hkv), ps * kv.D, num_pages * Hkv):
            units[u].fill_(float("nan"))
        rows = cm.dev16(torch, cm.poisoned(src.reshape(B, Hkv, Ncap, kv.D), kv.FAR_PAGED_LENS), fmt)   # NaN past the lengths
        for b, entries in enumerate(kv.FAR_PAGED_TABLE):
            for pi, page in enumerate(entries):
                table[b, pi] = page
                pool[page].copy_(rows[b, :, pi * ps:(pi + 1) * ps])
    need = fa.kvcache_decode_d256_workspace_bytes(B, Hkv, 1, 1, max_pages=max_pages, page_size=ps, num_splits=g["S"])
    assert need == kv.workspace_bytes(B, Hkv, 1, 1, g["S"])
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv, kv.D)
    o, lse = fa.fa_kvcache_decode_d256(dq, kp, vp, torch.arange(B + 1, dtype=torch.int32, device="cuda"), 1, cache_seqlens=_ints(torch, kv.FAR_PAGED_LENS),
                                       block_table=torch.from_numpy(table).cuda(), return_lse=True, num_splits=g["S"],
                                       workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    del kp, vp
    tde._check(oracle, (o, lse.T.contiguous()), want, want_lse, fmt, "far pages, paged")
    torch.cuda.empty_cache()
