"""GPU tier of the key census: every entry point on inputs whose result is an integer count in closed form
(tests/census_inputs.py; its CPU tier is tests/test_census_inputs.py).

Family Z (K = 0, V entries 0 or m_h) makes the weights uniform over the keys a row sees, family R (row-constant K, one score per
row) does the same while the pipeline's references, gates and fallback chain see real logits.  O[h, i, col] * c_i / m_h is then the
NUMBER of keys of column col row i added up, and census_check holds it to the closed-form count within 0.25 -- a decision between
neighbouring integers: a key dropped, counted twice, read from another tile or from another head fails it, on every row of every
shape, the full-size ones included (expected values computed on the device).

The decode entries run on the poison of tests/decode_inputs.py and tests/window_inputs.py (NaN behind every length and below every
window's start, in every page no table names and in the workspace), so reading too much shows as a NaN and reading too little as
a count that is short.  Every test prints `CENSUS|entry|family|largest deviation`; profiles/census.txt holds a run's figures.
"""
import os

import numpy as np
import pytest

import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import fp8_inputs as f8
import window_inputs as wi

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
FMTS = [pytest.param(fmt, id=cm.FMT_NAME[fmt]) for fmt in (0, 1)]
_EXPERIMENTAL = (21, 22, 25)   # A/B kernels: only in the experimental library (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _ints(torch, values):
    return torch.tensor(list(values), dtype=torch.int32, device="cuda")


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _algos_for(fa, d):
    """tests/test_gpu_parity.py::_algos_for"""
    have_exp = fa.lib().fa_mi355_has_experiments() == 1
    algos = (0, 1, 2, 5, 6, 21, 22, 23, 24, 25, 26, 27, 29) if d == 64 else ((0, 1, 2, 21, 23, 24, 26, 28) if d == 128 else (0, 1))
    return tuple(a for a in algos if a not in _EXPERIMENTAL or have_exp)


def _causal_algos(d):
    return ci.CAUSAL_ALGOS.get(d, (0, 1))


def _note(entry, family, dev):
    print(f"CENSUS|{entry}|{family}|{dev:.3e}")


def _launches(fa, d, causal):
    return [(algo, causal) for algo in (_causal_algos(d) if causal else _algos_for(fa, d))]


# ---- prefill, family Z ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("d", [64, 128, 16, 32, 256])
@pytest.mark.parametrize("fmt", FMTS)
def test_prefill_zero_k(fa, oracle, torch_cuda, fmt, d, coding):
    """fa_forward without a mask over every algo and under the mask over the algos that implement it, three heads with m = 1, 2, 3:
    N below, at and above a tile, ragged over several row blocks of every kernel; fp32 output."""
    torch = torch_cuda
    worst = 0.0
    for n in ci.Z_PREFILL_N[d]:
        case = ci.z_prefill(oracle, ci.Z_BH, n, d, fmt, coding)
        dq, dk, dv = (cm.dev16(torch, x, fmt) for x in case["bits"])
        for causal in (False, True):
            lo, c = ci.prefill_limits(n, causal)
            S = ci.expected_sums_torch(torch, case["m"], lo, c, n, d, coding, "cuda")
            for algo, _ in _launches(fa, d, causal):
                o = fa.fa_forward(dq, dk, dv, algo=algo, causal=causal)
                torch.cuda.synchronize()
                worst = max(worst, ci.census_check(o, S, torch.as_tensor(c - lo), case["m"],
                                                   what=f"fa_forward Z n={n} d={d} {cm.FMT_NAME[fmt]} {coding} algo={algo} causal={causal}"))
    _note("fa_forward", "Z", worst)


@pytest.mark.parametrize("fmt", FMTS)
def test_prefill_zero_k_16bit_output(fa, oracle, torch_cuda, fmt):
    """the short shape with 16-bit output, in the codings the exactness rule admits for the format"""
    torch = torch_cuda
    n, d, bh = ci.Z_OUT16["n"], ci.Z_OUT16["d"], ci.Z_OUT16["bh"]
    worst = 0.0
    for coding in ci.out16_codings(fmt):
        case = ci.z_prefill(oracle, bh, n, d, fmt, coding)
        dq, dk, dv = (cm.dev16(torch, x, fmt) for x in case["bits"])
        for causal in (False, True):
            lo, c = ci.prefill_limits(n, causal)
            S = ci.expected_sums_torch(torch, case["m"], lo, c, n, d, coding, "cuda")
            assert ci.out16_exact(fmt, ci.max_count(lo, c, n, d, coding))
            for algo, _ in _launches(fa, d, causal):
                o = fa.fa_forward(dq, dk, dv, algo=algo, causal=causal, out_dtype=_tdtype(torch, fmt))
                torch.cuda.synchronize()
                assert o.dtype == _tdtype(torch, fmt)
                worst = max(worst, ci.census_check(o, S, torch.as_tensor(c - lo), case["m"],
                                                   what=f"fa_forward Z out16 {cm.FMT_NAME[fmt]} {coding} algo={algo} causal={causal}"))
    _note("fa_forward out16", "Z", worst)


# ---- the persistent grid: all rows, expected values on the device ----------------------------------------------------------------------
def _grid_inputs(torch, bh, n, d, fmt, coding, seed):
    """family Z on the device: Q random (its values cannot matter: K = 0), V coded with m_h = (h % 8) + 1 -- neighbouring items of
    the persistent grid carry different values"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = ci.head_values(bh, "Z")
    q = torch.randn(bh, n, d, generator=g, device="cuda").to(_tdtype(torch, fmt))
    return q, torch.zeros_like(q), ci.v_coded_torch(torch, m, n, d, coding, _tdtype(torch, fmt), "cuda"), m


def _grid_check(fa, torch, q, k, v, m, n, d, coding, causal, algos, what):
    lo, c = ci.prefill_limits(n, causal)
    S = ci.expected_sums_torch(torch, m, lo, c, n, d, coding, "cuda")
    worst = 0.0
    for algo in algos:
        o = fa.fa_forward(q, k, v, algo=algo, causal=causal)
        torch.cuda.synchronize()
        worst = max(worst, ci.census_check(o.view(S.shape), S, torch.as_tensor(c - lo), m, what=f"{what} algo={algo}"))
        del o
    return worst


@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("bh,n,d", ci.GRID_CAUSAL, ids=[f"bh{b}-n{n}-d{d}" for (b, n, d) in ci.GRID_CAUSAL])
@pytest.mark.parametrize("fmt", FMTS)
def test_causal_grid_all_rows(fa, torch_cuda, fmt, bh, n, d, coding):
    """more causal items than CUs (the item order of tests/test_gpu_parity.py::test_causal_large_grid_item_order), every row"""
    torch = torch_cuda
    q, k, v, m = _grid_inputs(torch, bh, n, d, fmt, coding, 9000 + bh)
    _note("fa_forward causal grid", "Z", _grid_check(fa, torch, q, k, v, m, n, d, coding, True, ci.GRID_ALGOS,
                                                     f"causal grid bh={bh} n={n} d={d} {cm.FMT_NAME[fmt]} {coding}"))


@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("fmt", FMTS)
def test_bench_shape_all_rows(fa, torch_cuda, fmt, coding):
    """B8 H16 N4096 d64 without a mask, through the dispatcher and the folded pipeline by name: all 524288 rows"""
    torch = torch_cuda
    g = ci.GRID_BENCH
    bh, n, d = g["B"] * g["H"], g["n"], g["d"]
    q, k, v, m = _grid_inputs(torch, bh, n, d, fmt, coding, 9100)
    q, k, v = (x.view(g["B"], g["H"], n, d) for x in (q, k, v))
    _note("fa_forward bench shape", "Z", _grid_check(fa, torch, q, k, v, m, n, d, coding, False, ci.GRID_ALGOS,
                                                     f"bench shape {cm.FMT_NAME[fmt]} {coding}"))


@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("fmt", FMTS)
def test_one_wave_grid_all_rows(fa, torch_cuda, fmt, coding):
    """BH = CUs // 8 heads of 8192 rows at d = 128 through the one-wave-per-SIMD kernel (algo 28)"""
    torch = torch_cuda
    g = ci.GRID_1W
    bh = max(torch.cuda.get_device_properties(0).multi_processor_count // 8, 2)
    q, k, v, m = _grid_inputs(torch, bh, g["n"], g["d"], fmt, coding, 9200)
    _note("fa_forward one-wave grid", "Z", _grid_check(fa, torch, q, k, v, m, g["n"], g["d"], coding, False, (g["algo"],),
                                                       f"one-wave grid bh={bh} {cm.FMT_NAME[fmt]} {coding}"))


# ---- the fallback chain, family R -------------------------------------------------------------------------------------------------------
_exp_lib = None


def _exp():
    """the experimental library (build() makes it): the product's kernels plus fa_lab_rp16_pass_ids"""
    global _exp_lib
    if _exp_lib is None:
        import ctypes as C
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


def _pass_id_set(torch, q, k, v, algo, causal):
    """The pass ids one head's row blocks were produced by (0 folded, 1 exact optimistic, 2 running max in the kernel, 3 the redo
    list), as a set: the head is launched alone, so the size of a kernel's row block need not be known -- the array has one entry
    per 16 rows and the entries no workgroup wrote keep 255."""
    L = _exp()
    n, d = q.shape
    ids = torch.full(((n + 15) // 16,), 255, dtype=torch.int32, device="cuda")
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    assert L.fa_lab_rp16_pass_ids(ids.data_ptr()) == 0
    try:
        fn = L.fa_forward_causal if causal else L.fa_forward_ex
        rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, 1, n, d, 1.0 / d ** 0.5,
                0 if q.dtype == torch.float16 else 1, 0, algo, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
    finally:
        assert L.fa_lab_rp16_pass_ids(None) == 0
    return set(int(x) for x in ids.cpu().numpy() if x != 255), out


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_fallback_chain_row_constant_k(fa, oracle, torch_cuda, fmt, d, causal):
    """Family R through the pipeline's widths: head 0 stays in the folded pass, head 1 is refused by the row-sum gates and kept by
    the exact pass, head 2 (fp16) goes straight to the running-max pass -- in the kernel on the narrow widths, through the redo
    list on the full one.  Every pass must count every key once; the pass ids show that the passes named here are the ones that ran."""
    torch = torch_cuda
    algos = ci.R_CAUSAL_ALGOS[d] if causal else ci.R_ALGOS[d]
    reached = {a: set() for a in algos}
    worst = 0.0
    for n in ci.R_SHAPES[d, fmt]:
        lo, c = ci.prefill_limits(n, causal)
        for coding in ci.r_codings(fmt):
            case = ci.r_case(oracle, n, d, fmt, coding)
            for wave in (ci.WAVE_ROWS[d], ci.WAVE_ROWS[d] // 2, 16):
                ci.assert_regimes(case, d, fmt, causal, wave)
            assert ci.r_exact(fmt, ci.max_count(lo, c, n, d, coding))
            dq, dk, dv = (cm.dev16(torch, x, fmt) for x in case["bits"])
            S = ci.expected_sums_torch(torch, case["m"], lo, c, n, d, coding, "cuda")
            for algo in algos:
                what = f"fa_forward R n={n} d={d} {cm.FMT_NAME[fmt]} {coding} algo={algo} causal={causal}"
                o = fa.fa_forward(dq, dk, dv, algo=algo, causal=causal)
                torch.cuda.synchronize()
                worst = max(worst, ci.census_check(o, S, torch.as_tensor(c - lo), case["m"], what=what))
                per_head = []
                for h in range(3):
                    ids, o_exp = _pass_id_set(torch, dq[h], dk[h], dv[h], algo, causal)
                    # (the head alone, in the experimental library: the launch the ids are read from must count right as well)
                    ci.census_check(o_exp[None], S[h:h + 1], torch.as_tensor(c - lo), case["m"][h:h + 1], what=what + f" head {h} alone")
                    per_head.append(ids)
                    reached[algo] |= ids
                print(f"{what}: pass ids per head {per_head}")
                if algo == 23:       # the exact kernel: its optimistic pass keeps a row-constant K whatever the score
                    assert per_head == [{1}, {1}, {1}], (what, per_head)
                    continue
                assert per_head[0] == {0} and per_head[1] == {1}, (what, per_head)
                if fmt == 0:
                    assert per_head[2] and per_head[2] <= {2, 3}, (what, per_head)
                    if algo in ci.R_HALF_WIDTH:
                        assert per_head[2] == {2}, (what, per_head)
                    else:            # the full-width kernels (24, and 28 at d = 128): the redo list
                        assert per_head[2] == {3}, (what, per_head)
                else:                # bf16 weights cannot overflow in the exact pass: it is tried first
                    assert per_head[2] == {1}, (what, per_head)
    _note("fa_forward fallback chain", "R", worst)
    if fmt == 0:
        for algo in algos:
            if algo != 23:
                assert ({0, 1, 2} if algo in ci.R_HALF_WIDTH else {0, 1, 3}) <= reached[algo], reached


# ---- decode, family Z -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_splitkv_zero_k(fa, oracle, torch_cuda, fmt, d, coding):
    """fa_forward_splitkv: one pass with a ragged last tile (5 x 100), 26 splits and the merge (3 x 8229), two row blocks (130 x 777)"""
    torch = torch_cuda
    worst = 0.0
    for (nq, nk) in ci.SPLITKV:
        (_, _, _), (qb, _, _) = oracle.make_qkv(2, nq, d, fmt=fmt, seed=9300 + nk)
        m = ci.head_values(2, "Z")
        v = ci.v_coded(m, nk, d, coding)
        S = ci.expected_sums(m, np.zeros(nq, np.int64), np.full(nq, nk, np.int64), nk, d, coding)
        assert ci.z_exact(fmt, S.max())
        need = fa.splitkv_workspace_bytes(1, 2, nq, nk, d)
        dq = cm.dev16(torch, qb[None], fmt)
        dv = cm.dev16(torch, oracle.encode16(v, fmt)[None], fmt)
        o = fa.fa_forward_splitkv(dq, torch.zeros_like(dv), dv, workspace=_nan_workspace(torch, need))
        torch.cuda.synchronize()
        worst = max(worst, ci.census_check(o.cpu().numpy().reshape(S.shape), S, np.full(nq, nk), m,
                                           what=f"splitkv Z nq={nq} nk={nk} d={d} {cm.FMT_NAME[fmt]} {coding}"))
    _note("fa_forward_splitkv", "Z", worst)


K_SCALE, V_SCALES = 3.0, (None, 0.5)   # fp8: any k_scale leaves a zero score zero; v_scale multiplies the count


def _cache_run(fa, torch, dq, kc, vc, lens, W, causal, fmt, ps=0, seed=0, v_scale=None):
    """kc, vc [B, Hkv, Ncap, d] poisoned for (lens, W): uint16 encodings (16-bit entries) or uint8 codes (fp8 entries, with
    k_scale = K_SCALE and the given v_scale).  ps = 0: the contiguous entry, else the paged one on cm.scatter's pool (W = 0: no
    start, no dead pages).  W = 0 is the base entries' call, W > 0 the windowed ones', both through fa_kvcache_decode.  -> O, lse"""
    B, Hq, Nq, d = dq.shape
    Hkv, Ncap = kc.shape[1], kc.shape[2]
    G = Hq // Hkv
    fp8 = kc.dtype == np.uint8
    need = fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W) if W else fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    kw = dict(cache_seqlens=_ints(torch, lens), causal=causal, return_lse=True, workspace=_nan_workspace(torch, need), window=W)
    if fp8:
        kw.update(k_scale=torch.full((Hkv,), K_SCALE, dtype=torch.float32, device="cuda"),
                  v_scale=None if v_scale is None else torch.full((Hkv,), v_scale, dtype=torch.float32, device="cuda"))
    if ps == 0:
        o, lse = (fa.fa_forward_kvcache_fp8 if fp8 else fa.fa_forward_kvcache)(dq, dev(kc), dev(vc), **kw)
    else:
        kp, vp, table = cm.scatter(kc, vc, lens, ps, seed, Nq, W, nan=wi.NAN8 if fp8 else cm.NAN16)
        o, lse = (fa.fa_forward_kvcache_paged_fp8 if fp8 else fa.fa_forward_kvcache_paged)(
            dq, dev(kp), dev(vp), torch.from_numpy(table).cuda(), **kw)
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and o.dtype == torch.float32 and lse.dtype == torch.float32
    return o, lse


def _cache_check(o, lse, S, cnt, m_q, fmt, what, v_scale=1.0):
    """census_check of O, and lse = ln(number of keys) within the decode tier's bound, -inf for a row without a key"""
    dev = ci.census_check(o.cpu().numpy().reshape(S.shape), S, cnt, m_q, v_scale=v_scale, what=what)
    got = lse.cpu().numpy().reshape(cnt.shape).astype(np.float64)
    live = cnt > 0
    assert not np.isnan(got).any(), what + ": NaN in lse"
    assert (got[~live] == -np.inf).all(), what + ": a row without a key has lse != -inf"
    le = float(np.abs(got[live] - np.log(cnt[live])).max()) if live.any() else 0.0
    assert le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"
    return dev


def _cache_entries(fa, oracle, torch, shape, lens, d, fmt, coding, W, causal, pages, what):
    """one launch configuration through the four entries: contiguous, paged (bit-equal), fp8 (v_scale None and 0.5), paged fp8
    (every page size, bit-equal to contiguous fp8) -> {entry: largest deviation}"""
    B, Hkv, G, Nq, Ncap = shape
    case = ci.z_decode(oracle, B, Hkv, G, Nq, Ncap, d, fmt, coding)
    qb, kb, vb = case["bits"]
    lo, c = ci.decode_limits(lens, B, Hkv, G, Nq, Ncap, causal, W)
    S, m_q = ci.decode_sums(case["m"], lo, c, G, Ncap, d, coding)
    cnt = c - lo
    assert ci.z_exact(fmt, S.max())
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    out = {}
    kc, vc = (cm.poisoned(x.reshape(B, Hkv, Ncap, d), lens, Nq, W) for x in (kb, vb))
    o, lse = _cache_run(fa, torch, dq, kc, vc, lens, W, causal, fmt)
    out["kvcache"] = _cache_check(o, lse, S, cnt, m_q, fmt, what + " contiguous")
    for ps in pages:
        po, plse = _cache_run(fa, torch, dq, kc, vc, lens, W, causal, fmt, ps=ps, seed=ps + d + W)
        assert torch.equal(po, o) and torch.equal(plse, lse), f"{what}: pages of {ps}: not the contiguous entry's bits"
    out["kvcache_paged"] = out["kvcache"]
    k8, v8 = (f8.encode(x).reshape(B, Hkv, Ncap, d) for x in (case["k"], case["v"]))
    assert np.array_equal(f8.decode(v8).reshape(case["v"].shape), case["v"]) and not k8.any()   # the codes hold the values exactly
    k8, v8 = cm.poisoned(k8, lens, Nq, W, nan=wi.NAN8), cm.poisoned(v8, lens, Nq, W, nan=wi.NAN8)
    for vs in V_SCALES:
        o8, lse8 = _cache_run(fa, torch, dq, k8, v8, lens, W, causal, fmt, v_scale=vs)
        dev = _cache_check(o8, lse8, S, cnt, m_q, fmt, what + f" fp8 v_scale={vs}", v_scale=1.0 if vs is None else vs)
        out["kvcache_fp8"] = max(out.get("kvcache_fp8", 0.0), dev)
        for ps in pages:
            po, plse = _cache_run(fa, torch, dq, k8, v8, lens, W, causal, fmt, ps=ps, seed=ps + d + W + 1, v_scale=vs)
            assert torch.equal(po, o8) and torch.equal(plse, lse8), f"{what}: fp8 pages of {ps}: not the contiguous fp8 entry's bits"
    out["kvcache_paged_fp8"] = out["kvcache_fp8"]
    return out


@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_cache_entries_zero_k(fa, oracle, torch_cuda, fmt, d, causal, coding):
    """the lengths of tests/decode_inputs.py's scale case (0, 2, 66, 200, 1024, 1, 513, 777; S = 4, three rows, two query heads per
    K/V head) through fa_forward_kvcache, _paged (pages of 16 and 256), _fp8 and _paged_fp8"""
    shape = tuple(di.D_SHAPE[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
    devs = _cache_entries(fa, oracle, torch_cuda, shape, di.D_LENS, d, fmt, coding, 0, causal, (di.D_PAGE, 256),
                          f"cache Z d={d} {cm.FMT_NAME[fmt]} {coding} causal={causal}")
    for entry, dev in devs.items():
        _note("fa_forward_" + entry, "Z", dev)


WINDOW_LAUNCHES = [pytest.param(name, W, causal, id=f"{name}-W{W}-{'causal' if causal else 'full'}")
                   for name, c in wi.CASES.items() for W in c["windows"] for causal in c["causal"]]


@pytest.mark.parametrize("name,W,causal", WINDOW_LAUNCHES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_window_entries_zero_k(fa, oracle, torch_cuda, fmt, d, name, W, causal):
    """every windowed launch of tests/window_inputs.py on all four entries: the lower edge is exact for every row -- rows with
    different lower limits in one tile (rows, W = 3) and the split case (W = 1024) among them"""
    case = wi.CASES[name]
    shape = tuple(case[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
    for coding in ci.CODINGS:
        devs = _cache_entries(fa, oracle, torch_cuda, shape, case["lens"], d, fmt, coding, W, causal, wi.PAGES,
                              f"window Z {name} W={W} d={d} {cm.FMT_NAME[fmt]} {coding} causal={causal}")
        for entry, dev in devs.items():
            _note("fa_forward_" + entry + "_window", "Z", dev)
