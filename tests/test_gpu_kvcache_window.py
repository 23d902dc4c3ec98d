"""GPU tier of the sliding-window decode entries (fa_forward_kvcache_window, _paged_window, _fp8_window, _paged_fp8_window).

Inputs, references and the restated range arithmetic are tests/window_inputs.py's (its CPU tier is tests/test_window_inputs.py).
Oracle parity has the method and the bounds of tests/test_gpu_kvcache_paged.py: expected O from oracle.forward_cross on the keys
[lo_i, c_i) a row sees, expected log-sum-exps from float64 numpy; the project's max-abs bar and relative-L2 bounds for O,
2 * P_EPS absolute for the log-sum-exp.  The bit-equality checks carry the base entries' guarantees over: paged == contiguous,
fp8 with scales of 1 == 16 bit on the widened cache, and the ties to the unwindowed entries the header promises.

Poison: the workspace is filled with NaN bytes; every cache row at or past L_b AND every row below start_b (row 0's lower limit)
holds NaN bit patterns; every pool page no table names holds NaN; every table entry past the last live page or wholly below start_b
holds garbage.  An over-read shows as a non-finite result, not as a fault.
"""
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import flat_entries as flat
import fp8_inputs as f8
import window_inputs as wi

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
LAUNCHES = [pytest.param(name, W, causal, id=f"{name}-W{W}-{'causal' if causal else 'full'}")
            for name, c in wi.CASES.items() for W in c["windows"] for causal in c["causal"]]
FP8_LAUNCHES = [p for p in LAUNCHES if p.values[0] in ("one_pass", "split")]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _ints(torch, values):
    return torch.tensor(list(values), dtype=torch.int32, device="cuda")


def _scales(torch, values):
    return None if values is None else torch.tensor(list(values), dtype=torch.float32, device="cuda")


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _shape(c):
    return tuple(c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))


def _run(fa, torch, dq, kc, vc, lens, W, causal, ps=0, seed=0, scale=None, fmt=None, k_scale=None, v_scale=None, want_S=None):
    """kc, vc: caches [B, Hkv, Ncap, d], poisoned for (lens, W): uint16 encodings (fmt given) or uint8 fp8 codes (fmt None).
    ps = 0: the contiguous windowed entry; else the paged one on the caches scattered into pages of ps keys under the window's
    contract (dead pages below the start are not in the pool, their table entries hold garbage).  -> O, lse (device tensors)"""
    B, Hq, Nq, d = dq.shape
    Hkv, Ncap = kc.shape[1], kc.shape[2]
    fp8 = fmt is None
    need = fa.kvcache_window_workspace_bytes(B, Hkv, Hq // Hkv, Nq, Ncap, d, W)
    if want_S is not None:
        assert di.splits_of(need, B * Hkv, (Hq // Hkv) * Nq, d) == want_S
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    kw = dict(cache_seqlens=_ints(torch, lens), causal=causal, scale=scale, return_lse=True, workspace=_nan_workspace(torch, need),
              window=W)
    if fp8:
        kw.update(k_scale=_scales(torch, k_scale), v_scale=_scales(torch, v_scale))
    if ps == 0:
        o, lse = (fa.fa_forward_kvcache_fp8 if fp8 else fa.fa_forward_kvcache)(dq, dev(kc), dev(vc), **kw)
    else:
        assert fa.kvcache_paged_window_workspace_bytes(B, Hkv, Hq // Hkv, Nq, Ncap // ps, ps, d, W) == need
        kp, vp, table = cm.scatter(kc, vc, lens, ps, seed, Nq, W, nan=wi.NAN8 if fp8 else cm.NAN16)
        o, lse = (fa.fa_forward_kvcache_paged_fp8 if fp8 else fa.fa_forward_kvcache_paged)(
            dq, dev(kp), dev(vp), torch.from_numpy(table).cuda(), **kw)
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o, lse


def _check(oracle, o, lse, want, want_lse, fmt, what):
    cm.check_decode(oracle, o.float().cpu().numpy().reshape(want.shape), lse.cpu().numpy().reshape(want_lse.shape), want, want_lse, fmt, what)


# ---- 1 - 4. oracle parity of the contiguous entry; the paged entry returns its bits ---------------------------------------------------
@pytest.mark.parametrize("name,W,causal", LAUNCHES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_oracle_parity_and_paged_bits(fa, oracle, torch_cuda, fmt, d, name, W, causal):
    """Cases 1 to 3 of tests/window_inputs.py (one pass; split and merge with a start inside a tile, a sequence shorter than the
    window and empty splits; several rows on folded heads under both masks) through fa_forward_kvcache_window against the oracle,
    and through fa_forward_kvcache_paged_window with pages of 16 and 256 keys: the same bits, O and lse."""
    torch = torch_cuda
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    _, (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    want, want_lse = wi.reference(oracle, name, d, fmt, W, causal)
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    kc, vc = (cm.poisoned(x.reshape(B, Hkv, Ncap, d), c["lens"], Nq, W) for x in (kb, vb))
    o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, fmt=fmt, want_S=c["S"])
    _check(oracle, o, lse, want, want_lse, fmt, f"window {name} W={W} causal={causal} d={d} fmt={fmt}")
    for ps in wi.PAGES:
        po, plse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, ps=ps, seed=ps + d + W, fmt=fmt)
        assert torch.equal(po, o) and torch.equal(plse, lse), f"pages of {ps}: not the contiguous entry's bits"


# ---- 5. fp8 -----------------------------------------------------------------------------------------------------------------------------
K_MULT, V_MULT = (1.0, 6.0), (6.0, 1.0)   # per-head scales 6x apart, in opposite order for K and V: a wrong head index shows


@functools.lru_cache(maxsize=None)
def _quantised(fa, oracle, name, d, fmt):
    """tests/test_gpu_kvcache_fp8.py::_quantised_inputs for a case: K and V quantised with fa.quantize_kv_fp8 on the helper's own
    scales times K_MULT / V_MULT.  -> q fp32, q encodings, K and V codes [B, Hkv, Ncap, d], the fp32 values decode(code) * scale[h]
    as [B*Hkv, Ncap, d], and the scale vectors."""
    import torch
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    (q, k, v), (qb, _, _) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    out = []
    for x, mult in ((k, K_MULT), (v, V_MULT)):
        x4 = torch.from_numpy(x.reshape(B, Hkv, Ncap, d).copy())
        _, s0 = fa.quantize_kv_fp8(x4)
        s = (s0 * torch.tensor([mult[h % 2] for h in range(Hkv)])).contiguous()
        x8, _ = fa.quantize_kv_fp8(x4, scale=s)
        codes = x8.view(torch.uint8).numpy().copy()
        assert not np.isin(codes, f8.NAN_CODES).any()
        deq = (f8.decode(codes) * s.numpy().reshape(1, Hkv, 1, 1)).astype(np.float32).reshape(B * Hkv, Ncap, d)
        for a in (codes, deq):
            a.setflags(write=False)
        out.append((codes, deq, tuple(float(t) for t in s)))
    (k8, kd, ks), (v8, vd, vs) = out
    return q, qb, k8, v8, kd, vd, ks, vs


@pytest.mark.parametrize("name,W,causal", FP8_LAUNCHES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_fp8_window(fa, oracle, torch_cuda, fmt, d, name, W, causal):
    """Cases 1 and 2 on a quantize_kv_fp8 cache through fa_forward_kvcache_fp8_window and _paged_fp8_window (pages of 16).  With all
    scales 1 (NULL): the bits of the 16-bit windowed entry on the widened cache (softmax scale 2^-7 / sqrt(d): the codes reach
    448).  With per-head scales: within the bounds of the oracle on the dequantised cache."""
    torch = torch_cuda
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    q, qb, k8, v8, kd, vd, ks, vs = _quantised(fa, oracle, name, d, fmt)
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    pk, pv = cm.poisoned(k8, c["lens"], Nq, W, nan=wi.NAN8), cm.poisoned(v8, c["lens"], Nq, W, nan=wi.NAN8)
    # the widened caches: torch's CPU conversion of the poisoned codes (0x7F widens to a NaN), as 16-bit encodings
    wide = [torch.from_numpy(x).view(torch.float8_e4m3fn).to(_tdtype(torch, fmt)).view(torch.int16).numpy().view(np.uint16) for x in (pk, pv)]
    sc = 2.0 ** -7 / np.sqrt(d)
    base, base_lse = _run(fa, torch, dq, wide[0], wide[1], c["lens"], W, causal, scale=sc, fmt=fmt, want_S=c["S"])
    assert torch.isfinite(base).all() and not torch.isnan(base_lse).any()
    want, want_lse = cm.expected(oracle, q, kd, vd, c["lens"], B, Hkv, G, Nq, causal, W)
    for ps in (0, 16):
        o, lse = _run(fa, torch, dq, pk, pv, c["lens"], W, causal, ps=ps, seed=ps + d, scale=sc, want_S=c["S"])
        assert torch.equal(o, base) and torch.equal(lse, base_lse), f"fp8 layout {ps}: not the 16-bit windowed entry's bits"
        o, lse = _run(fa, torch, dq, pk, pv, c["lens"], W, causal, ps=ps, seed=ps + d + 1, k_scale=ks, v_scale=vs)
        _check(oracle, o, lse, want, want_lse, fmt, f"fp8 window {name} W={W} layout={ps} d={d} fmt={fmt}")


# ---- 6. exact ties to the existing entries ------------------------------------------------------------------------------------------
def _raw_window(fa, torch, dq, dk, dv, dl, W, causal, fmt, need):
    """fa_forward_kvcache_window called through the C ABI as it is, window = 0 included (the Python front end goes through
    fa_kvcache_decode)"""
    return flat.decode(fa, torch, dq, dk, dv, dl, causal, fmt, _nan_workspace(torch, need), window=W)


@pytest.mark.parametrize("name", ["split", "rows"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_no_window_and_full_window_are_the_base_entry(fa, oracle, torch_cuda, fmt, d, name):
    """W = 0 through the C entry, and W = Ncap (same S, start_b = 0): the bits of fa_forward_kvcache, O and lse, under both masks."""
    torch = torch_cuda
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    _, (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    kc, vc = (cm.poisoned(x.reshape(B, Hkv, Ncap, d), c["lens"]) for x in (kb, vb))
    dk, dv, dl = cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), _ints(torch, c["lens"])
    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    assert need > 0 and fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, Ncap) == need
    for causal in (False, True):
        base, base_lse = fa.fa_forward_kvcache(dq, dk, dv, dl, causal=causal, return_lse=True, workspace=_nan_workspace(torch, need))
        torch.cuda.synchronize()
        assert torch.isfinite(base).all() and not torch.isnan(base_lse).any()
        o, lse = _raw_window(fa, torch, dq, dk, dv, dl, 0, causal, fmt, need)
        assert torch.equal(o, base) and torch.equal(lse, base_lse), f"W = 0, causal={causal}"
        o, lse = fa.fa_forward_kvcache(dq, dk, dv, dl, causal=causal, return_lse=True, workspace=_nan_workspace(torch, need), window=Ncap)
        torch.cuda.synchronize()
        assert torch.equal(o, base) and torch.equal(lse, base_lse), f"W = Ncap, causal={causal}"


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_window_is_the_base_entry_on_the_shifted_cache(fa, oracle, torch_cuda, fmt, d):
    """Nq = 1, W = 1024, Ncap = 4096, lengths with (L - W) % 64 == 0: the windowed result EQUALS fa_forward_kvcache on a cache of
    capacity W + 64 that holds cache[L - W : L] at length W -- both stream the same 16 tiles with the same S, chunk, rotation and
    order.  This is what pins the split rule to the one the header states."""
    torch = torch_cuda
    s = wi.SHIFT
    B, Hkv, G, Nq, Ncap, W = s["B"], s["Hkv"], s["G"], s["Nq"], s["Ncap"], s["W"]
    _, (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, s["seed"])
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    kc, vc = (cm.poisoned(x.reshape(B, Hkv, Ncap, d), s["lens"], Nq, W) for x in (kb, vb))
    o, lse = _run(fa, torch, dq, kc, vc, s["lens"], W, False, fmt=fmt, want_S=4)
    small = []
    for src in (kc, vc):
        x = np.full((B, Hkv, W + 64, d), cm.NAN16, np.uint16)
        for b, L in enumerate(s["lens"]):
            x[b, :, :W] = src[b, :, L - W:L]
        small.append(cm.dev16(torch, x, fmt))
    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, W + 64, d)
    assert need == fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W) and di.splits_of(need, B * Hkv, 1, d) == 4
    base, base_lse = fa.fa_forward_kvcache(dq, small[0], small[1], _ints(torch, [W] * B), return_lse=True,
                                           workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert torch.isfinite(base).all() and torch.isfinite(base_lse).all()
    assert torch.equal(o, base) and torch.equal(lse, base_lse)


# ---- 7. graph -------------------------------------------------------------------------------------------------------------------------
def test_captured_append_then_windowed_decode(fa, oracle, torch_cuda):
    """append(seqlens_out == seqlens_k) -> decode with a window of 60, captured once (a linear graph) and replayed over nine steps
    that take sequence 0 from 58 keys across L = W and across the tile edge at 64; every step matches the oracle on the keys the
    row must see."""
    torch = torch_cuda
    g = wi.GRAPH
    B, Hkv, G, Ncap, W, steps, fmt, d = g["B"], g["Hkv"], g["G"], g["Ncap"], g["W"], g["steps"], 0, 64
    (q, k, v), (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, steps, Ncap, d, fmt, g["seed"])
    kb4, vb4, qb4 = kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), qb.reshape(B, Hkv * G, steps, d)
    lens = list(g["start"])
    # the cache holds the drawn rows below the start lengths and NaN above; step t appends the drawn row at each sequence's length
    dk, dv = (cm.dev16(torch, cm.poisoned(x, lens), fmt) for x in (kb4, vb4))
    dl = _ints(torch, lens)

    def new_rows(t):
        rows = [np.stack([src[b, :, lens[b] + t:lens[b] + t + 1] for b in range(B)]) for src in (kb4, vb4)]
        return cm.dev16(torch, rows[0], fmt), cm.dev16(torch, rows[1], fmt), cm.dev16(torch, qb4[:, :, t:t + 1], fmt)

    need = fa.kvcache_window_workspace_bytes(B, Hkv, G, 1, Ncap, d, W)
    ws = _nan_workspace(torch, need)

    def step(dkn, dvn, dq, ck, cv, cl):
        fa.fa_kvcache_append(dkn, dvn, ck, cv, cache_seqlens=cl, seqlens_out=cl)
        return fa.fa_forward_kvcache(dq, ck, cv, cl, causal=True, return_lse=True, workspace=ws, window=W)

    dkn, dvn, dq = new_rows(0)
    step(dkn, dvn, dq, dk.clone(), dv.clone(), dl.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(dkn, dvn, dq, dk, dv, dl)
    assert dl.tolist() == lens   # a capture runs nothing
    for t in range(steps):
        a, b, c = new_rows(t)
        dkn.copy_(a), dvn.copy_(b), dq.copy_(c)
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        now = [L + t + 1 for L in lens]
        assert dl.tolist() == now
        qt = np.ascontiguousarray(q.reshape(B * Hkv * G, steps, d)[:, t:t + 1])
        want, want_lse = cm.expected(oracle, qt, k, v, now, B, Hkv, G, 1, True, W)
        _check(oracle, o, lse, want, want_lse, fmt, f"graph step {t} lengths {now}")


# ---- 8. scale 0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,causal", [p for p in LAUNCHES if p.values[0] == "rows"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_scale_zero(fa, oracle, torch_cuda, fmt, d, name, W, causal):
    """scale = 0 under a window: every key in [lo_i, c_i) weighs the same, so O is the mean of those V rows and lse = ln(their
    number); a masked -inf must not meet the 0 (the host rule of fa_dispatch.hpp), below the window as above it."""
    torch = torch_cuda
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    (_, _, v), (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    want, want_lse = cm.uniform_expected(v, c["lens"], B, Hkv, G, Nq, causal, W)
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    kc, vc = (cm.poisoned(x.reshape(B, Hkv, Ncap, d), c["lens"], Nq, W) for x in (kb, vb))
    for scale in (0.0, -0.0):
        for ps in (0, 16):
            o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, ps=ps, seed=3, scale=scale, fmt=fmt)
            _check(oracle, o, lse, want.astype(np.float32), want_lse, fmt, f"scale {scale} W={W} causal={causal} layout={ps} d={d} fmt={fmt}")
