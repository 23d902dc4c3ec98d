"""GPU tier of attention sinks and soft-capped logits on KV-cache decode: fa_kvcache_decode behind the `sinks` and `softcap` keywords
of the four decode front ends, and the descriptor entry itself.

Inputs, the float64 reference and the sink census are tests/logit_inputs.py's (its CPU tier, tests/test_logit_inputs.py, shows that
no parity launch here passes on a kernel that ignores the feature); shapes and poison are tests/window_inputs.py's.  Bounds are the
project's, applied as tests/test_gpu_kvcache_window.py::_check applies them: the max-abs bar and the relative-L2 bounds for O,
2 * P_EPS absolute for the log-sum-exp; a row without a key gets exact zeros, and lse = -inf without a sink, lse = a with one.

Poison: the workspace is filled with NaN bytes; every cache row at or past L_b and every row below start_b holds NaN bit patterns;
every pool page no table names holds NaN; every dead table entry holds garbage.
"""
import ctypes
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import flat_entries as flat
import fp8_inputs as f8
import logit_inputs as li
import window_inputs as wi

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
LAUNCHES = [pytest.param(*x, id=f"{x[0]}-W{x[1]}-{'causal' if x[2] else 'full'}-{x[3]}") for x in li.LAUNCHES]
FP8_LAUNCHES = [p for p in LAUNCHES if p.values[0] in ("one_pass", "split") and p.values[3] in ("sinks", "both")]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _ints(torch, values):
    return torch.tensor(list(values), dtype=torch.int32, device="cuda")


def _floats(torch, values):
    return None if values is None else torch.tensor(np.asarray(values, np.float32), dtype=torch.float32, device="cuda")


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _shape(c):
    return tuple(c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))


def _run(fa, torch, dq, kc, vc, lens, W, causal, ps=0, seed=0, scale=None, fmt=None, k_scale=None, v_scale=None, want_S=None,
         sinks=None, softcap=0.0):
    """tests/test_gpu_kvcache_window.py::_run with the two options: kc, vc are caches [B, Hkv, Ncap, d] poisoned for (lens, W), uint16
    encodings (fmt given) or uint8 fp8 codes (fmt None); ps = 0: the contiguous entry, else the paged one on the scattered caches.
    sinks: numpy [Hq] or None.  -> O, lse (device tensors)"""
    B, Hq, Nq, d = dq.shape
    Hkv, Ncap = kc.shape[1], kc.shape[2]
    fp8 = fmt is None
    need = fa.kvcache_window_workspace_bytes(B, Hkv, Hq // Hkv, Nq, Ncap, d, W)
    if want_S is not None:
        assert di.splits_of(need, B * Hkv, (Hq // Hkv) * Nq, d) == want_S
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    kw = dict(cache_seqlens=_ints(torch, lens), causal=causal, scale=scale, return_lse=True, workspace=_nan_workspace(torch, need),
              window=W, sinks=_floats(torch, sinks), softcap=softcap)
    if fp8:
        kw.update(k_scale=_floats(torch, k_scale), v_scale=_floats(torch, v_scale))
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


def _nokey(lens, B, Hq, Nq, Ncap, causal):
    """[B*Hq, Nq] bool: rows that see no key"""
    return np.array([cm.row_limits(cm.clamp(lens[b], Ncap), Nq, Nq, causal)[1] == 0 for b in range(B) for _ in range(Hq)])


def _check(oracle, o, lse, want, want_lse, fmt, what, nokey=None, sinks=None):
    """tests/test_gpu_kvcache_window.py::_check; `nokey` marks the rows that see no key: exact zeros, and lse = -inf without a sink,
    lse = a (to fp32 rounding: the kernel forms a log2(e) ln(2)) with a finite one"""
    want = np.asarray(want, np.float32)
    got = o.float().cpu().numpy().reshape(want.shape)
    got_lse = lse.cpu().numpy().reshape(want_lse.shape)
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    live = np.isfinite(want_lse)
    le = float(np.abs(got_lse[live] - want_lse[live]).max()) if live.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert np.isfinite(got).all(), what + ": O is not finite"
    assert not np.isnan(got_lse).any(), what + ": NaN in lse"
    assert ma <= cm.MAX_ABS and rl <= cm.REL_L2[fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert (got[~live] == 0.0).all(), what + ": a row without a key is not exactly zero"
    assert (got_lse[~live] == -np.inf).all(), what + ": a row without a key or a sink has lse != -inf"
    assert np.isfinite(got_lse[live]).all(), what
    assert le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"
    if nokey is not None:
        assert (got[nokey] == 0.0).all(), what + ": a row without a key is not exactly zero"
        if sinks is not None:
            a = np.tile(np.asarray(sinks, np.float32), got_lse.shape[0] // len(sinks))[:, None].repeat(got_lse.shape[1], 1)
            sel = nokey & np.isfinite(a)
            assert (np.abs(got_lse[sel] - a[sel]) <= 2 * np.spacing(np.abs(a[sel]))).all(), what + ": no key, lse != the sink"


def _case(oracle, torch, name, d, fmt, W):
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    _, (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    return c, dq, *(cm.poisoned(x.reshape(B, Hkv, Ncap, d), c["lens"], Nq, W) for x in (kb, vb))


# ---- 1. parity of the contiguous entry; the paged entry returns its bits ----------------------------------------------------------
@pytest.mark.parametrize("name,W,causal,variant", LAUNCHES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity_and_paged_bits(fa, oracle, torch_cuda, fmt, d, name, W, causal, variant):
    """The three families of tests/window_inputs.py, without a window and under one, with sinks, with a soft-cap and with both,
    through fa_forward_kvcache against the float64 reference, and through fa_forward_kvcache_paged with pages of 16 and 256 keys:
    the same bits, O and lse."""
    torch = torch_cuda
    c, dq, kc, vc = _case(oracle, torch, name, d, fmt, W)
    B, Hkv, G, Nq, Ncap = _shape(c)
    sinks, softcap = li.options(variant, Hkv * G)
    want, want_lse = li.reference(oracle, name, d, fmt, W, causal, variant)
    o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, fmt=fmt, want_S=li.want_S(name, W), sinks=sinks, softcap=softcap)
    _check(oracle, o, lse, want, want_lse, fmt, f"logits {name} W={W} causal={causal} {variant} d={d} fmt={fmt}",
           nokey=_nokey(c["lens"], B, Hkv * G, Nq, Ncap, causal), sinks=sinks)
    for ps in wi.PAGES:
        po, plse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, ps=ps, seed=ps + d + W, fmt=fmt, sinks=sinks, softcap=softcap)
        assert torch.equal(po, o) and torch.equal(plse, lse), f"pages of {ps}: not the contiguous entry's bits"


# ---- 2. fp8 ---------------------------------------------------------------------------------------------------------------------------
K_MULT, V_MULT = (1.0, 6.0), (6.0, 1.0)   # per-head scales 6x apart, in opposite order for K and V: a wrong head index shows


@functools.lru_cache(maxsize=None)
def _quantised(fa, oracle, name, d, fmt):
    """tests/test_gpu_kvcache_window.py::_quantised: K and V of a case quantised on the helper's own scales times K_MULT / V_MULT ->
    q fp32, q encodings, K and V codes [B, Hkv, Ncap, d], the dequantised fp32 values [B*Hkv, Ncap, d], and the scale vectors"""
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


@pytest.mark.parametrize("name,W,causal,variant", FP8_LAUNCHES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_fp8(fa, oracle, torch_cuda, fmt, d, name, W, causal, variant):
    """On a quantize_kv_fp8 cache, contiguous and in pages of 16.  With all scales 1 (NULL): the bits of the 16-bit entry on the
    widened cache under the same options.  With per-head scales: within the bounds of the float64 reference on the dequantised
    cache.  The sinks are not scaled: k_scale is far from 1 here (the codes reach 448), so a sink multiplied by it would move lse
    by far more than the bound."""
    torch = torch_cuda
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    sinks, softcap = li.options(variant, Hkv * G)
    q, qb, k8, v8, kd, vd, ks, vs = _quantised(fa, oracle, name, d, fmt)
    assert max(abs(np.log(s)) for s in ks) > 1.0   # k_scale != 1 by far
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    pk, pv = cm.poisoned(k8, c["lens"], Nq, W, nan=wi.NAN8), cm.poisoned(v8, c["lens"], Nq, W, nan=wi.NAN8)
    wide = [torch.from_numpy(x).view(torch.float8_e4m3fn).to(_tdtype(torch, fmt)).view(torch.int16).numpy().view(np.uint16) for x in (pk, pv)]
    sc = 2.0 ** -7 / np.sqrt(d)
    S = li.want_S(name, W)
    base, base_lse = _run(fa, torch, dq, wide[0], wide[1], c["lens"], W, causal, scale=sc, fmt=fmt, want_S=S, sinks=sinks, softcap=softcap)
    assert torch.isfinite(base).all() and not torch.isnan(base_lse).any()
    want, want_lse = cm.expected_f64(q, kd, vd, c["lens"], B, Hkv, G, Nq, causal, W, softcap=softcap, sinks=sinks)
    for ps in (0, 16):
        o, lse = _run(fa, torch, dq, pk, pv, c["lens"], W, causal, ps=ps, seed=ps + d, scale=sc, want_S=S, sinks=sinks, softcap=softcap)
        assert torch.equal(o, base) and torch.equal(lse, base_lse), f"fp8 layout {ps}: not the 16-bit entry's bits"
        o, lse = _run(fa, torch, dq, pk, pv, c["lens"], W, causal, ps=ps, seed=ps + d + 1, k_scale=ks, v_scale=vs, sinks=sinks,
                      softcap=softcap)
        _check(oracle, o, lse, want, want_lse, fmt, f"fp8 logits {name} W={W} {variant} layout={ps} d={d} fmt={fmt}")


# ---- 3. bit ties ------------------------------------------------------------------------------------------------------------------------
def _raw(fa, torch, dq, dk, dv, dl, W, causal, fmt, need, table=None, scales=None, sinks=None, softcap=0.0):
    """fa_kvcache_decode called through the C ABI as it is: the descriptor filled here, not by the Python front end"""
    B, Hq, Nq, d = dq.shape
    Hkv = dk.shape[1]
    o = torch.full(dq.shape, float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full(dq.shape[:3], float("nan"), dtype=torch.float32, device="cuda")
    ws = _nan_workspace(torch, need)
    geo = dict(Ncap=dk.shape[2]) if table is None else dict(block_table=table.data_ptr(), num_pages=dk.shape[0], page_size=dk.shape[2],
                                                           max_pages=table.shape[1])
    desc = fa.capi.KvDecodeDesc(
        Q=dq.data_ptr(), K=dk.data_ptr(), V=dv.data_ptr(), O=o.data_ptr(), lse=lse.data_ptr(), seqlens_k=dl.data_ptr(),
        k_scale=scales[0].data_ptr() if scales else None, v_scale=scales[1].data_ptr() if scales else None,
        sinks=None if sinks is None else sinks.data_ptr(), kv_dtype=fa.capi.KV_16BIT if scales is None else fa.capi.KV_FP8_E4M3,
        B=B, Hkv=Hkv, G=Hq // Hkv, Nq=Nq, d=d, scale=1.0 / np.sqrt(d), causal=1 if causal else 0, window=W, softcap=softcap,
        in_dtype=fmt, out_dtype=fa.capi.OUT_F32, workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
        stream=torch.cuda.current_stream().cuda_stream, **geo)
    assert fa.lib().fa_kvcache_decode_workspace_bytes(ctypes.byref(desc)) == need
    torch.cuda.synchronize()
    assert fa.lib().fa_kvcache_decode(ctypes.byref(desc)) == 0
    torch.cuda.synchronize()
    return o, lse


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_descriptor_without_options_is_each_of_the_eight_entries(fa, oracle, torch_cuda, fmt, d):
    """sinks = NULL, softcap = 0 through fa_kvcache_decode: O and lse of fa_forward_kvcache and its _paged, _fp8, _paged_fp8 forms,
    without a window (S = 4) and under one (S = 1, their _window forms), on the rows case under the causal mask.  The eight flat
    entries are called through the C ABI (tests/flat_entries.py): the Python front end goes through the descriptor entry alone."""
    torch = torch_cuda
    name = "rows"
    for W in li.case_windows(name):
        c, dq, kc, vc = _case(oracle, torch, name, d, fmt, W)
        B, Hkv, G, Nq, Ncap = _shape(c)
        need = fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W)
        dl = _ints(torch, c["lens"])
        k8, v8 = (torch.from_numpy(np.array(x).view(np.int16)).view(_tdtype(torch, fmt)).float().clamp(-400, 400).nan_to_num(0.0)
                  .to(torch.float8_e4m3fn).view(torch.uint8).numpy() for x in (kc, vc))
        k8, v8 = cm.poisoned(k8, c["lens"], Nq, W, nan=wi.NAN8), cm.poisoned(v8, c["lens"], Nq, W, nan=wi.NAN8)
        sc = (_floats(torch, [0.5, 2.0]), _floats(torch, [3.0, 0.25]))
        for paged in (False, True):
            for fp8 in (False, True):
                kk, vv = (k8, v8) if fp8 else (kc, vc)
                dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
                table = None
                if paged:
                    kk, vv, table = cm.scatter(kk, vv, c["lens"], 16, 77, Nq, W, nan=wi.NAN8 if fp8 else cm.NAN16)
                    table = torch.from_numpy(table).cuda()
                dk, dv = dev(kk), dev(vv)
                base, base_lse = flat.decode(fa, torch, dq, dk, dv, dl, True, fmt, _nan_workspace(torch, need), table=table,
                                             scales=sc if fp8 else None, window=W or None)
                assert torch.isfinite(base).all() and not torch.isnan(base_lse).any()
                o, lse = _raw(fa, torch, dq, dk, dv, dl, W, True, fmt, need, table=table, scales=sc if fp8 else None)
                assert torch.equal(o, base) and torch.equal(lse, base_lse), f"W={W} paged={paged} fp8={fp8}"


@pytest.mark.parametrize("name,W", [("rows", 64), ("rows", 0), ("split", 1024)])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_sinks_of_minus_inf_are_no_sinks(fa, oracle, torch_cuda, fmt, d, name, W):
    """sinks all -inf: O and lse of sinks=None at the same softcap -- with softcap 0 that is the base entry (S = 1 and S = 4).  A
    vector with -inf for some heads: those heads return the no-sink call's bits, the others do not."""
    torch = torch_cuda
    c, dq, kc, vc = _case(oracle, torch, name, d, fmt, W)
    B, Hkv, G, Nq, Ncap = _shape(c)
    Hq = Hkv * G
    causal = c["causal"][-1]
    for softcap in (0.0, li.SOFTCAP):
        base, base_lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, fmt=fmt, want_S=li.want_S(name, W), softcap=softcap)
        o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, fmt=fmt, sinks=np.full(Hq, -np.inf, np.float32), softcap=softcap)
        assert torch.equal(o, base) and torch.equal(lse, base_lse), f"softcap={softcap}"
        if Hq > 1:
            mixed = li.sinks_for(Hq)
            mixed[1::2] = -np.inf
            o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, fmt=fmt, sinks=mixed, softcap=softcap)
            assert torch.equal(o[:, 1::2], base[:, 1::2]) and torch.equal(lse[:, 1::2], base_lse[:, 1::2]), f"softcap={softcap}"
            assert not torch.equal(lse[:, 0::2], base_lse[:, 0::2])


# ---- 4. the sink census -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,causal", [pytest.param(*x, id=f"{x[0]}-W{x[1]}-{'causal' if x[2] else 'full'}") for x in li.CENSUS])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_sink_census(fa, oracle, torch_cuda, fmt, d, name, W, causal):
    """K = 0, V in the residue coding, sinks alternating 0 and -inf: on a head with a sink of 0 the row divides by cnt + 1, on a
    head with -inf by cnt -- every row, all four cache forms.  A sink added per split or by an empty split, taken from another head
    of a folded group, or dropped by the one-pass kernel moves a row total and exp(lse) by a whole number."""
    torch = torch_cuda
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = _shape(c)
    z = li.census_case(oracle, name, d, fmt, W, causal)
    qb, kb, vb = z["bits"]
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    kc, vc = (cm.poisoned(x.reshape(B, Hkv, Ncap, d), c["lens"], Nq, W) for x in (kb, vb))
    to8 = lambda bits: oracle.decode16(np.array(bits), fmt)   # K = 0 and V in {0, m_h <= 8}: exact in e4m3fn
    k8, v8 = (torch.from_numpy(to8(x).reshape(B, Hkv, Ncap, d)).to(torch.float8_e4m3fn).view(torch.uint8).numpy() for x in (kb, vb))
    assert np.array_equal(f8.decode(v8).reshape(-1), to8(vb).reshape(-1))
    k8, v8 = cm.poisoned(k8, c["lens"], Nq, W, nan=wi.NAN8), cm.poisoned(v8, c["lens"], Nq, W, nan=wi.NAN8)
    sinks = li.census_sinks(Hkv * G)
    for ps in (0, 16):
        for fp8 in (False, True):
            kk, vv = (k8, v8) if fp8 else (kc, vc)
            o, lse = _run(fa, torch, dq, kk, vv, c["lens"], W, causal, ps=ps, seed=11 + ps, fmt=None if fp8 else fmt,
                          want_S=li.want_S(name, W), sinks=sinks)
            li.sink_census_check(o.cpu().numpy(), lse.cpu().numpy(), z, what=f"sink census {name} W={W} pages={ps} fp8={fp8}")


# ---- 5. the range of a sink ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W", [("rows", 64), ("split", 1024)])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_sinks_far_from_the_logits(fa, oracle, torch_cuda, fmt, d, name, W):
    """finite sinks 200 above and 200 below ordinary logits, one pass and merge: lse is finite and within the bound (the sink takes
    part in the reference maximum); at +200 O is ~0 without a NaN; at -200 O and lse are the no-sink reference's"""
    torch = torch_cuda
    c, dq, kc, vc = _case(oracle, torch, name, d, fmt, W)
    B, Hkv, G, Nq, Ncap = _shape(c)
    causal = c["causal"][-1]
    (q, k, v), _ = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    nokey = _nokey(c["lens"], B, Hkv * G, Nq, Ncap, causal)
    for a in (200.0, -200.0):
        sinks = np.full(Hkv * G, a, np.float32)
        want, want_lse = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, causal, W, sinks=sinks)
        o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, causal, fmt=fmt, want_S=li.want_S(name, W), sinks=sinks)
        assert torch.isfinite(lse).all()
        _check(oracle, o, lse, want, want_lse, fmt, f"sink {a} {name} d={d} fmt={fmt}", nokey=nokey, sinks=sinks)
        if a > 0:
            assert float(o.abs().max()) < 1e-30
        else:
            base, base_lse = li.reference(oracle, name, d, fmt, W, causal, "none")
            live = np.isfinite(base_lse)
            assert np.abs(want - base).max() < 1e-12 and np.abs(want_lse[live] - base_lse[live]).max() < 1e-12


# ---- 6. the soft-cap under the masks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", li.case_windows("rows"))
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_softcap_under_the_masks(fa, oracle, torch_cuda, fmt, d, W):
    """the rows case (lengths 1000 and 4) under the causal mask with softcap 1: the row without a key still gives exact zeros and
    -inf -- tanh(-inf) = -1 must not make a masked key the finite logit -softcap (_check; every masked key of every other row would
    show as well).  scale = 0 under the cap: uniform weights.  A negative scale: the reference on the negated logits."""
    torch = torch_cuda
    name = "rows"
    c, dq, kc, vc = _case(oracle, torch, name, d, fmt, W)
    B, Hkv, G, Nq, Ncap = _shape(c)
    (q, k, v), _ = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
    nokey = _nokey(c["lens"], B, Hkv * G, Nq, Ncap, True)
    assert nokey.any()
    want, want_lse = li.reference(oracle, name, d, fmt, W, True, "softcap")
    assert (want_lse[nokey] == -np.inf).all()
    for ps in (0, 16):
        o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, True, ps=ps, seed=5, fmt=fmt, softcap=li.SOFTCAP)
        _check(oracle, o, lse, want, want_lse, fmt, f"softcap under the mask W={W} layout={ps} d={d} fmt={fmt}", nokey=nokey)
    uni, uni_lse = cm.uniform_expected(v, c["lens"], B, Hkv, G, Nq, True, W)
    for scale in (0.0, -0.0):
        o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, True, scale=scale, fmt=fmt, softcap=li.SOFTCAP)
        _check(oracle, o, lse, uni, uni_lse, fmt, f"scale {scale} under the cap W={W} d={d} fmt={fmt}", nokey=nokey)
    neg = -1.0 / np.sqrt(d)
    want, want_lse = cm.expected_f64(q, -k, v, c["lens"], B, Hkv, G, Nq, True, W, softcap=li.SOFTCAP)
    o, lse = _run(fa, torch, dq, kc, vc, c["lens"], W, True, scale=neg, fmt=fmt, softcap=li.SOFTCAP)
    _check(oracle, o, lse, want, want_lse, fmt, f"negative scale under the cap W={W} d={d} fmt={fmt}", nokey=nokey)
    assert np.abs(want - li.reference(oracle, name, d, fmt, W, True, "softcap")[0]).max() >= 3 * cm.MAX_ABS   # the sign matters


# ---- 7. graph -------------------------------------------------------------------------------------------------------------------------
def test_captured_append_rope_then_decode_with_sinks_and_softcap(fa, oracle, torch_cuda):
    """append_rope -> decode with a window of 60, sinks and a soft-cap, captured once and replayed over nine steps that take sequence
    0 from 58 keys across L = W and across the tile edge at 64; every step matches the float64 reference on the cache as it then
    stands.  Between the last two replays the sink vector is rewritten in place: the replay follows it."""
    torch = torch_cuda
    g = wi.GRAPH
    B, Hkv, G, Ncap, W, steps, fmt, d = g["B"], g["Hkv"], g["G"], g["Ncap"], g["W"], g["steps"], 0, 64
    Hq = Hkv * G
    (q, k, v), (qb, kb, vb) = wi.inputs(oracle, B, Hkv, G, steps, Ncap, d, fmt, g["seed"])
    kb4, vb4, qb4 = kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), qb.reshape(B, Hq, steps, d)
    lens = list(g["start"])
    dk, dv = (cm.dev16(torch, cm.poisoned(x, lens), fmt) for x in (kb4, vb4))
    dl = _ints(torch, lens)
    # a rotation by angle 0 (cos 1, sin 0): the fused append is on the captured path, and K and Q reach the cache as they were drawn
    cos = torch.ones(Ncap, d // 2, dtype=torch.float32, device="cuda")
    sin = torch.zeros(Ncap, d // 2, dtype=torch.float32, device="cuda")
    sinks = li.sinks_for(Hq)
    dsinks = _floats(torch, sinks)

    def new_rows(t):
        rows = [np.stack([src[b, :, lens[b] + t:lens[b] + t + 1] for b in range(B)]) for src in (kb4, vb4)]
        return cm.dev16(torch, rows[0], fmt), cm.dev16(torch, rows[1], fmt), cm.dev16(torch, qb4[:, :, t:t + 1], fmt)

    need = fa.kvcache_window_workspace_bytes(B, Hkv, G, 1, Ncap, d, W)
    ws = _nan_workspace(torch, need)

    def step(dkn, dvn, dq, ck, cv, cl):
        fa.fa_kvcache_append(dkn, dvn, ck, cv, cache_seqlens=cl, seqlens_out=cl, q=dq, rotary_cos=cos, rotary_sin=sin)
        return fa.fa_forward_kvcache(dq, ck, cv, cl, causal=True, return_lse=True, workspace=ws, window=W, sinks=dsinks,
                                     softcap=li.SOFTCAP)

    dkn, dvn, dq = new_rows(0)
    step(dkn, dvn, dq.clone(), dk.clone(), dv.clone(), dl.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(dkn, dvn, dq, dk, dv, dl)
    assert dl.tolist() == lens   # a capture runs nothing
    for t in range(steps):
        if t == steps - 1:   # rewritten in place: other values, and no sink at all for head 1
            sinks = sinks[::-1].copy() - 1.0
            sinks[1] = -np.inf
            dsinks.copy_(_floats(torch, sinks))
        a, b, c = new_rows(t)
        dkn.copy_(a), dvn.copy_(b), dq.copy_(c)
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        now = [L + t + 1 for L in lens]
        assert dl.tolist() == now
        qt = np.ascontiguousarray(q.reshape(B * Hq, steps, d)[:, t:t + 1])
        want, want_lse = cm.expected_f64(qt, k, v, now, B, Hkv, G, 1, True, W, softcap=li.SOFTCAP, sinks=sinks)
        _check(oracle, o, lse, want, want_lse, fmt, f"graph step {t} lengths {now}")
        if t == steps - 1:
            old, old_lse = cm.expected_f64(qt, k, v, now, B, Hkv, G, 1, True, W, softcap=li.SOFTCAP, sinks=li.sinks_for(Hq))
            assert np.abs(old_lse - want_lse).min() >= li.LSE_MOVES   # the rewritten vector shows on every row


# ---- 8. the torch ops -------------------------------------------------------------------------------------------------------------------
def test_ex_ops_are_the_front_ends(fa, oracle, torch_cuda):
    """one call per _ex op: the bits of the ops front end it stands for"""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    fmt, d, name, W = 1, 128, "rows", 64
    c, dq, kc, vc = _case(oracle, torch, name, d, fmt, W)
    B, Hkv, G, Nq, Ncap = _shape(c)
    dl, ds = _ints(torch, c["lens"]), _floats(torch, li.sinks_for(Hkv * G))
    sc = 1.0 / np.sqrt(d)
    kp, vp, table = cm.scatter(kc, vc, c["lens"], 16, 3, Nq, W)
    dk, dv, dkp, dvp, dt = cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(table).cuda()
    z8 = lambda x: torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(-400, 400).to(torch.float8_e4m3fn)
    dk8, dv8, dkp8, dvp8 = z8(dk.float()), z8(dv.float()), z8(dkp.float()), z8(dvp.float())
    s8 = _floats(torch, [0.5, 2.0])
    kw = dict(cache_seqlens=dl, causal=True, scale=sc, window=W, sinks=ds, softcap=li.SOFTCAP, out_dtype=torch.float32)
    pairs = (
        (ops.decode_ex(dq, dk, dv, dl, sc, True, W, ds, li.SOFTCAP, True), fa.fa_forward_kvcache(dq, dk, dv, **kw)),
        (ops.decode_paged_ex(dq, dkp, dvp, dt, dl, sc, True, W, ds, li.SOFTCAP, True), fa.fa_forward_kvcache_paged(dq, dkp, dvp, dt, **kw)),
        (ops.decode_fp8_ex(dq, dk8, dv8, s8, s8, dl, sc, True, W, ds, li.SOFTCAP, True),
         fa.fa_forward_kvcache_fp8(dq, dk8, dv8, s8, s8, **kw)),
        (ops.decode_paged_fp8_ex(dq, dkp8, dvp8, dt, s8, s8, dl, sc, True, W, ds, li.SOFTCAP, True),
         fa.fa_forward_kvcache_paged_fp8(dq, dkp8, dvp8, dt, s8, s8, **kw)),
    )
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(pairs):
        assert torch.isfinite(want).all() and torch.equal(got, want), i
    plain = fa.fa_forward_kvcache(dq, dk, dv, cache_seqlens=dl, causal=True, scale=sc, window=W)
    assert not torch.equal(pairs[0][0], plain)
