"""GPU tier of fa_merge_states and fa_forward_kvcache_shared_prefix.

Inputs, the float64 rule, the float64 reference of the composed call and the derived fp32 bound are tests/merge_inputs.py's (its CPU
tier, tests/test_merge_inputs.py, shows that no parity launch here passes on a merge that drops a part, doubles one, takes lse for
log2 units or ignores the strides).  The merge is held against the float64 rule on the SAME parts within the derived bound; the
composed call against the float64 reference on the concatenated keys within the project's bounds for two kernels in a row
(cm.peaked_tol(kernels=2), cm.REL_L2, 2 * cm.P_EPS on lse); the exact cases, the ties and the graph replay are bit comparisons.

Poison: rows a part's strides do not name hold NaN; every cache row at or past a length (prefix and suffix) holds NaN bit patterns;
every pool page no table names holds NaN and every dead table entry garbage; the blocks the front end's own allocations reuse
(workspaces, the two states) are filled with NaN bytes beforehand.
"""
import ctypes

import numpy as np
import pytest

import census_inputs as ci
import common_inputs as cm
import fp8_inputs as f8
import logit_inputs as li
import merge_inputs as mi

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
CASES = [pytest.param(*c, id=f"Nq{c[0]}-{'causal' if c[1] else 'full'}-{c[2]}") for c in mi.CASES]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, 0: torch.float16, 1: torch.bfloat16}[name]


def _ints(torch, values):
    return torch.tensor(list(values), dtype=torch.int32, device="cuda")


def _floats(torch, values):
    return None if values is None else torch.tensor(np.asarray(values, np.float32), dtype=torch.float32, device="cuda")


def _bits(torch, t):
    """a tensor's bit patterns, for comparisons that tell -0 from +0 and do not stumble over NaN"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _dev_state(torch, oracle, o, dtype):
    """an O array [X, d] of fp32 values (exact in `dtype`, NaN in the gaps) as a device tensor of that dtype"""
    if dtype == "f32":
        return torch.from_numpy(np.array(o, np.float32)).cuda()
    fmt = 0 if dtype == "f16" else 1
    bits = oracle.encode16(np.nan_to_num(o), fmt)
    bits[np.isnan(o)] = cm.NAN16
    return cm.dev16(torch, bits, fmt)


def _poison_allocator(torch, sizes):
    """blocks of NaN bytes handed back to torch's caching allocator: what the front end allocates next (workspaces, the two states,
    the outputs) starts out as NaN"""
    junk = [torch.full((max(int(s), 1),), 0xFF, dtype=torch.uint8, device="cuda") for s in sizes for _ in range(2)]
    torch.cuda.synchronize()
    del junk


# ---- 1. the merge against the float64 rule on the same parts --------------------------------------------------------------------------
def _merge_raw(fa, torch, dev_parts, B, H, rows, d, part_dtype, out_dtype, with_lse=True):
    """fa_merge_states through the C ABI: dev_parts a list of (O tensor, lse tensor, stride_b, stride_h)"""
    ids = {"f16": fa.capi.STATE_F16, "bf16": fa.capi.STATE_BF16, "f32": fa.capi.STATE_F32}
    out = torch.full((B, H, rows, d), float("nan"), dtype=_tdtype(torch, out_dtype), device="cuda")
    lse = torch.full((B, H, rows), float("nan"), dtype=torch.float32, device="cuda")
    desc = fa.capi.MergeDesc(parts=[(o.data_ptr(), l.data_ptr(), sb, sh) for (o, l, sb, sh) in dev_parts], R=len(dev_parts), B=B, H=H,
                             rows=rows, d=d, part_dtype=ids[part_dtype], O=out.data_ptr(), lse=lse.data_ptr() if with_lse else None,
                             out_dtype=ids[out_dtype], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert fa.lib().fa_merge_states(ctypes.byref(desc)) == 0
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("out_dtype", mi.STATE_DTYPES)
@pytest.mark.parametrize("part_dtype", mi.STATE_DTYPES)
@pytest.mark.parametrize("R", mi.MERGE_R)
@pytest.mark.parametrize("d", (64, 128))
def test_merge_against_the_float64_rule(fa, oracle, torch_cuda, d, R, part_dtype, out_dtype):
    """B2 H2 rows 6, parts with |lse_r - M| <= 40 in the three layouts (contiguous, the [H,B,rows] strides, padded strides with NaN
    in the gaps): O within mi.out_bound -- the derived fp32 bound plus half an ulp of a 16-bit output -- and lse within mi.lse_bound
    of the float64 rule on the same parts."""
    torch = torch_cuda
    B, H, rows = (mi.MERGE_SHAPE[k] for k in ("B", "H", "rows"))
    for lay in mi.LAYOUTS:
        parts = mi.merge_parts(oracle, R, d, part_dtype, lay)
        want, want_lse = mi.merge_f64(parts, B, H, rows)
        dev = [(_dev_state(torch, oracle, o, part_dtype), torch.from_numpy(np.array(l)).cuda(), sb, sh) for (o, l, sb, sh) in parts]
        out, lse = _merge_raw(fa, torch, dev, B, H, rows, d, part_dtype, out_dtype)
        got, got_lse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
        vmax = max(float(np.nanmax(np.abs(o))) for (o, _, _, _) in parts)
        err, bound = np.abs(got - want), mi.out_bound(R, vmax, want, out_dtype)
        lerr, lbound = float(np.abs(got_lse - want_lse).max()), mi.lse_bound(R, np.abs(want_lse).max())
        print(f"merge d={d} R={R} {part_dtype}->{out_dtype} {lay}: O err {err.max():.3e} (fp32 bound {mi.f32_bound(R, vmax):.3e}, "
              f"worst err/bound {float((err / bound).max()):.3f}) lse err {lerr:.3e} (bound {lbound:.3e})")
        assert np.isfinite(got).all() and np.isfinite(got_lse).all(), lay
        assert (err <= bound).all(), f"{lay}: O off by {err.max():.3e}, {float((err / bound).max()):.2f} of the bound"
        assert lerr <= lbound, f"{lay}: lse off by {lerr:.3e} > {lbound:.3e}"


# ---- 2. the exact cases ------------------------------------------------------------------------------------------------------------------
def _exact_part(torch, dtype, B, Hq, Nq, d, seed):
    """a part with zeros of both signs, values below the 16-bit normal range and ordinary ones"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    o = (torch.randn(B, Hq, Nq, d, device="cuda", generator=g) * 3).to(_tdtype(torch, dtype))
    o[..., 0], o[..., 1], o[..., 2] = 0.0, -0.0, 2.0 ** -20
    o[..., 3] = -(2.0 ** -130) if dtype != "f16" else -(2.0 ** -24)
    lse = torch.randn(B, Hq, Nq, device="cuda", generator=g) * 20
    return o, lse


@pytest.mark.parametrize("dtype", mi.STATE_DTYPES)
@pytest.mark.parametrize("d", (64, 128))
def test_exact_cases(fa, torch_cuda, d, dtype):
    """R = 1 returns the part's bits, O and lse (and its one rounding when the output type differs); one finite part among -inf
    parts whose O rows hold NaN bit patterns comes through exactly; all parts -inf gives +0 and -inf; without lse the O is the same."""
    torch = torch_cuda
    B, Hq, Nq = 2, 4, 3
    tdt = _tdtype(torch, dtype)
    o, lse = _exact_part(torch, dtype, B, Hq, Nq, d, 5 + d)
    got, got_lse = fa.fa_merge_states([o], [lse], out_dtype=tdt)
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch, got), _bits(torch, o)) and torch.equal(_bits(torch, got_lse), _bits(torch, lse))
    for other in mi.STATE_DTYPES:
        if other != dtype:
            g2, l2 = fa.fa_merge_states([o], [lse], out_dtype=_tdtype(torch, other))
            assert torch.equal(_bits(torch, g2), _bits(torch, o.to(_tdtype(torch, other)))) and torch.equal(l2, lse), other
    dead_o = torch.full_like(o, float("nan"))
    dead_l = torch.full_like(lse, float("-inf"))
    for R, at in ((2, 0), (2, 1), (5, 3), (16, 15), (16, 6)):
        outs = [o if r == at else dead_o for r in range(R)]
        lses = [lse if r == at else dead_l for r in range(R)]
        g2, l2 = fa.fa_merge_states(outs, lses, out_dtype=tdt)
        assert torch.equal(_bits(torch, g2), _bits(torch, o)) and torch.equal(_bits(torch, l2), _bits(torch, lse)), (R, at)
        g3 = fa.fa_merge_states(outs, lses, out_dtype=tdt, return_lse=False)
        assert torch.equal(_bits(torch, g3), _bits(torch, o))
    # rows where every part is neutral, next to rows with one live part
    mixed = lse.clone()
    mixed[:, ::2] = float("-inf")
    for R in (1, 3, 16):
        g2, l2 = fa.fa_merge_states([dead_o if r else o for r in range(R)], [dead_l if r else mixed for r in range(R)], out_dtype=tdt)
        torch.cuda.synchronize()
        assert torch.equal(_bits(torch, g2[:, ::2]), torch.zeros_like(_bits(torch, g2[:, ::2]))), R     # +0, not -0, not NaN
        assert (l2[:, ::2] == float("-inf")).all()
        assert torch.equal(_bits(torch, g2[:, 1::2]), _bits(torch, o[:, 1::2])) and torch.equal(l2[:, 1::2], lse[:, 1::2])
    # two live parts: the lse output does not move O
    o2, lse2 = _exact_part(torch, dtype, B, Hq, Nq, d, 6 + d)
    a, _ = fa.fa_merge_states([o, o2], [lse, lse2], out_dtype=tdt)
    b = fa.fa_merge_states([o, o2], [lse, lse2], out_dtype=tdt, return_lse=False)
    assert torch.isfinite(a.float()).all() and torch.equal(_bits(torch, a), _bits(torch, b))


# ---- 3. the composed call against the float64 reference -------------------------------------------------------------------------------
def _device_inputs(torch, oracle, shape_name, Nq, d, fmt, fp8, lens=None, P=None):
    """the caches of a case on the device, poisoned past the lengths -> dict dq, prefix (k, v), suffix numpy caches, scales"""
    c = mi.SHAPE if shape_name == "base" else mi.LONG
    B, Hkv, G = c["B"], c["Hkv"], c["G"]
    lens = c["lens"] if lens is None else lens
    P = c["P"] if P is None else P
    x = mi.inputs(oracle, shape_name, Nq, d, fmt, fp8)
    kpb, vpb, ksb, vsb = x["bits"]
    dq = cm.dev16(torch, x["qb"], fmt).view(B, Hkv * G, Nq, d)
    dev, nan = ((lambda a: cm.dev8(torch, a)), f8.NAN_CODES[0]) if fp8 else ((lambda a: cm.dev16(torch, a, fmt)), cm.NAN16)
    pre = [dev(cm.poisoned(a.reshape(1, Hkv, c["Pcap"], d), [P], nan=nan)) for a in (kpb, vpb)]
    suf = [cm.poisoned(a.reshape(B, Hkv, c["Ncap"], d), lens, nan=nan) for a in (ksb, vsb)]
    return dict(x=x, c=c, dq=dq, pre=pre, suf=suf, lens=lens, P=P, k_scale=_floats(torch, x["k_scale"]), v_scale=_floats(torch, x["v_scale"]))


def _composed(fa, torch, t, fmt, fp8, causal, variant, paged, seed=0, out_dtype=None, dsinks=None, dlens=None, dP=None):
    """fa_forward_kvcache_shared_prefix on a case's device inputs, contiguous or in pages of 16 -> O, lse"""
    c = t["c"]
    B, Hkv, G = c["B"], c["Hkv"], c["G"]
    Nq, d = t["dq"].shape[2:]
    sinks, softcap = li.options(variant, Hkv * G)
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    kw = dict(prefix_len=_ints(torch, [t["P"]]) if dP is None else dP, cache_seqlens=_ints(torch, t["lens"]) if dlens is None else dlens,
              causal=causal, return_lse=True, softcap=softcap, out_dtype=out_dtype,
              sinks=(_floats(torch, sinks) if dsinks is None else dsinks) if sinks is not None else None)
    if fp8:
        kw.update(k_scale=t["k_scale"], v_scale=t["v_scale"])
    if paged:
        kp, vp, table = cm.scatter(t["suf"][0], t["suf"][1], t["lens"], c["page"], seed, nan=f8.NAN_CODES[0] if fp8 else cm.NAN16)
        kw.update(block_table=torch.from_numpy(table).cuda())
        ks, vs = dev(kp), dev(vp)
    else:
        ks, vs = dev(t["suf"][0]), dev(t["suf"][1])
    need = (fa.kvcache_workspace_bytes(1, Hkv, B * G, Nq, c["Pcap"], d), fa.kvcache_workspace_bytes(B, Hkv, G, Nq, c["Ncap"], d),
            4 * t["dq"].numel(), 4 * t["dq"].numel() // d)
    _poison_allocator(torch, need)
    o, lse = fa.fa_forward_kvcache_shared_prefix(t["dq"], t["pre"][0], t["pre"][1], ks, vs, **kw)
    torch.cuda.synchronize()
    assert o.shape == t["dq"].shape and lse.shape == t["dq"].shape[:3] and lse.dtype == torch.float32
    return o, lse


def _check(oracle, o, lse, want, want_lse, fmt, vmax, what):
    """the project's bounds for two kernels in a row: cm.peaked_tol(fmt, vmax, kernels=2) and cm.REL_L2 for O, 2 * cm.P_EPS absolute
    for lse; every figure is printed before it is judged"""
    want = np.asarray(want, np.float32)
    got = o.float().cpu().numpy().reshape(want.shape)
    got_lse = lse.cpu().numpy().reshape(want_lse.shape)
    assert np.isfinite(want_lse).all()
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    le = float(np.abs(got_lse - want_lse).max())
    tol = cm.peaked_tol(fmt, vmax, kernels=2)
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {tol:.2e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert np.isfinite(got).all(), what + ": O is not finite"
    assert np.isfinite(got_lse).all(), what + ": lse is not finite"
    assert ma <= tol and rl <= cm.REL_L2[fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"


@pytest.mark.parametrize("Nq,causal,variant", CASES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_composed_parity(fa, oracle, torch_cuda, fmt, d, Nq, causal, variant):
    """B3 Hkv2 G4, Pcap 200 with prefix_len 130, Ncap 192 with cache_seqlens (0, 1, 150): the contiguous suffix and the one in pages
    of 16 against the float64 reference on the concatenated keys; the two return the same bits."""
    torch = torch_cuda
    t = _device_inputs(torch, oracle, "base", Nq, d, fmt, False)
    want, want_lse = mi.reference(oracle, "base", Nq, d, fmt, causal, variant)
    o, lse = _composed(fa, torch, t, fmt, False, causal, variant, False)
    _check(oracle, o, lse, want, want_lse, fmt, mi.vmax_of(t["x"]), f"shared prefix Nq={Nq} causal={causal} {variant} d={d} fmt={fmt}")
    po, plse = _composed(fa, torch, t, fmt, False, causal, variant, True, seed=d + Nq)
    assert torch.equal(po, o) and torch.equal(plse, lse), "pages of 16: not the contiguous suffix's bits"


@pytest.mark.parametrize("Nq,causal,variant", CASES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_composed_parity_fp8(fa, oracle, torch_cuda, fmt, d, Nq, causal, variant):
    """the same on e4m3fn caches with per-head scales that prefix and suffix share, contiguous and paged, against the float64
    reference on the dequantised values"""
    torch = torch_cuda
    t = _device_inputs(torch, oracle, "base", Nq, d, fmt, True)
    assert max(abs(np.log(s)) for s in t["x"]["k_scale"]) > 1.0   # the scales are far from 1: dropping one shows
    want, want_lse = mi.reference(oracle, "base", Nq, d, fmt, causal, variant, True)
    for paged in (False, True):
        o, lse = _composed(fa, torch, t, fmt, True, causal, variant, paged, seed=d + Nq + 1)
        _check(oracle, o, lse, want, want_lse, fmt, mi.vmax_of(t["x"]),
               f"shared prefix fp8 paged={paged} Nq={Nq} causal={causal} {variant} d={d} fmt={fmt}")


@pytest.mark.parametrize("Nq", mi.NQS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_composed_parity_with_a_split_prefix(fa, oracle, torch_cuda, fmt, d, Nq):
    """a prefix long enough that the prefix decode splits its keys (a workspace is needed): the merge kernel behind the split merge"""
    torch = torch_cuda
    c = mi.LONG
    assert fa.kvcache_workspace_bytes(1, c["Hkv"], c["B"] * c["G"], Nq, c["Pcap"], d) > 0
    t = _device_inputs(torch, oracle, "long", Nq, d, fmt, False)
    want, want_lse = mi.reference(oracle, "long", Nq, d, fmt, True, "both")
    o, lse = _composed(fa, torch, t, fmt, False, True, "both", False)
    _check(oracle, o, lse, want, want_lse, fmt, mi.vmax_of(t["x"]), f"split prefix Nq={Nq} d={d} fmt={fmt}")


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_ties(fa, oracle, torch_cuda, fmt, d):
    """prefix_len = 0: the bits of the plain entry on the suffix, O in both output types and lse.  A sequence with cache_seqlens = 0:
    its rows are the prefix part's, bit for bit."""
    torch = torch_cuda
    Nq, causal = 3, True
    c = mi.SHAPE
    B, Hkv, G = c["B"], c["Hkv"], c["G"]
    lens = (5, 1, 150)
    t = _device_inputs(torch, oracle, "base", Nq, d, fmt, False, lens=lens, P=0)
    ks, vs = cm.dev16(torch, t["suf"][0], fmt), cm.dev16(torch, t["suf"][1], fmt)
    sinks = _floats(torch, li.sinks_for(Hkv * G))
    for out_dtype in (torch.float32, _tdtype(torch, fmt)):
        plain, plain_lse = fa.fa_forward_kvcache(t["dq"], ks, vs, _ints(torch, lens), causal=causal, return_lse=True, out_dtype=out_dtype,
                                                 sinks=sinks, softcap=li.SOFTCAP)
        o, lse = _composed(fa, torch, t, fmt, False, causal, "both", False, out_dtype=out_dtype)
        assert o.dtype == out_dtype and torch.isfinite(o.float()).all()
        assert torch.equal(_bits(torch, o), _bits(torch, plain)) and torch.equal(_bits(torch, lse), _bits(torch, plain_lse)), out_dtype
    # an empty suffix: the prefix part, as the folded decode returns it
    t = _device_inputs(torch, oracle, "base", Nq, d, fmt, False)
    assert t["lens"][0] == 0
    o, lse = _composed(fa, torch, t, fmt, False, causal, "none", False)
    qp = t["dq"].view(B, Hkv, G, Nq, d).permute(1, 0, 2, 3, 4).reshape(1, Hkv * B * G, Nq, d).contiguous()
    o_p, lse_p = fa.fa_forward_kvcache(qp, t["pre"][0], t["pre"][1], _ints(torch, [t["P"]]), return_lse=True)
    o_p = o_p.view(Hkv, B, G, Nq, d).permute(1, 0, 2, 3, 4).reshape(B, Hkv * G, Nq, d)
    lse_p = lse_p.view(Hkv, B, G, Nq).permute(1, 0, 2, 3).reshape(B, Hkv * G, Nq)
    torch.cuda.synchronize()
    assert torch.isfinite(o_p).all() and torch.equal(_bits(torch, o[0]), _bits(torch, o_p[0])) and torch.equal(lse[0], lse_p[0])
    assert not torch.equal(o[2], o_p[2])


# ---- 5. the census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_census(fa, oracle, torch_cuda, fmt, d, causal):
    """K = 0, V in the residue coding: every prefix key and every suffix key a row sees is counted exactly once on every row, the
    causal rows that see no suffix key included -- contiguous and paged."""
    torch = torch_cuda
    c = mi.SHAPE
    B, Hkv, G, Pcap, P, Ncap = (c[k] for k in ("B", "Hkv", "G", "Pcap", "P", "Ncap"))
    Nq = 3
    z = mi.census_case(oracle, Nq, d, fmt, causal)
    assert (z["cnt"] == P).any()
    dq = cm.dev16(torch, z["qb"], fmt).view(B, Hkv * G, Nq, d)
    pre = [cm.dev16(torch, cm.poisoned(a.reshape(1, Hkv, Pcap, d), [P]), fmt) for a in z["prefix"]]
    suf = [cm.poisoned(a.reshape(B, Hkv, Ncap, d), c["lens"]) for a in z["suffix"]]
    t = dict(c=c, dq=dq, pre=pre, suf=suf, lens=c["lens"], P=P)
    for paged in (False, True):
        o, lse = _composed(fa, torch, t, fmt, False, causal, "none", paged, seed=3)
        got = o.cpu().numpy().astype(np.float64).reshape(z["S"].shape)
        assert np.isfinite(got).all()
        ci.census_check(got, z["S"], z["cnt"], np.ones(B * Hkv * G), what=f"shared prefix census paged={paged}")
        assert (np.abs(np.exp(lse.cpu().numpy().astype(np.float64).reshape(z["cnt"].shape)) - z["cnt"]) <= ci.MARGIN).all()


# ---- 6. graph -----------------------------------------------------------------------------------------------------------------------------
def test_captured_call_follows_lengths_and_sinks(fa, oracle, torch_cuda):
    """the composed call captured once; prefix_len, cache_seqlens and the sinks rewritten in place: every replay returns the bits
    of the eager call on the same values"""
    torch = torch_cuda
    fmt, d, Nq = 1, 128, 3
    c = mi.SHAPE
    B, Hkv, G = c["B"], c["Hkv"], c["G"]
    t = _device_inputs(torch, oracle, "base", Nq, d, fmt, False, lens=(c["Ncap"],) * B, P=c["Pcap"])   # nothing poisoned: any length is live
    ks, vs = cm.dev16(torch, t["suf"][0], fmt), cm.dev16(torch, t["suf"][1], fmt)
    dP, dlens, dsinks = _ints(torch, [c["P"]]), _ints(torch, c["lens"]), _floats(torch, li.sinks_for(Hkv * G))

    def call():
        return fa.fa_forward_kvcache_shared_prefix(t["dq"], t["pre"][0], t["pre"][1], ks, vs, prefix_len=dP, cache_seqlens=dlens,
                                                   causal=True, return_lse=True, sinks=dsinks, softcap=li.SOFTCAP)

    call()                                       # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = call()
    seen = []
    for P, lens, shift in ((c["P"], c["lens"], 0.0), (0, (7, 150, 2), -1.0), (c["Pcap"], (192, 0, 64), 2.0), (1, (0, 0, 0), 0.5)):
        dP.copy_(_ints(torch, [P])), dlens.copy_(_ints(torch, lens)), dsinks.copy_(_floats(torch, li.sinks_for(Hkv * G) + shift))
        o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eo, elo = call()
        torch.cuda.synchronize()
        assert torch.isfinite(eo).all() and torch.equal(_bits(torch, o), _bits(torch, eo)) and torch.equal(lse, elo), (P, lens)
        seen.append(eo.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- 7. the torch ops ---------------------------------------------------------------------------------------------------------------------
def test_ops_are_the_front_ends(fa, oracle, torch_cuda):
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    fmt, d, Nq = 0, 64, 3
    c = mi.SHAPE
    B, Hkv, G = c["B"], c["Hkv"], c["G"]
    t = _device_inputs(torch, oracle, "base", Nq, d, fmt, False)
    ks, vs = cm.dev16(torch, t["suf"][0], fmt), cm.dev16(torch, t["suf"][1], fmt)
    dP, dlens, dsinks = _ints(torch, [c["P"]]), _ints(torch, c["lens"]), _floats(torch, li.sinks_for(Hkv * G))
    sc = 1.0 / np.sqrt(d)
    for f32 in (True, False):
        want = fa.fa_forward_kvcache_shared_prefix(t["dq"], t["pre"][0], t["pre"][1], ks, vs, prefix_len=dP, cache_seqlens=dlens, causal=True,
                                                   scale=sc, sinks=dsinks, softcap=li.SOFTCAP, out_dtype=None if f32 else t["dq"].dtype)
        got = ops.decode_shared_prefix(t["dq"], t["pre"][0], t["pre"][1], ks, vs, dP, dlens, sc, True, dsinks, li.SOFTCAP, f32)
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all() and torch.equal(got, want), f32
    g = torch.Generator(device="cuda").manual_seed(3)
    outs = torch.randn(3, 2, 4, 3, d, device="cuda", generator=g).half()
    lses = torch.randn(3, 2, 4, 3, device="cuda", generator=g) * 5
    for f32 in (True, False):
        want, want_lse = fa.fa_merge_states(list(outs), list(lses), out_dtype=torch.float32 if f32 else torch.float16)
        got, got_lse = ops.merge_states(outs, lses, f32)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(got_lse, want_lse), f32
