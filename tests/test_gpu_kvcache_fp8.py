"""GPU tier of the fp8 KV-cache decode entries (fa_forward_kvcache_fp8, fa_forward_kvcache_paged_fp8).

Two kinds of check.
Bit equality: an e4m3fn value is exactly an fp16 and a bf16 value, and the fp8 kernels are the 16-bit kernels behind another way of
filling LDS, so on a cache whose bytes run through all 254 finite codes O and the log-sum-exp must EQUAL what fa_forward_kvcache
returns on the same cache widened by torch on the CPU.  With power-of-two scales the scales commute with every rounding, so they
are part of that check.  This is also the first run of v_cvt_scalef32_pk_{f16,bf16}_fp8 over every code on hardware.
Oracle parity: method and tolerances of tests/test_gpu_kvcache_paged.py.  Expected O from oracle.forward_cross on the fp32 values
decode(k8) * k_scale[h] and decode(v8) * v_scale[h] (the table of tests/fp8_inputs.py, not torch's conversion), expected
log-sum-exps from float64 numpy on the same values.  The oracle sees the dequantised values, so the quantisation error is not part
of the comparison and the 16-bit entries' bounds apply unchanged: the project's max-abs bar and relative-L2 bounds for O,
2 * P_EPS absolute for the log-sum-exp.  Data is N(0,1) quantised with fa.quantize_kv_fp8, so the outputs have the magnitude of
the 16-bit tests'.

Every row at and past a length, every page no table names and every dead table entry holds 0x7F (NaN) or garbage, and the workspace
is filled with NaN bytes: an over-read shows as a non-finite result, not as a fault.
"""
import functools

import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import fp8_inputs as f8

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
LAYOUTS = [pytest.param(0, id="contiguous"), pytest.param(16, id="p16"), pytest.param(64, id="p64")]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _q_dev(torch, qb, fmt, B, Hq):
    return torch.from_numpy(np.array(qb).view(np.int16)).cuda().view(_tdtype(torch, fmt)).view(B, Hq, qb.shape[1], qb.shape[2])


def _widened(torch, codes, fmt):
    """the cache a 16-bit entry takes for the same values: torch's CPU conversion, then the copy"""
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn).to(_tdtype(torch, fmt)).cuda()


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _scales(torch, values):
    return None if values is None else torch.tensor(list(values), dtype=torch.float32, device="cuda")


def _run(fa, torch, dq, k8, v8, lens, ps, seed, k_scale=None, v_scale=None, causal=False, scale=None, out_dtype=None):
    """k8, v8: poisoned caches [B, Hkv, Ncap, d] of codes.  ps = 0: the contiguous entry; else the paged one on the caches scattered
    into pages of ps keys.  -> (O, lse) device tensors, workspace bytes"""
    B, Hq, Nq, d = dq.shape
    Hkv, Ncap = k8.shape[1], k8.shape[2]
    dl = torch.tensor(list(lens), dtype=torch.int32, device="cuda")
    need = fa.kvcache_workspace_bytes(B, Hkv, Hq // Hkv, Nq, Ncap, d)
    kw = dict(k_scale=_scales(torch, k_scale), v_scale=_scales(torch, v_scale), cache_seqlens=dl, causal=causal, scale=scale,
              out_dtype=out_dtype, return_lse=True, workspace=_nan_workspace(torch, need))
    if ps == 0:
        o, lse = fa.fa_forward_kvcache_fp8(dq, cm.dev8(torch, k8), cm.dev8(torch, v8), **kw)
    else:
        assert fa.kvcache_paged_workspace_bytes(B, Hkv, Hq // Hkv, Nq, Ncap // ps, ps, d) == need
        kp, vp, table = cm.scatter(k8, v8, lens, ps, seed, nan=f8.NAN_CODES[0])
        o, lse = fa.fa_forward_kvcache_paged_fp8(dq, cm.dev8(torch, kp), cm.dev8(torch, vp), torch.from_numpy(table).cuda(), **kw)
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o, lse, need


def _check(oracle, o, lse, want, want_lse, fmt, what, max_abs=cm.MAX_ABS):
    got = o.float().cpu().numpy().reshape(want.shape)
    got_lse = lse.cpu().numpy().reshape(want_lse.shape)
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    live = np.isfinite(want_lse)
    le = float(np.abs(got_lse[live] - want_lse[live]).max()) if live.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {max_abs:.1e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert np.isfinite(got).all(), what + ": O is not finite"
    assert not np.isnan(got_lse).any(), what + ": NaN in lse"
    assert ma <= max_abs and rl <= cm.REL_L2[fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    # rows without a key: exact zeros and -inf; every other row: a finite lse within the bound
    assert (got[~live] == 0.0).all(), what + ": a row without a key is not exactly zero"
    assert (got_lse[~live] == -np.inf).all(), what + ": a row without a key has lse != -inf"
    assert np.isfinite(got_lse[live]).all(), what
    assert le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"


# ---- bit equality on all finite codes ----------------------------------------------------------------------------------------------
BITEQ_SHAPE = dict(B=3, Hkv=2, G=2, Nq=3)
BITEQ_CACHES = ((1280, (1, 773, 1280), True), (256, (5, 200, 256), False))   # (Ncap, lens, splits)


@functools.lru_cache(maxsize=None)
def _all_code_inputs(oracle, Ncap, lens, d, fmt):
    B, Hkv, G, Nq = (BITEQ_SHAPE[n] for n in ("B", "Hkv", "G", "Nq"))
    _, (qb, _, _) = oracle.make_qkv(B * Hkv * G, Nq, d, fmt=fmt, seed=2101)
    k8 = f8.all_codes_cache(B, Hkv, Ncap, d, lens, seed=2102)
    v8 = f8.all_codes_cache(B, Hkv, Ncap, d, lens, seed=2103)
    for b, L in enumerate(lens):   # what the test is named for
        if L * d >= 254:
            assert all(set(x[b, h, :L].ravel().tolist()) == set(f8.FINITE_CODES.tolist()) for x in (k8, v8) for h in range(Hkv))
    for a in (qb, k8, v8):
        a.setflags(write=False)
    return qb, k8, v8


@functools.lru_cache(maxsize=None)
def _all_code_base(fa, oracle, Ncap, lens, d, fmt, causal, scale):
    """fa_forward_kvcache on the widened cache: computed once per case, shared by the layouts (device tensors, never written)"""
    import torch
    B, Hkv, G, Nq = (BITEQ_SHAPE[n] for n in ("B", "Hkv", "G", "Nq"))
    qb, k8, v8 = _all_code_inputs(oracle, Ncap, lens, d, fmt)
    dq = _q_dev(torch, qb, fmt, B, Hkv * G)
    need = fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    base, base_lse = fa.fa_forward_kvcache(dq, _widened(torch, k8, fmt), _widened(torch, v8, fmt),
                                           torch.tensor(lens, dtype=torch.int32, device="cuda"), causal=causal, scale=scale,
                                           return_lse=True, workspace=_nan_workspace(torch, need))
    torch.cuda.synchronize()
    assert torch.isfinite(base).all() and not torch.isnan(base_lse).any()   # -inf: a row the mask leaves without a key
    return dq, base, base_lse, need


@pytest.mark.parametrize("ps", LAYOUTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bit_equal_to_16bit_entry_on_all_codes(fa, oracle, torch_cuda, fmt, d, causal, ps):
    """K and V bytes cover all 254 finite codes; k_scale 2^-7 for both heads, v_scale (2^-8, 2^-9), fp32 output.  Expected:
    fa_forward_kvcache on the widened cache with scale * 2^-7, times v_scale on the host -- every one of those products is exact, so
    O and the log-sum-exp are compared with torch.equal.  Behind a split (1280 keys) and in one pass (256 keys)."""
    torch = torch_cuda
    B, Hkv, G, Nq = (BITEQ_SHAPE[n] for n in ("B", "Hkv", "G", "Nq"))
    ks, vs = (2.0 ** -7, 2.0 ** -7), (2.0 ** -8, 2.0 ** -9)
    scale = 1.0 / np.sqrt(d)
    for Ncap, lens, split in BITEQ_CACHES:
        dq, base, base_lse, need = _all_code_base(fa, oracle, Ncap, lens, d, fmt, causal, scale * ks[0])
        assert (need > 0) == split
        want = (base.view(B, Hkv, G, Nq, d) * torch.tensor(vs, device="cuda").view(1, Hkv, 1, 1, 1)).view(base.shape)
        _, k8, v8 = _all_code_inputs(oracle, Ncap, lens, d, fmt)
        got, got_lse, _ = _run(fa, torch, dq, k8, v8, lens, ps, seed=ps + d, k_scale=ks, v_scale=vs, causal=causal, scale=scale)
        assert torch.isfinite(got).all() and not torch.isnan(got_lse).any()
        diff, ldiff = (got - want).abs().max().item(), (got_lse - base_lse).abs().max().item()
        print(f"fmt={fmt} d={d} layout={ps} Ncap={Ncap} causal={causal}: max |fp8 - 16 bit| = {diff:.3e}, lse {ldiff:.3e}")
        assert torch.equal(got, want) and torch.equal(got_lse, base_lse), (ps, Ncap, causal, diff, ldiff)


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_null_scales_are_ones(fa, oracle, torch_cuda, fmt, d):
    """NULL scale pointers, tensors of ones, and one of each: the same bits, and those of the 16-bit entry on the widened cache."""
    torch = torch_cuda
    B, Hkv, G, Nq = (BITEQ_SHAPE[n] for n in ("B", "Hkv", "G", "Nq"))
    scale = 2.0 ** -7 / np.sqrt(d)   # all-code values reach 448: the factor k_scale carries in the test above
    for Ncap, lens, _ in BITEQ_CACHES:
        dq, base, base_lse, _ = _all_code_base(fa, oracle, Ncap, lens, d, fmt, True, scale)
        _, k8, v8 = _all_code_inputs(oracle, Ncap, lens, d, fmt)
        for ps in (0, 16):
            for ks, vs in ((None, None), ((1.0, 1.0), (1.0, 1.0)), (None, (1.0, 1.0)), ((1.0, 1.0), None)):
                got, got_lse, _ = _run(fa, torch, dq, k8, v8, lens, ps, seed=7, k_scale=ks, v_scale=vs, causal=True, scale=scale)
                assert torch.equal(got, base) and torch.equal(got_lse, base_lse), (ps, Ncap, ks, vs)


# ---- oracle parity -------------------------------------------------------------------------------------------------------------------
K_MULT, V_MULT = (1.0, 6.0), (6.0, 1.0)   # per-head scales 6x apart, in opposite order for K and V: a wrong head index shows


@functools.lru_cache(maxsize=None)
def _quantised_inputs(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed):
    """N(0,1) inputs (tests/decode_inputs.py::inputs), K and V quantised with fa.quantize_kv_fp8 on scales that are the helper's own
    times K_MULT / V_MULT cycled over the heads (not powers of two).  -> q fp32, q encodings, K and V codes [B, Hkv, Ncap, d], the
    fp32 values decode(code) * scale[h] as [B*Hkv, Ncap, d], and the two scale vectors."""
    import torch
    (q, k, v), (qb, _, _) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed)
    out = []
    for x, mult in ((k, K_MULT), (v, V_MULT)):
        x4 = torch.from_numpy(x.reshape(B, Hkv, Ncap, d).copy())
        _, s0 = fa.quantize_kv_fp8(x4)
        s = (s0 * torch.tensor([mult[h % 2] for h in range(Hkv)])).contiguous()
        x8, s_back = fa.quantize_kv_fp8(x4, scale=s)
        assert torch.equal(s_back, s)
        codes = x8.view(torch.uint8).numpy().copy()
        assert not np.isin(codes, f8.NAN_CODES).any()
        deq = (f8.decode(codes) * s.numpy().reshape(1, Hkv, 1, 1)).astype(np.float32).reshape(B * Hkv, Ncap, d)
        for a in (codes, deq):
            a.setflags(write=False)
        out.append((codes, deq, tuple(float(t) for t in s)))
    (k8, kd, ks), (v8, vd, vs) = out
    if Hkv > 1:
        assert max(ks) / min(ks) > 4 and max(vs) / min(vs) > 4 and (ks[0] < ks[1]) != (vs[0] < vs[1])
    return q, qb, k8, v8, kd, vd, ks, vs


@functools.lru_cache(maxsize=None)
def _reference(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed, lens, causal):
    q, _, _, _, kd, vd, _, _ = _quantised_inputs(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed)
    out, lse = cm.expected(oracle, q, kd, vd, lens, B, Hkv, G, Nq, causal)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


@pytest.mark.parametrize("ps,Ncap", [(0, 1088), (16, 1056), (64, 1088), (256, 1280)], ids=["contiguous", "p16", "p64", "p256"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_oracle_parity(fa, oracle, torch_cuda, fmt, d, ps, Ncap):
    """The shapes of tests/test_gpu_kvcache_paged.py::test_oracle_parity: split over the keys with lengths 1, 3 pages + 5 and the
    capacity; both output types; per-head scales that are no powers of two."""
    B, Hkv, G, Nq = 3, 2, 2, 1
    lens = (1, 3 * (ps or 64) + 5, Ncap)
    _, qb, k8, v8, _, _, ks, vs = _quantised_inputs(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2201)
    want, want_lse = _reference(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2201, lens, False)
    dq = _q_dev(torch_cuda, qb, fmt, B, Hkv * G)
    pk, pv = (cm.poisoned(x, lens, nan=f8.NAN_CODES[0]) for x in (k8, v8))
    for out_same in (False, True):
        o, lse, need = _run(fa, torch_cuda, dq, pk, pv, lens, ps, seed=ps + d, k_scale=ks, v_scale=vs,
                            out_dtype=_tdtype(torch_cuda, fmt) if out_same else None)
        assert need > 0 and o.dtype == (_tdtype(torch_cuda, fmt) if out_same else torch_cuda.float32)
        _check(oracle, o, lse, want, want_lse, fmt, f"fp8 parity d={d} fmt={fmt} layout={ps} out_same={out_same}")


@pytest.mark.parametrize("ps", LAYOUTS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_single_pass(fa, oracle, torch_cuda, fmt, d, ps):
    """The shape of tests/test_gpu_kvcache_paged.py::test_single_pass: S = 1, no workspace, the kernel applies v_scale and writes O
    and the log-sum-exp itself.  A sequence of one key returns v_scale * its V row."""
    B, Hkv, G, Nq, Ncap, lens = 3, 2, 1, 1, 192, (1, 64, 190)
    _, qb, k8, v8, _, vd, ks, vs = _quantised_inputs(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2301)
    want, want_lse = _reference(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2301, lens, False)
    dq = _q_dev(torch_cuda, qb, fmt, B, Hkv * G)
    pk, pv = (cm.poisoned(x, lens, nan=f8.NAN_CODES[0]) for x in (k8, v8))
    for out_same in (False, True):
        o, lse, need = _run(fa, torch_cuda, dq, pk, pv, lens, ps, seed=ps + d + 1, k_scale=ks, v_scale=vs,
                            out_dtype=_tdtype(torch_cuda, fmt) if out_same else None)
        assert need == 0
        _check(oracle, o, lse, want, want_lse, fmt, f"fp8 single pass d={d} fmt={fmt} layout={ps} out_same={out_same}")
        if not out_same:   # weight exactly 1, and code * v_scale is one fp32 product on either side
            assert np.array_equal(o.cpu().numpy().reshape(want.shape)[:Hkv, 0], vd[:Hkv, 0]), "a sequence of one key must return v_scale * v[0]"


@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="p16"), pytest.param(128, id="p128")])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_mask_and_degenerate_rows(fa, oracle, torch_cuda, fmt, d, causal, ps):
    """Lengths 0, 2, 66 and the capacity with five query rows in two folded heads (tests/test_gpu_kvcache_paged.py, same name).
    Under the mask: length 66 puts keys 64-65 in a tile only rows 3 and 4 see, length 2 leaves rows 0-2 without a key, length 0
    leaves every row (and, paged, the whole table row: all garbage) without one."""
    B, Hkv, G, Nq, Ncap, lens = 4, 1, 2, 5, 1024, (0, 2, 66, 1024)
    _, qb, k8, v8, _, _, ks, vs = _quantised_inputs(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2401)
    want, want_lse = _reference(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2401, lens, causal)
    dead = np.isinf(want_lse).reshape(B, Hkv * G, Nq)
    assert dead[0].all() and (dead[1].all(0).tolist() == [causal] * 3 + [False] * 2) and not dead[2:].any()
    dq = _q_dev(torch_cuda, qb, fmt, B, Hkv * G)
    o, lse, need = _run(fa, torch_cuda, dq, *(cm.poisoned(x, lens, nan=f8.NAN_CODES[0]) for x in (k8, v8)), lens, ps, seed=ps + d + 2, k_scale=ks,
                        v_scale=vs, causal=causal)
    assert need > 0
    _check(oracle, o, lse, want, want_lse, fmt, f"fp8 mask + degenerate rows d={d} fmt={fmt} layout={ps} causal={causal}")


@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="p16")])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_scale_zero_with_half_k_scale(fa, oracle, torch_cuda, fmt, d, causal, ps):
    """scale = 0 reaches the kernel as +-FLT_MIN; times k_scale = 0.5 that is below FLT_MIN, and a product flushed to 0 would meet the
    -inf of a masked key as 0 * -inf.  The clamp after the product keeps the rule: every visible key weighs the same, so O is
    v_scale * the mean of the visible V rows and lse = ln(their number) -- under the mask, at ragged lengths, with rows that see no
    key.  The weights are all exactly 1, so the usual bounds hold with room to spare."""
    B, Hkv, G, Nq, Ncap, lens = 4, 2, 2, 5, 1024, (0, 2, 66, 1021)
    _, qb, k8, v8, _, vd, _, vs = _quantised_inputs(fa, oracle, B, Hkv, G, Nq, Ncap, d, fmt, 2501)
    want, want_lse = cm.uniform_expected(vd, lens, B, Hkv, G, Nq, causal)
    dq = _q_dev(torch_cuda, qb, fmt, B, Hkv * G)
    for scale in (0.0, -0.0):
        o, lse, need = _run(fa, torch_cuda, dq, *(cm.poisoned(x, lens, nan=f8.NAN_CODES[0]) for x in (k8, v8)), lens, ps, seed=ps + d + 3,
                            k_scale=(0.5, 0.5), v_scale=vs, causal=causal, scale=scale)
        assert need > 0
        _check(oracle, o, lse, want.astype(np.float32), want_lse, fmt, f"fp8 scale {scale} d={d} fmt={fmt} layout={ps} causal={causal}")


def test_graph_replay_follows_table_lengths_and_scales(fa, torch_cuda):
    """One captured paged call; table, lengths, k_scale and v_scale are overwritten in place between replays.  Nothing on the host
    read any of them at capture time, so every replay equals the eager call bit for bit."""
    torch = torch_cuda
    B, Hkv, G, Nq, ps, max_pages, d = 2, 2, 1, 1, 16, 44, 64
    Ncap, num_pages = ps * max_pages, 2 * max_pages + 5
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.randn(B, Hkv * G, Nq, d, generator=g, device="cuda").half()
    k0, ks0 = fa.quantize_kv_fp8(torch.randn(B, Hkv, Ncap, d, generator=g, device="cuda"))
    v0, vs0 = fa.quantize_kv_fp8(torch.randn(B, Hkv, Ncap, d, generator=g, device="cuda"))
    k0, v0 = k0.view(torch.uint8), v0.view(torch.uint8)
    kp, vp = (torch.empty(num_pages, Hkv, ps, d, dtype=torch.uint8, device="cuda") for _ in range(2))
    table = torch.empty(B, max_pages, dtype=torch.int32, device="cuda")
    lens = torch.empty(B, dtype=torch.int32, device="cuda")
    ks, vs = torch.empty(Hkv, device="cuda"), torch.empty(Hkv, device="cuda")
    steps = (((704, 5), 1, (1.0, 3.0), (0.5, 1.5)), ((64, 699), 2, (2.5, 0.75), (7.0, 1.0)))

    def place(lengths, seed, kmul, vmul):
        """pools, table, lengths and scales rewritten IN PLACE: 0x7F everywhere but the live rows, garbage past the live entries"""
        perm = np.random.default_rng(seed).permutation(num_pages)
        kp.fill_(0x7F), vp.fill_(0x7F)
        tb = np.empty((B, max_pages), np.int32)
        nxt = 0
        for b, L in enumerate(lengths):
            for pi in range(max_pages):
                if pi >= di.live_pages(L, ps):
                    tb[b, pi] = cm.GARBAGE[pi % 2]
                    continue
                page, n = int(perm[nxt]), min(ps, L - pi * ps)
                nxt += 1
                tb[b, pi] = page
                kp[page, :, :n] = k0[b, :, pi * ps:pi * ps + n]
                vp[page, :, :n] = v0[b, :, pi * ps:pi * ps + n]
        table.copy_(torch.from_numpy(tb).cuda())
        lens.copy_(torch.tensor(lengths, dtype=torch.int32, device="cuda"))
        ks.copy_(ks0 * torch.tensor(kmul, device="cuda")), vs.copy_(vs0 * torch.tensor(vmul, device="cuda"))

    def call():
        return fa.fa_forward_kvcache_paged_fp8(q, kp.view(torch.float8_e4m3fn), vp.view(torch.float8_e4m3fn), table, ks, vs, lens,
                                               return_lse=True, workspace=ws)

    need = fa.kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, ps, d)
    assert need > 0
    ws = _nan_workspace(torch, need)
    eager = []
    for step in steps:
        place(*step)
        ws.fill_(0xFF)
        o, lse = call()
        eager.append((o.clone(), lse.clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    place((300, 300), 3, (1.0, 1.0), (1.0, 1.0))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = call()
    for step, (eo, el) in zip(steps, eager):
        place(*step)
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), step
        assert torch.equal(o, eo) and torch.equal(lse, el), step
