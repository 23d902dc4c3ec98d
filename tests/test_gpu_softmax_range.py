"""GPU tier of the wide-logit-range inputs (tests/softmax_range_inputs.py): the reference-maximum rescale of fa_mla_decode with its
private merge, and of the varlen prefill template behind fa_forward_varlen (plain, window, soft-cap, sinks), fa_forward_varlen_kvcache
(contiguous, paged), fa_forward_varlen_kvcache_fp8 and the prefill arm of fa_kvcache_attend_varlen.  The other tiers hold these
kernels against N(0,1) logits, under which a reference moves by a few log2 units at most; here rows climb a staircase of 7 per tile,
jump by 40 and by 150, fall by 210, and meet spikes the mask hides.  tests/test_softmax_range_inputs.py shows without a GPU that the
inputs force those events and that the check below rejects a model of the scheme with O or l not rescaled, a vote against the previous
tile, a maximum taken before the mask, a merge that ignores m or takes the first split's, and an lse written with a stale m.

References: mla_inputs.expected_f64 and varlen_logit_inputs.varlen_logits_f64 (float64 numpy on the rounded inputs).  Bounds, fixed
before any run: softmax_range_inputs.bounds -- fp16 cm.MAX_ABS and cm.REL_L2, bf16 cm.peaked_tol and 3e-2 (the peaked rule of
test_gpu_fallback_paths.py), rel-L2 x 1.5 for a 16-bit output -- 2 * cm.P_EPS absolute on lse, rows without a key exactly 0 / -inf; the
fp8 case keeps test_gpu_varlen_cache_fp8.py's (vi.problems).  Two of our kernels are compared bit for bit.

Poison as in test_gpu_mla.py and test_gpu_varlen.py: workspaces NaN-filled, O and lse sentinel-filled, caches NaN at and past every
length, pool pages no table names NaN, Q / K / V rows of no sequence NaN.  Every test prints RANGE|entry|case|max_abs|rel_l2|lse_abs.
"""
import numpy as np
import pytest

import common_inputs as cm
import softmax_range_inputs as sr
import test_gpu_mla as tgm
import varlen_cache_fp8_inputs as v8
import varlen_cache_inputs as ci
import varlen_inputs as vi

pytestmark = pytest.mark.gpu

FMTS = [pytest.param(fmt, id=cm.FMT_NAME[fmt]) for fmt in sr.FMTS]
MASKS = [pytest.param(True, id="causal"), pytest.param(False, id="full")]
NCAP, PAGE = 512, 16


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _i32(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.int32)).cuda()


def _f32(torch, x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.float32)).cuda()


def _np(t):
    return t.float().cpu().numpy()


def _tdt(torch, fmt):
    return torch.bfloat16 if fmt else torch.float16


def _same(torch, a, b, what):
    for x, y, n in zip(a, b, ("O", "lse")):
        assert torch.equal(tgm._bits(torch, x), tgm._bits(torch, y)), f"{what}: {n} differs"


# ---- 1. fa_mla_decode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sr.MLA_SPLITS)
@pytest.mark.parametrize("causal", MASKS)
@pytest.mark.parametrize("fmt", FMTS)
def test_mla_decode(fa, oracle, torch_cuda, fmt, causal, S):
    """one pass, two and three splits, as many splits as the capacity has 64-key units, and the library's choice: fp32 output against
    the float64 reference, the same-type output the rounded fp32 bits, the paged cache (pages of 16) the contiguous cache's bits"""
    torch = torch_cuda
    f, lay = sr.MLA, sr.mla_layout()
    q = cm.dev16(torch, sr.mla_packed_q_bits(fmt), fmt)
    cache = cm.dev16(torch, sr.mla_poisoned_cache(fmt), fmt)
    assert torch.isnan(cache[0, f["lens"][0]:]).all() and torch.isnan(q[~torch.from_numpy(lay.owned).cuda()]).all()
    cu, lens = tgm._ints(torch, lay.cu), tgm._ints(torch, f["lens"])
    o, lse = tgm._run(fa, torch, q, cache, cu, f["max_q"], lens, None, f["Hq"], causal=causal, S=S)
    want, want_lse = sr.mla_reference(fmt, causal)
    sr.check_packed(oracle, lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, sr.mla_vmax(fmt), "fa_mla_decode",
                    f"{cm.FMT_NAME[fmt]} causal={int(causal)} S={S}")
    o16, lse16 = tgm._run(fa, torch, q, cache, cu, f["max_q"], lens, None, f["Hq"], causal=causal, S=S, out_dtype=_tdt(torch, fmt))
    tgm._check_16bit(torch, lay, o16, lse16, o, lse, f"S={S} causal={causal}")
    pool, table = sr.mla_paged_cache(fmt, PAGE)
    got = tgm._run(fa, torch, q, cm.dev16(torch, pool, fmt), cu, f["max_q"], lens, torch.from_numpy(table).cuda(), f["Hq"], causal=causal, S=S)
    _same(torch, got, (o, lse), f"pages of {PAGE}, S={S} causal={causal}")


# ---- 2. the varlen prefill ---------------------------------------------------------------------------------------------------------------
def _poisoned_out(torch, c, out_same):
    tq, Hq, d = c["q"].shape
    tdt = _tdt(torch, c["fmt"]) if out_same else torch.float32
    return (torch.full((tq, Hq, d), vi.POISON, dtype=tdt, device="cuda"), torch.full((Hq, tq), vi.POISON, dtype=torch.float32, device="cuda"))


def _opts(torch, c, causal):
    return dict(causal=causal, scale=c["scale"], window=c["W"], softcap=c["softcap"], sinks=_f32(torch, c["sinks"]))


def _packed(torch, fa, c, causal, out_same=False):
    q, k, v = (cm.dev16(torch, c[n], c["fmt"]) for n in ("qb", "kb", "vb"))
    assert torch.isnan(q[-vi.TAIL:]).all() and torch.isnan(k[-vi.TAIL:]).all() and torch.isnan(v[-vi.TAIL:]).all()
    out, lse = _poisoned_out(torch, c, out_same)
    fa.fa_forward_varlen(q, k, v, _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"]), out=out, lse=lse, **_opts(torch, c, causal))
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("causal", MASKS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
@pytest.mark.parametrize("feature", sr.FEATURES)
def test_forward_varlen(fa, torch_cuda, feature, d, fmt, causal):
    """the plain case and one case per logit feature, fp32 and 16-bit output"""
    c = sr.varlen_case(d, fmt, feature)
    want, want_lse = sr.varlen_reference(d, fmt, feature, causal)
    for out_same in (False, True):
        o, lse = _packed(torch_cuda, fa, c, causal, out_same)
        sr.check_varlen(c, _np(o), _np(lse), want, want_lse, "fa_forward_varlen",
                        f"d{d} {cm.FMT_NAME[fmt]} {feature} causal={int(causal)} o16={int(out_same)}", out_same)


def _cache_run(torch, fa, c, kc, vc, lens, table, causal, out_same=False):
    q = cm.dev16(torch, c["qb"], c["fmt"])
    out, lse = _poisoned_out(torch, c, out_same)
    fa.fa_forward_varlen_kvcache(q, kc, vc, _i32(torch, c["cu_q"]), _i32(torch, lens), block_table=table, out=out, lse=lse,
                                 **_opts(torch, c, causal))
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
@pytest.mark.parametrize("feature", sr.FEATURES)
def test_forward_varlen_kvcache(fa, torch_cuda, feature, d, fmt):
    """the same keys laid into a contiguous cache (NaN at and past every length): the packed entry's bits, as
    test_gpu_varlen_cache.py::test_bits_of_the_packed_entry requires of every case; pages of 16 (pages wholly below the window freed,
    garbage in the table entries nothing may read): the contiguous form's bits"""
    torch = torch_cuda
    c = sr.varlen_case(d, fmt, feature)
    kc, vc, lens = sr.varlen_cache(c, NCAP)
    kp, vp, table = ci.scatter(kc, vc, c["lk"], ci.lo0_of(c["lq"], c["lk"], c["W"]), PAGE, seed=9500 + d)
    for causal in (True, False):
        ref = _packed(torch, fa, c, causal)
        got = _cache_run(torch, fa, c, cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt), lens, None, causal)
        want, want_lse = sr.varlen_reference(d, fmt, feature, causal)
        sr.check_varlen(c, _np(got[0]), _np(got[1]), want, want_lse, "fa_forward_varlen_kvcache", f"d{d} {cm.FMT_NAME[fmt]} {feature} causal={int(causal)}")
        _same(torch, got, ref, f"contiguous cache against the packed entry, causal={causal}")
        paged = _cache_run(torch, fa, c, cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), lens, _i32(torch, table), causal)
        _same(torch, paged, got, f"pages of {PAGE} against the contiguous cache, causal={causal}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
def test_forward_varlen_kvcache_fp8(fa, torch_cuda, d, fmt):
    """the plain case quantised to e4m3fn codes with one scale per K/V head: every jump still lies more than 21 log2 units above its
    row's benign scores on the decoded codes; against the float64 reference on those codes at the fp8 tier's bounds (vi.problems),
    contiguous and in pages of 16"""
    torch = torch_cuda
    c = dict(sr.varlen_fp8_case(d, fmt), causal=True, f32=True)
    assert all(got > sr.FP8_MIN_LIFT for (_, _, _, _, lift, got, _) in c["spikes"] if lift >= 40.0)
    want, want_lse = v8.reference_f64(c)
    kc, vc, lens = sr.varlen_fp8_cache(c, NCAP)
    q = cm.dev16(torch, c["qb"], fmt)
    own = vi.owned(c["cu_q"], q.shape[0])
    results = []
    for ps in (0, PAGE):
        k8, v8c, table = (kc, vc, None) if ps == 0 else v8.scatter(kc, vc, c["lk"], [0, 0], ps, seed=9600 + d)
        out, lse = _poisoned_out(torch, c, False)
        fa.fa_forward_varlen_kvcache_fp8(q, cm.dev8(torch, k8), cm.dev8(torch, v8c), _i32(torch, c["cu_q"]), _i32(torch, lens),
                                         block_table=None if table is None else _i32(torch, table), k_scale=_f32(torch, c["k_scale"]),
                                         v_scale=_f32(torch, c["v_scale"]), out=out, lse=lse, **_opts(torch, c, True))
        torch.cuda.synchronize()
        got, got_lse = _np(out), _np(lse)
        ma, rl, le = vi.figures(got, got_lse, want, want_lse, own)
        print(f"RANGE|fa_forward_varlen_kvcache_fp8|d{d} {cm.FMT_NAME[fmt]} causal=1 page={ps}|{ma:.3e}|{rl:.3e}|{le:.3e}   "
              f"(bounds {cm.MAX_ABS:.1e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
        found = vi.problems(got, got_lse, want, want_lse, own, fmt)
        assert not found, f"fp8 d{d} page={ps}: {found}"
        results.append((out, lse))
    _same(torch, results[1], results[0], f"fp8 pages of {PAGE} against the contiguous cache")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
def test_attend_varlen_prefill_arm(fa, torch_cuda, d, fmt):
    """split_rows = 8: the (130, 421) sequence takes the tiled kernel, the (5, 66) one the split-KV stream.  The long sequence's rows
    are fa_forward_varlen_kvcache's bits; the whole result stays inside the bounds"""
    torch = torch_cuda
    T = 8
    c = sr.varlen_case(d, fmt, "plain")
    assert c["lq"][1] <= T < c["lq"][0]
    kc, vc, lens = sr.varlen_cache(c, NCAP)
    dk, dv_ = cm.dev16(torch, kc, fmt), cm.dev16(torch, vc, fmt)
    ref = _cache_run(torch, fa, c, dk, dv_, lens, None, True)
    out, lse = _poisoned_out(torch, c, False)
    need = fa.kvcache_decode_varlen_workspace_bytes(len(c["lq"]), c["Hkv"], c["G"], T, d, Ncap=NCAP)
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN
    fa.fa_kvcache_attend_varlen(cm.dev16(torch, c["qb"], fmt), dk, dv_, _i32(torch, c["cu_q"]), _i32(torch, lens), None, split_rows=T,
                                scale=c["scale"], out=out, lse=lse, workspace=ws)
    torch.cuda.synchronize()
    n0 = c["lq"][0]
    _same(torch, (out[:n0], lse[:, :n0]), (ref[0][:n0], ref[1][:, :n0]), "the prefill arm against fa_forward_varlen_kvcache")
    want, want_lse = sr.varlen_reference(d, fmt, "plain", True)
    sr.check_varlen(c, _np(out), _np(lse), want, want_lse, "fa_kvcache_attend_varlen", f"d{d} {cm.FMT_NAME[fmt]} split_rows={T}")
