"""CPU tier of tests/varlen_cache_fp8_inputs.py: the float64 reference of fa_forward_varlen_kvcache_fp8 equals a brute-force loop; the
kernel's reads restated (gather + attend) pass the check of the GPU tier on every case; and each of the seven wrong kernels is rejected
by that same check on at least one parity case, at pages of 16 and of 128 -- a condition on the chosen scales and data, asserted here
so that the GPU tier cannot pass on such a kernel.  No GPU."""
import numpy as np
import pytest

import common_inputs as cm
import fp8_inputs as f8
import varlen_cache_fp8_inputs as v8
import varlen_inputs as vi
import varlen_logit_inputs as li

BASE = (vi.POISON, vi.POISON)


def _found(case, got):
    c = v8.make(case)
    want, want_lse = v8.expected(case)
    return vi.problems(got[0], got[1], want, want_lse, vi.owned(c["cu_q"], c["q"].shape[0]), c["fmt"])


def test_scales_and_poison():
    for Hkv in (1, 2, 3):
        ks, vs = v8.scales_for(Hkv)
        both = np.concatenate([ks, vs])
        assert (both > 0).all() and (both != 1.0).all() and len(set(both.tolist())) == both.size
    for case in v8.CASES:
        c = v8.make(case)
        lo0 = v8.lo0_of(c["lq"], c["lk"], c["W"])
        for cache in (c["kc"], c["vc"]):
            for b, Lk in enumerate(c["lk"]):
                assert (cache[b, :, :lo0[b]] == v8.NAN8).all() and (cache[b, :, Lk:] == v8.NAN8).all()
                assert not np.isin(cache[b, :, lo0[b]:Lk], f8.NAN_CODES).any()
        for ps in (16, 128):
            kp, vp, table = v8.paged(case, ps)
            named = set(int(p) for p in table.reshape(-1) if 0 <= p < kp.shape[0])
            for page in range(kp.shape[0]):
                if page not in named:
                    assert (kp[page] == v8.NAN8).all() and (vp[page] == v8.NAN8).all()
            assert set(table.reshape(-1).tolist()) - named <= set(cm.GARBAGE)


def test_the_cases_cover_the_ground():
    cs = v8.CASES
    assert {c[3] for c in cs} == {64, 128} and {c[4] for c in cs} == {0, 1} and {c[6] for c in cs} == {0, 1}
    assert {c[5] for c in cs} == {0, 1} and any(c[7] is not None and c[7] < 0 for c in cs)
    assert {c[8] for c in cs} == {0, 1, 17, 100, 400}
    assert {(c[9], c[10]) for c in cs if c[8] == 0} >= {(0, 0), (1, 0), (0, 1)} and any(c[9] and c[10] for c in cs)
    assert {c[0] for c in cs} == {"chunk", "short"}


def test_reference_equals_brute_force():
    """row by row, key by key, on one case with a window, the cap and sinks"""
    case = v8.CASES[8]
    c = v8.make(case)
    want, want_lse = v8.expected(case)
    G, cap = c["G"], c["softcap"]
    worst = 0.0
    for b, (sq, eq) in enumerate(vi.bounds(c["cu_q"], c["q"].shape[0])):
        Lq, Lk = eq - sq, c["lk"][b]
        for i in range(0, Lq, 7):
            pos = Lk - Lq + 1 + i
            hi = max(0, pos) if c["causal"] else Lk
            lo = max(0, pos - c["W"]) if c["W"] else 0
            for hq in range(c["Hkv"] * G):
                h = hq // G
                ts, rows = [], []
                for j in range(lo, hi):
                    kj = f8.decode(c["kc"][b, h, j]).astype(np.float64)
                    s = c["scale"] * float(c["k_scale"][h]) * float(kj @ c["q"][sq + i, hq].astype(np.float64))
                    ts.append(cap * np.tanh(s / cap) if cap else s)
                    rows.append(f8.decode(c["vc"][b, h, j]).astype(np.float64))
                a = float(c["sinks"][hq]) if c["sinks"] is not None else -np.inf
                m = max(ts + [a])
                if m == -np.inf:
                    assert (want[sq + i, hq] == 0).all() and want_lse[hq, sq + i] == -np.inf
                    continue
                den = sum(np.exp(t - m) for t in ts) + np.exp(a - m)
                o = float(c["v_scale"][h]) * sum((np.exp(t - m) / den * r for t, r in zip(ts, rows)), np.zeros(c["d"]))
                worst = max(worst, float(np.abs(o - want[sq + i, hq]).max()), abs(m + np.log(den) - want_lse[hq, sq + i]))
    assert worst < 1e-12, worst


@pytest.mark.parametrize("ps", (16, 128))
@pytest.mark.parametrize("case", v8.CASES, ids=v8.case_id)
def test_the_restated_kernel_passes(case, ps):
    assert _found(case, v8.run_paged(case, ps, None, BASE)) == []


@pytest.mark.parametrize("ps", (16, 128))
@pytest.mark.parametrize("wrong", v8.WRONG)
def test_every_wrong_kernel_is_rejected(wrong, ps):
    """on the first two cases (d = 64 fp16 and d = 128 bf16, the widest bounds) and on one with every option on"""
    rejected = [bool(_found(case, v8.run_paged(case, ps, wrong, BASE))) for case in (v8.CASES[0], v8.CASES[1], v8.CASES[8])]
    assert all(rejected), (wrong, ps, rejected)


def test_reference_is_li_run_f64_with_unit_scales():
    """with both scales 1 the reference is tests/varlen_logit_inputs.py's on the decoded codes, untouched"""
    c = v8.make(v8.CASES[5])
    ones = np.ones(c["Hkv"], np.float32)
    a = v8.reference_f64(c, ones, ones)
    b = li.run_f64(c)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
