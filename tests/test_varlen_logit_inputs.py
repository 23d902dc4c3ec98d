"""CPU tier of the windowed / soft-capped / sink varlen prefill tests: what shows that tests/test_gpu_varlen_logits.py can fail for the
right reasons.  The float64 restatement of tests/varlen_logit_inputs.py equals tests/varlen_inputs.py's with every option off, agrees
with a per-row brute force and with the decode reference per sequence; a kernel that ignores an option, and nine wrong kernels
restated in numpy, each miss a bound the GPU test applies, on a named row.  No GPU."""
import numpy as np
import pytest

import common_inputs as cm
import varlen_inputs as vi
import varlen_logit_inputs as li


def test_all_options_off_is_the_base_reference():
    for case in (vi.CASES[0], vi.CASES[4], vi.CASES[7], vi.CASES[12]):
        c = vi.make(case)
        want, want_lse = vi.expected(case)
        o, lse = li.varlen_logits_f64(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["Hkv"], c["G"], c["causal"], c["scale"])
        # the same sums in another order of operations (a matrix product per head, not a dot product per row): a few ulps
        assert np.abs(o - want).max() <= 1e-13 and (np.isfinite(lse) == np.isfinite(want_lse)).all()
        live = np.isfinite(want_lse)
        assert np.abs(lse[live] - want_lse[live]).max() <= 1e-13
        # ... and on the rows without a key, and of no sequence, exactly
        assert (o[~live.T] == want[~live.T]).all()


def _brute(c):
    """row by row: every key of the sequence gets a logit or -inf, the sink is one more column with a zero V row"""
    q, k, v = c["q"], c["k"], c["v"]
    Hq = c["Hkv"] * c["G"]
    out = np.zeros(q.shape, np.float64)
    lse = np.full((Hq, q.shape[0]), -np.inf)
    for (sq, eq), (sk, ek) in zip(vi.bounds(c["cu_q"], q.shape[0]), vi.bounds(c["cu_k"], k.shape[0])):
        Lq, Lk = eq - sq, ek - sk
        for i in range(Lq):
            pos = Lk - Lq + 1 + i
            hi = max(0, pos) if c["causal"] else Lk
            lo = max(0, pos - c["W"]) if c["W"] else 0
            for hq in range(Hq):
                hk = hq // c["G"]
                t = np.full(Lk + 1, -np.inf)
                for j in range(lo, hi):
                    s = float(np.dot(q[sq + i, hq].astype(np.float64), k[sk + j, hk].astype(np.float64))) * c["scale"]
                    t[j] = c["softcap"] * np.tanh(s / c["softcap"]) if c["softcap"] else s
                if c["sinks"] is not None:
                    t[Lk] = float(c["sinks"][hq])
                if not np.isfinite(t.max()):
                    continue
                w = np.exp(t - t.max())
                vv = np.concatenate([v[sk:ek, hk].astype(np.float64), np.zeros((1, q.shape[2]))])
                out[sq + i, hq] = (w[w > 0] / w.sum()) @ vv[w > 0]
                lse[hq, sq + i] = t.max() + np.log(w.sum())
    return out, lse


@pytest.mark.parametrize("case", (li.CASES[3], li.CASES[6], li.CASES[15]), ids=li.case_id)
def test_restatement_is_the_brute_force(case):
    c = li.make(case)
    want, want_lse = li.expected(case)
    o, lse = _brute(c)
    assert not np.isnan(want).any() and not np.isnan(want_lse).any()      # the NaN tails of Q, K and V are never used
    assert np.abs(o - want).max() <= 1e-12 and (np.isfinite(lse) == np.isfinite(want_lse)).all()
    live = np.isfinite(lse)
    assert np.abs(lse[live] - want_lse[live]).max() <= 1e-12


@pytest.mark.parametrize("case", li.CASES, ids=li.case_id)
def test_restatement_is_the_decode_reference_per_sequence(case):
    """cm.expected_f64 -- the reference of the decode tier, whose semantics the entry takes word for word -- with Lq in the place of Nq"""
    c = li.make(case)
    want, want_lse = li.expected(case)
    for (sq, eq), (sk, ek) in zip(vi.bounds(c["cu_q"], c["q"].shape[0]), vi.bounds(c["cu_k"], c["k"].shape[0])):
        if eq == sq or ek == sk:
            continue
        qb, kb, vb = (np.ascontiguousarray(x.transpose(1, 0, 2)) for x in (c["q"][sq:eq], c["k"][sk:ek], c["v"][sk:ek]))
        o, lse = cm.expected_f64(qb, kb, vb, [ek - sk], 1, c["Hkv"], c["G"], eq - sq, c["causal"], c["W"], scale=c["scale"],
                                 softcap=c["softcap"], sinks=c["sinks"])
        assert np.abs(want[sq:eq].transpose(1, 0, 2) - o).max() <= 1e-12
        got = want_lse[:, sq:eq]
        assert (np.isfinite(got) == np.isfinite(lse)).all()
        live = np.isfinite(lse)
        assert np.abs(got[live] - lse[live]).max(initial=0.0) <= 1e-12


def _rejected(c, want, want_lse, o, lse):
    own = vi.owned(c["cu_q"], c["q"].shape[0])
    return vi.problems(o, lse, want, want_lse, own, c["fmt"])


@pytest.mark.parametrize("case", li.CASES, ids=li.case_id)
def test_a_dropped_option_misses_a_bound(case):
    c = li.make(case)
    want, want_lse = li.expected(case)
    base = (vi.POISON, vi.POISON)
    right = li.run_f64(c, base=base)
    assert _rejected(c, want, want_lse, *right) == []
    assert li.dropped(c)
    for name, over in li.dropped(c):
        found = _rejected(c, want, want_lse, *li.run_f64(c, base=base, **over))
        print(li.case_id(case), "without", name, found)
        assert found and all("row" in f for f in found), (name, found)


def _differs(c, wrong):
    """can the wrong kernel differ from the entry on this case: does any row see other keys, or another sink weight"""
    if wrong in ("no_window", "lo_low", "lo_high", "lo_start", "t0_last"):
        if not c["W"]:
            return False
        for Lq, Lk in zip(c["lq"], c["lk"]):
            (lo, hi), (lo2, hi2) = li.limits(Lq, Lk, c["causal"], c["W"]), li.limits(Lq, Lk, c["causal"], c["W"], wrong)
            assert (hi == hi2).all()
            if ((np.where(lo < hi, lo, hi) != np.where(lo2 < hi, lo2, hi))).any():   # an empty range is [hi, hi) in both
                return True
        return False
    if wrong == "cap_after":      # some key of a sequence is masked for some row
        return c["softcap"] > 0 and any(((hi - lo) < Lk).any() for Lq, Lk in zip(c["lq"], c["lk"]) if Lq
                                        for lo, hi in [li.limits(Lq, Lk, c["causal"], c["W"])])
    if c["sinks"] is None:
        return False
    if wrong == "sink_per_tile":  # some row's visible keys lie in two tiles or more
        return any(((hi > lo) & ((np.maximum(hi, 1) - 1) // li.TILE > lo // li.TILE)).any() for Lq, Lk in zip(c["lq"], c["lk"]) if Lq
                   for lo, hi in [li.limits(Lq, Lk, c["causal"], c["W"])])
    return True                   # sink_scaled (no case has scale 1), sink_dead (every case has tail rows)


@pytest.mark.parametrize("case", li.CASES, ids=li.case_id)
def test_wrong_kernels_miss_a_bound(case):
    """the GPU test's check (vi.problems) rejects every wrong implementation that can differ from the entry on this case, naming a row"""
    c = li.make(case)
    want, want_lse = li.expected(case)
    base = (vi.POISON, vi.POISON)
    for wrong in li.WRONG:
        if not _differs(c, wrong):
            continue
        found = _rejected(c, want, want_lse, *li.run_f64(c, wrong=wrong, base=base))
        print(li.case_id(case), wrong, found)
        assert found and all("row" in f for f in found), (wrong, found)


def test_every_wrong_kernel_is_covered_at_each_head_dim():
    cs = [li.make(case) for case in li.CASES]
    for wrong in li.WRONG:
        for d in (64, 128):
            assert any(_differs(c, wrong) for c in cs if c["d"] == d), (wrong, d)
    assert {c["d"] for c in cs} == {64, 128} and {c["fmt"] for c in cs} == {0, 1} and {c["causal"] for c in cs} == {False, True}
    assert {c["f32"] for c in cs} == {False, True} and {c["W"] for c in cs} == {0} | set(li.WINDOWS) == {0, 1, 17, 64, 100}
    assert li.BATCHES["self"] == (vi.LQ, vi.LQ) and li.BATCHES["cross"] == (vi.LQ, vi.LK2) and li.BATCHES["long"] == ((449, 130), (449, 513))
    assert vi.LQ == (1, 63, 65, 0, 129, 257) and len(li.CASES) == 16 and sum(c["scale"] < 0 for c in cs) == 1
    for Hq in (3, 4):                                    # a mixed vector: finite values and -inf
        s = li.sinks_for(Hq)
        assert np.isfinite(s).any() and np.isinf(s).any()


def test_the_long_batch_reaches_the_tile_skips():
    """W = 64, causal, the 449-row sequence: its last workgroup starts at tile 5, and in the block of rows 128..255 the first wave
    computes tile 1, which the last wave skips; at W = 17 the first wave's last tile lies below the last wave's first"""
    Lq, Lk, W = 449, 449, 64
    lo, c = li.limits(Lq, Lk, True, W)
    assert lo[384] // li.TILE == 5 and lo[128] // li.TILE == 1 and lo[128 + 96] // li.TILE == 2
    lo, c = li.limits(Lq, Lk, True, 17)
    assert (c[128 + 31] - 1) // li.TILE < lo[128 + 96] // li.TILE
    # W = 1: every causal row sees exactly its own key
    lo, c = li.limits(Lq, Lk, True, 1)
    assert (c - lo == 1).all() and (lo == np.arange(Lq)).all()
    # lo_i < c_i whenever c_i >= 1, with and without the mask, on every batch
    for lq, lk in li.BATCHES.values():
        for a, b in zip(lq, lk):
            for causal in (False, True):
                for W in li.WINDOWS:
                    lo, c = li.limits(a, b, causal, W)
                    assert ((lo < c) | (c == 0)).all()
