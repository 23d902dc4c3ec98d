"""CPU tier of the variable-length prefill tests: what shows that tests/test_gpu_varlen.py can fail for the right reasons.  The float64
reference of tests/varlen_inputs.py agrees with the project's decode reference and with the oracle; five wrong kernels, restated in
numpy, each miss a bound the GPU test applies, on a named row; the block-slot arithmetic of the kernel holds.  No GPU."""
import numpy as np
import pytest

import common_inputs as cm
import varlen_inputs as vi

SOME = (vi.CASES[0], vi.CASES[4], vi.CASES[6], vi.CASES[7], vi.CASES[12])


def _per_sequence(c):
    """[(b, (sq, eq), (sk, ek), q_b [Hq, Lq, d], k_b, v_b [Hkv, Lk, d])] of a made case"""
    tq, tk = c["q"].shape[0], c["k"].shape[0]
    out = []
    for b, ((sq, eq), (sk, ek)) in enumerate(zip(vi.bounds(c["cu_q"], tq), vi.bounds(c["cu_k"], tk))):
        out.append((b, (sq, eq), (sk, ek), np.ascontiguousarray(c["q"][sq:eq].transpose(1, 0, 2)),
                    np.ascontiguousarray(c["k"][sk:ek].transpose(1, 0, 2)), np.ascontiguousarray(c["v"][sk:ek].transpose(1, 0, 2))))
    return out


@pytest.mark.parametrize("case", vi.CASES, ids=vi.case_id)
def test_reference_is_the_decode_reference_per_sequence(case):
    c = vi.make(case)
    want, want_lse = vi.expected(case)
    assert not np.isnan(want).any() and not np.isnan(want_lse).any()   # the NaN tails of Q, K and V are never used
    for b, (sq, eq), (sk, ek), qb, kb, vb in _per_sequence(c):
        if eq == sq:
            continue
        o, lse = cm.expected_f64(qb, kb, vb, [ek - sk], 1, c["Hkv"], c["G"], eq - sq, c["causal"], scale=c["scale"])
        assert np.abs(want[sq:eq].transpose(1, 0, 2) - o).max() <= 1e-12, b
        got = want_lse[:, sq:eq]
        assert (np.isfinite(got) == np.isfinite(lse)).all(), b
        live = np.isfinite(lse)
        assert np.abs(got[live] - lse[live]).max(initial=0.0) <= 1e-12, b
    own = vi.owned(c["cu_q"], c["q"].shape[0])
    assert (want[~own] == 0).all() and (want_lse[:, ~own] == -np.inf).all() and (~own).sum() == vi.TAIL


@pytest.mark.parametrize("case", SOME, ids=vi.case_id)
def test_reference_is_the_oracle_on_the_visible_keys(oracle, case):
    c = vi.make(case)
    want, want_lse = vi.expected(case)
    for b, (sq, eq), (sk, ek), qb, kb, vb in _per_sequence(c):
        if eq == sq:
            continue
        o, lse = cm.expected(oracle, qb, kb, vb, [ek - sk], 1, c["Hkv"], c["G"], eq - sq, c["causal"], scale=c["scale"])
        # the oracle returns fp32 from float64 accumulators: half an ulp of values below 8, plus its own exp
        assert np.abs(want[sq:eq].transpose(1, 0, 2) - o).max() <= 2e-6, b
        live = np.isfinite(lse)
        assert (np.isfinite(want_lse[:, sq:eq]) == live).all(), b
        assert np.abs(want_lse[:, sq:eq][live] - lse[live]).max(initial=0.0) <= 1e-9, b


def _applies(wrong, c):
    if wrong == "start":
        return c["causal"] and any(a != b for a, b in zip(c["lq"], c["lk"]) if a)
    if wrong == "head_mod":
        return c["Hkv"] > 1 and c["G"] > 1      # hq % Hkv == hq // G for every head otherwise
    return True


@pytest.mark.parametrize("case", vi.CASES, ids=vi.case_id)
def test_wrong_kernels_miss_a_bound(case):
    """the GPU test's check (vi.problems) rejects every wrong implementation that differs from the entry on this case, and names the row"""
    c = vi.make(case)
    want, want_lse = vi.expected(case)
    own = vi.owned(c["cu_q"], c["q"].shape[0])
    base = (vi.POISON, vi.POISON)
    right = vi.varlen_f64(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["Hkv"], c["G"], c["causal"], c["scale"], base=base)
    assert vi.problems(right[0], right[1], want, want_lse, own, c["fmt"]) == []
    for wrong in vi.WRONG:
        if not _applies(wrong, c):
            continue
        with np.errstate(invalid="ignore"):
            o, lse = vi.varlen_f64(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["Hkv"], c["G"], c["causal"], c["scale"], wrong=wrong,
                                   base=base)
        found = vi.problems(o, lse, want, want_lse, own, c["fmt"])
        print(vi.case_id(case), wrong, found)
        assert found and all("row" in f for f in found), (wrong, found)


def test_every_wrong_kernel_is_covered():
    for wrong in vi.WRONG:
        assert any(_applies(wrong, vi.make(case)) for case in vi.CASES), wrong
    cs = [vi.make(case) for case in vi.CASES]
    assert {(c["Hkv"], c["G"]) for c in cs} == {(2, 2), (1, 4), (3, 1)} and {c["d"] for c in cs} == {64, 128}
    assert {c["fmt"] for c in cs} == {0, 1} and {c["causal"] for c in cs} == {False, True} and {c["f32"] for c in cs} == {False, True}
    assert sum(c["scale"] < 0 for c in cs) == 1
    assert vi.LQ == (1, 63, 65, 0, 129, 257) and vi.LK2 == (1, 200, 65, 5, 70, 300) and vi.BATCHES["one"] == ((64,), (64,))
    for fmt in (0, 1):                                  # the poison is exact in every output type
        assert vi.decode16(vi.encode16(np.float32([vi.POISON]), fmt), fmt)[0] == vi.POISON


def test_slot_arithmetic():
    """sequence b owns [first_b, first_{b+1}) with at least ceil(Lq_b / BM) slots, and all of them lie inside the grid"""
    rng = np.random.default_rng(5)
    for trial in range(200):
        B = int(rng.integers(1, 12))
        lens = rng.integers(0, 700, B) * (rng.random(B) > 0.2)
        cu = vi.cu_of(lens) + int(rng.integers(0, 300))          # a first entry above 0 too
        total_q = int(cu[-1]) + int(rng.integers(0, 200))
        if trial % 5 == 0:
            total_q = max(int(cu[-1]) - int(rng.integers(0, 400)), 1)   # ... and vectors that overrun the tensor: clamped
        for bm in (64, 128, 256):
            for b, (s, e) in enumerate(vi.bounds(cu, total_q)):
                have = vi.first_slot(cu, total_q, b + 1, bm) - vi.first_slot(cu, total_q, b, bm)
                assert have >= -(-(e - s) // bm), (trial, bm, b)
            assert vi.first_slot(cu, total_q, B, bm) <= vi.num_slots(total_q, B, bm), (trial, bm)
