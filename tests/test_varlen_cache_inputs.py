"""CPU tier of the varlen-prefill-against-the-KV-cache tests: what shows that tests/test_gpu_varlen_cache.py can fail for the right
reasons.  The kernel's addressing restated on the laid-out pools (tests/varlen_cache_inputs.py) gives the reference of the gathered
keys for every page size, although the pools hold NaN in every row and page no visible key lies in and garbage in every table entry
nothing may read; six wrong kernels restated in numpy each miss a bound the GPU test applies, on a named row; the cases reach a
page boundary inside a tile, a freed page and a window across the prefix boundary.  No GPU."""
import numpy as np
import pytest

import common_inputs as cm
import varlen_cache_inputs as ci
import varlen_inputs as vi
import varlen_logit_inputs as li


def _rejected(c, want, want_lse, o, lse):
    own = vi.owned(c["cu_q"], c["q"].shape[0])
    return vi.problems(o, lse, want, want_lse, own, c["fmt"])


@pytest.mark.parametrize("case", ci.CASES, ids=ci.case_id)
def test_reference_is_accepted_through_every_page_size(case):
    """the right addressing on the poisoned pools reads exactly the gathered keys: the check passes, and nothing NaN or garbage is seen"""
    c = ci.make(case)
    want, want_lse = ci.expected(case)
    assert not np.isnan(want).any() and not np.isnan(want_lse).any()
    base = (vi.POISON, vi.POISON)
    for ps in ci.PAGE_SIZES:
        o, lse = ci.run_paged(case, ps, base=base)
        assert _rejected(c, want, want_lse, o, lse) == [], ps
        own = vi.owned(c["cu_q"], c["q"].shape[0])
        assert np.abs(o[own] - want[own]).max(initial=0.0) <= 1e-12, ps


def test_attend_is_the_logit_reference():
    """attend_f64 on the packed keys cut per sequence is li.varlen_logits_f64, to rounding"""
    for case in (ci.CASES[0], ci.CASES[6], ci.CASES[13], ci.CASES[16]):
        c = ci.make(case)
        want, want_lse = ci.expected(case)
        seqs = [(c["k"][s:e], c["v"][s:e]) for s, e in vi.bounds(c["cu_k"], c["k"].shape[0] - vi.TAIL)]
        o, lse = ci.attend_f64(c, seqs)
        assert np.abs(o - want).max() <= 1e-12 and (np.isfinite(lse) == np.isfinite(want_lse)).all()
        live = np.isfinite(lse)
        assert np.abs(lse[live] - want_lse[live]).max() <= 1e-12


def _can_differ(c, ps, wrong):
    """can the wrong kernel read other keys than the entry on this case and page size"""
    live = [(Lq, Lk) for Lq, Lk in zip(c["lq"], c["lk"]) if Lq and Lk]
    if wrong == "len_excl":
        return True                                           # every batch has a row whose chunk tokens are keys
    if wrong == "page_pitch":
        return True                                           # every sequence but the first reads another row of the table
    if wrong == "row_in_page":
        return ps != cm.TILE and any(Lk > min(ps, cm.TILE) for _, Lk in live)
    if wrong == "tile_one_page":
        return ps < cm.TILE and any(Lk > ps for _, Lk in live)
    if wrong == "head_in_page":
        return c["Hkv"] > 1
    if wrong == "lo_prefix":                                  # some row's window reaches below the prefix boundary
        return bool(c["W"]) and any((li.limits(Lq, Lk, c["causal"], c["W"])[0] < Lk - Lq).any() for Lq, Lk in live)
    raise AssertionError(wrong)


@pytest.mark.parametrize("wrong", ci.WRONG)
def test_wrong_kernels_miss_a_bound(wrong):
    """the GPU test's check (vi.problems) rejects every wrong kernel wherever it can differ from the entry, naming a row; each wrong
    kernel is rejected on a case of either head dimension"""
    base = (vi.POISON, vi.POISON)
    hit = set()
    for case in ci.CASES:
        c = ci.make(case)
        want, want_lse = ci.expected(case)
        for ps in ci.PAGE_SIZES:
            if not _can_differ(c, ps, wrong):
                continue
            found = _rejected(c, want, want_lse, *ci.run_paged(case, ps, wrong=wrong, base=base))
            print(ci.case_id(case), ps, wrong, found)
            assert found and all("row" in f or "rel_l2" in f for f in found), (ci.case_id(case), ps, wrong, found)
            hit.add(c["d"])
    assert hit == {64, 128}, (wrong, hit)


def test_cases_cover_what_the_issue_names():
    cs = [ci.make(case) for case in ci.CASES]
    assert ci.LQ == (1, 63, 65, 0, 129, 257) and ci.PREFIX == (0, 200, 15, 5, 70, 300) and ci.NCAP == 640
    assert ci.BATCHES["chunk"][1] == tuple(p + n for p, n in zip(ci.PREFIX, ci.LQ))
    assert ci.PAGE_SIZES == (16, 32, 64, 128) and all(ci.NCAP % ps == 0 for ps in ci.PAGE_SIZES)
    lq, lk = ci.BATCHES["short"]
    assert any(Lk < Lq for Lq, Lk in zip(lq, lk)) and any(Lk == 0 and Lq > 0 for Lq, Lk in zip(lq, lk))
    assert {c["d"] for c in cs} == {64, 128} and {c["fmt"] for c in cs} == {0, 1} and {c["f32"] for c in cs} == {False, True}
    assert {(c["Hkv"], c["G"]) for c in cs} == {(2, 2), (1, 4), (3, 1)} and {c["causal"] for c in cs} == {False, True}
    assert {c["W"] for c in cs} == set(ci.WINDOWS) == {0, 1, 17, 64, 100, 400}
    assert any(c["softcap"] for c in cs) and any(c["sinks"] is not None for c in cs) and sum(c["scale"] < 0 for c in cs) == 2
    assert max(max(lk) for _, lk in ci.BATCHES.values()) <= ci.NCAP


@pytest.mark.parametrize("case", ci.CASES, ids=ci.case_id)
def test_every_case_has_a_page_boundary_inside_a_tile(case):
    """for ps < 64 some sequence of the case has visible keys on both sides of a page boundary that is no tile boundary: a streamed
    tile takes rows that count from two pages (under W = 1 no single row sees both sides, the tile still holds both)"""
    c = ci.make(case)
    for ps in (16, 32):
        ok = False
        for Lq, Lk in zip(c["lq"], c["lk"]):
            if not Lq:
                continue
            lo, lim = li.limits(Lq, Lk, c["causal"], c["W"])
            j = np.arange(Lk)
            seen = ((j[None, :] >= lo[:, None]) & (j[None, :] < lim[:, None])).any(axis=0)
            ok = ok or any(edge % cm.TILE and seen[edge - 1] and seen[edge] for edge in range(ps, Lk, ps))
        assert ok, ps


def test_a_windowed_case_frees_pages_and_a_window_crosses_the_prefix():
    freed = crossing = 0
    for case in ci.CASES:
        c = ci.make(case)
        if not c["W"]:
            continue
        for ps in ci.PAGE_SIZES:
            _, _, table = ci.paged(case, ps)
            for b, (Lq, Lk, lo0) in enumerate(zip(c["lq"], c["lk"], ci.lo0_of(c["lq"], c["lk"], c["W"]))):
                if Lq and lo0 >= ps:
                    assert all(int(table[b, pi]) in cm.GARBAGE for pi in range(lo0 // ps))
                    freed += lo0 // ps
        if case[0] == "chunk":
            for Lq, Lk in zip(c["lq"], c["lk"]):
                if Lq:
                    lo, lim = li.limits(Lq, Lk, c["causal"], c["W"])
                    crossing += int(((lo < Lk - Lq) & (lim > Lk - Lq) & (lo > 0)).sum())
    assert freed > 0 and crossing > 0


def test_the_layout_poisons_what_no_row_sees():
    """rows at or past Lk and below lo_0 are NaN in the cache and in the pools; unnamed pages are NaN; entries past the last live page
    and of pages wholly below lo_0 are garbage"""
    case = ci.CASES[6]
    c = ci.make(case)
    for ps in ci.PAGE_SIZES:
        kp, vp, table = ci.paged(case, ps)
        named = set()
        for b, (Lk, lo0) in enumerate(zip(c["lk"], ci.lo0_of(c["lq"], c["lk"], c["W"]))):
            assert (c["kc"][b, :, Lk:] == cm.NAN16).all() and (c["vc"][b, :, :lo0] == cm.NAN16).all()
            for pi in range(ci.NCAP // ps):
                e = int(table[b, pi])
                if pi * ps >= Lk or (pi + 1) * ps <= lo0:
                    assert e in cm.GARBAGE
                else:
                    assert 0 <= e < kp.shape[0] and e not in named
                    named.add(e)
        rest = [p for p in range(kp.shape[0]) if p not in named]
        assert len(rest) >= ci.SPARE and (kp[rest] == cm.NAN16).all() and (vp[rest] == cm.NAN16).all()
