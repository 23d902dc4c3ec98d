"""CPU tier of tests/attend_varlen_inputs.py: the families of the mixed prefill + decode step are sharp enough.  The routing rule is a
numpy model over the float64 reference; every WRONG rule must be rejected by the check the GPU tier applies (av.problems) on at least
one family and part -- by values or by sentinels in rows that must stay untouched -- and the rule as specified must pass everywhere."""
import numpy as np
import pytest

import attend_varlen_inputs as av
import common_inputs as cm
import decode_varlen_inputs as dv

D, FMT = 64, 0
# where each wrong rule must show: (family, parts)
SHOWS = {
    "short_takes_below_T_only": [("mixed", 3), ("mixed", 1)],     # the span-T sequence is taken by neither half
    "long_takes_T": [("mixed", 2)],                               # the span-T sequence is written by a parts = 2 call
    "short_cuts_long": [("mixed", 1), ("all_long", 1)],           # T rows of every LONG sequence are written by a parts = 1 call
    "long_takes_all": [("mixed", 2), ("all_short", 2)],
    "class_from_raw_cu": [("clamped", 1), ("clamped", 2)],        # sequence 0 (raw 82, span 3) changes halves
    "long_aligned_to_T": [("mixed", 3), ("mixed", 2), ("all_long", 3), ("nokey", 3)],
    "T_plus_1_dropped": [("mixed", 3), ("all_long", 2)],
    "idle_slot_writes": [("mixed", 3)],                           # the idle slot's s_b is the first token of the 140-row sequence
}


def test_the_families_are_what_the_issue_names():
    lay = av.layout("mixed")
    assert lay.span == [1, 4, 5, 0, 140] and lay.cls == [av.SHORT, av.SHORT, av.LONG, 0, av.LONG] and av.T == 4
    assert lay.s[0] == 3 and lay.total_q == lay.s[4] + 140 + 2 and lay.s[3] == lay.s[4]
    assert 140 > cm.ROWS                                            # crosses the tiled kernel's row block
    assert set(av.layout("all_short").cls) == {av.SHORT} and set(av.layout("all_long").cls) == {av.LONG}
    c = av.layout("clamped")
    raw = np.diff(np.asarray(av.FAMILIES["clamped"]["cu"]))
    assert c.span == [3, 0, 5, 2, 4] and list(raw) == [82, -96, 5, 2, 4] and c.cu[1] > c.total_q
    assert c.cls == [av.SHORT, 0, av.LONG, av.SHORT, av.SHORT]
    assert av.Layout(c.cu, c.total_q, raw_class=True).cls[0] == av.LONG
    own = np.zeros(c.total_q, int)
    for s, n in zip(c.s, c.span):
        own[s:s + n] += 1
    assert own.max() == 1 and (own == 0).sum() == 6                 # disjoint, with tokens of no sequence in front and between
    n = av.layout("nokey")
    b = n.cls.index(av.LONG)
    assert av.FAMILIES["nokey"]["lens"][b] < n.span[b]
    assert av.layout("tiny").total_q <= av.T and set(av.layout("tiny").cls) == {av.SHORT}
    for name in av.NAMES:
        lay, f = av.layout(name), av.FAMILIES[name]
        assert len(f["lens"]) == len(lay.span) and f["Ncap"] % av.PAGE == 0
        assert not lay.rows(3)[:1].any() and not (lay.rows(1) & lay.rows(2)).any()
        assert name == "clamped" or not lay.rows(3)[-1:].any()      # (clamped's sequence 0 ends where the tensor ends)
    assert av.want_S("mixed") == 1 and av.want_S("mixed", av.WINDOW) == 1 and av.want_S("split") > 1
    dflt = av.layout("default")
    assert av.threshold("default") == 128 and dflt.span == [1, 128, 129] and dflt.cls == [av.SHORT, av.SHORT, av.LONG]


def test_the_reference_is_the_packed_decode_tiers_on_short_rows_and_sees_no_key_where_it_must():
    """a SHORT sequence's rows are cm.expected_f64 with nq = span (what dv.reference computes); the first rows of nokey's LONG
    sequence have no key"""
    o, lse = av.model("nokey", D, FMT)
    lay = av.layout("nokey")
    b = lay.cls.index(av.LONG)
    L, n, s = av.FAMILIES["nokey"]["lens"][b], lay.span[b], lay.s[b]
    assert (lse[:, s:s + n - L] == -np.inf).all() and (o[s:s + n - L] == 0).all() and np.isfinite(lse[:, s + n - L:s + n]).all()
    o, lse = av.model("nokey", D, FMT, on=True)                    # with sinks: the sink logit, except on the head without one
    sinks = av.options(True, av.HKV * av.G)[2]
    assert np.allclose(lse[0, s:s + n - L], sinks[0]) and (lse[1, s:s + n - L] == -np.inf).all()


@pytest.mark.parametrize("name", [n for n in av.NAMES if n not in ("split", "default")])
def test_the_rule_as_specified_passes(name):
    for parts in (1, 2, 3):
        for on in (False, True):
            o, lse = av.model(name, D, FMT, parts, on)
            assert not av.problems(name, o, lse, o, lse, parts, FMT), (name, parts, on)
    # the two halves overlaid are the whole
    o1, l1 = av.model(name, D, FMT, 1)
    o2, l2 = av.model(name, D, FMT, 2)
    o3, l3 = av.model(name, D, FMT, 3)
    r1 = av.layout(name).rows(1)
    assert np.array_equal(np.where(r1[:, None, None], o1, o2).view(np.uint32), o3.view(np.uint32))
    assert np.array_equal(np.where(r1[None, :], l1, l2), l3)
    if name == "tiny":
        assert (o2.view(np.uint32) == dv.SENTINEL_O32).all() and (l2 == np.float32(dv.SENTINEL_LSE)).all()


@pytest.mark.parametrize("wrong", av.WRONG)
def test_every_wrong_rule_is_rejected(wrong):
    assert set(SHOWS) == set(av.WRONG)
    for name, parts in SHOWS[wrong]:
        want = av.model(name, D, FMT, parts)
        got = av.model(name, D, FMT, parts, wrong=wrong)
        found = av.problems(name, *got, *want, parts, FMT)
        print(wrong, name, parts, found)
        assert found, f"{wrong} passes on {name} with parts = {parts}"
        # not by rounding: a sentinel finding, or an error far above the bound
        if not any("sentinel" in f or "not written" in f for f in found):
            own = av.layout(name).rows(parts)
            fin = np.isfinite(want[1][:, own]) & np.isfinite(got[1][:, own])
            with np.errstate(invalid="ignore"):
                err = np.abs(got[1][:, own] - want[1][:, own])
            assert err[fin].max() > 100 * 2 * cm.P_EPS[FMT], (wrong, name, found)
