"""CPU tier of tests/softmax_range_inputs.py: the hostile inputs force what they are named for (measured in float64 on the rounded
values), the numpy model of the lazy reference maximum shows each event on the row built for it, the check of
tests/test_gpu_softmax_range.py accepts the correct model with at least 4x headroom on every bound, and rejects each of the seven
defects on a named case.  No GPU and no library call here.

One defect is not visible in one format, by arithmetic and not by a gap in the inputs: `vote_prev` (the vote compares against the
previous tile) only lets weights grow by the sum of the sub-threshold steps.  On the staircase that is 2^42: it overflows fp16 (the
check sees inf) and is an ordinary bf16 number, so with fp32 accumulators the bf16 result is the correct one.  No input of these
shapes can change that -- at most 13 steps of less than 8 stay below bf16's 2^127 -- and test_vote_prev_is_benign_in_bf16 asserts
exactly this instead of a rejection.
"""
import numpy as np
import pytest

import common_inputs as cm
import mla_inputs as mi
import softmax_range_inputs as sr
import varlen_inputs as vi
import varlen_logit_inputs as li

FMTS = [pytest.param(fmt, id=cm.FMT_NAME[fmt]) for fmt in sr.FMTS]
HEADROOM = 4.0


def _votes(rise):
    return int(np.nansum(rise > sr.KTHR))


def _quiet_steps(rise):
    """rises of a staircase step (7) that stayed under the threshold"""
    return int(np.nansum((rise > sr.STEP - 1.0) & (rise <= sr.KTHR)))


# ---- 1. the inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_mla_lifts_and_masks(fmt):
    case = sr.mla_case(fmt)
    f, lay = sr.MLA, sr.mla_layout()
    assert lay.n == [4, 2, 4] and f["Hq"] * max(lay.n) == 20 <= mi.DR, "20 rows per sequence: one 64-row workgroup, one wave"
    for (b, kind, i, h, key, lift, got) in case["spikes"]:
        print(f"MLA {cm.FMT_NAME[fmt]} seq {b} {kind}: token {i} head {h} key {key}: built {lift} measured {got:.3f}")
        assert abs(got - lift) < 1.0, (kind, key, got)
    assert np.abs(case["c"]).max() < 200.0 and np.abs(case["c"][:, :, :mi.DC]).max() < 6.0, "V stays N(0,1)"
    L = f["lens"][0]
    # the staircase: tiles 0..6 of 32 keys, across a 64-key unit and across the split boundaries of S = 3 and 8
    stair = sr.MLA_KINDS[0][3]
    assert [key // sr.MLA_TILE for key, _ in stair] == list(range(sr.MLA_STAIR_TILES))
    for S in (2, 3, 8):
        chunk = -(-(-(-L // 64)) // S) * 64
        assert len({key // chunk for key, _ in stair}) >= 2 or S == 2, S   # (S = 2 cuts at key 256, behind the staircase)
        assert all(key // chunk == (L - 1) // chunk for key in (390, 400)), "the last split that holds a key"
    assert all(384 <= key < 416 for key in (390, 400)) and 416 <= 420 == L - 1, "ahead of / inside the partial last tile"
    # the masked spike: token 0 sees the keys [0, 418) under the mask, and key 420 without it
    lim = cm.row_limits(L, 4, 4, True)[1]
    assert lim[0] == 418 and lim[3] == L
    # sequence 1: key 65 is the last token's alone; both spikes are its rows'
    lim1 = cm.row_limits(f["lens"][1], 2, 4, True)[1]
    assert lim1[0] == 65 and lim1[1] == 66 and all(i == 1 for _, i, _, _ in sr.MLA_SEQ1)
    # sequence 2: one head near -300, one near +300, the others near 0
    for h, level in sr.MLA_SHIFTED:
        for i in range(4):
            s = sr.mla_scores(case["q"], case["c"], 2, f["Hq"], i, h, f["lens"][2])
            assert np.abs(s - level).max() < 16.0, (h, i, np.abs(s - level).max())


@pytest.mark.parametrize("fmt", FMTS)
def test_mla_benign_scores_never_vote(fmt):
    """every row, with the keys rebuilt for it left out: the largest tile maximum lies less than kThr - 1 above the smallest maximum of
    a whole 32-key tile -- whichever tile a split starts at, a benign row's reference is never voted up by the row itself"""
    case = sr.mla_case(fmt)
    f = sr.MLA
    worst = 0.0
    for b in range(f["B"]):
        L, n = f["lens"][b], f["spans"][b]
        hostile = sr.mla_hostile(b)
        for i in range(n):
            for h in range(f["Hq"]):
                s = sr.mla_scores(case["q"], case["c"], b, f["Hq"], i, h, L).copy()
                s[hostile.get((i, h), [])] = -np.inf
                whole = L // sr.MLA_TILE
                tmax = [s[t * 32:(t + 1) * 32].max() for t in range(-(-L // 32))]
                worst = max(worst, max(tmax) - min(tmax[:whole]))
    print(f"MLA {cm.FMT_NAME[fmt]}: benign tile maxima differ by at most {worst:.2f} log2 units")
    assert worst < sr.KTHR - 1.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
@pytest.mark.parametrize("feature", sr.FEATURES)
def test_varlen_lifts_and_masks(d, fmt, feature):
    c = sr.varlen_case(d, fmt, feature)
    Lq, Lk = c["lq"][0], c["lk"][0]
    assert Lq > d, "more rows than dimensions: the hostile rows are orthogonal, the others orthogonal to their span"
    kinds = sr.varlen_kinds(feature)
    rows = [(i, g) for _, i, g, _, _ in kinds]
    for (kind, i, g, key, lift, got, _) in c["spikes"]:
        print(f"varlen d={d} {cm.FMT_NAME[fmt]} {feature} {kind}: row {i} head {g} key {key}: built {lift} measured {got:.3f}")
        assert abs(got - lift) < 1.0, (kind, key, got)
    # a key rebuilt for one row is benign for every other row of the head
    spiked = {}
    for _, i, g, keys, _ in kinds:
        for key, _ in keys:
            spiked.setdefault(key, []).append((i, g))
    for key, owners in spiked.items():
        for g in range(c["G"]):
            s = (c["q"][:Lq, g].astype(np.float64) @ c["k"][key, 0].astype(np.float64)) * (sr.LOG2E / np.sqrt(d))
            others = np.delete(s, [i for i, gg in owners if gg == g])
            assert np.abs(others).max() < 2.0, (key, g, np.abs(others).max())
    # visibility, causal and not, as the kind says
    for causal in (True, False):
        lo, lim = li.limits(Lq, Lk, causal, c["W"])
        for (kind, i, g, key, lift, got, _) in c["spikes"]:
            seen = lo[i] <= key < lim[i]
            if kind.startswith("masked"):
                assert seen == (not causal and "window" not in kind), (kind, causal)
            else:
                assert seen, (kind, causal)
    if feature == "window":
        lo, lim = li.limits(Lq, Lk, True, sr.WINDOW)
        assert lo[50] - 1 == kinds[0][3][0][0] and lo[51] == kinds[1][3][0][0] and lim[52] - 1 == kinds[2][3][0][0]
        return
    # the kinds sit where they are named for: 64-key tiles, the partial tile from key 384 on, the diagonal at row + 291
    assert [key // cm.TILE for key, _ in kinds[0][3]] == list(range(sr.VARLEN_STAIR_TILES))
    assert all(320 <= kinds[n][3][0][0] < 384 for n in (1, 2)) and kinds[3][3][0][0] < 64 and kinds[4][3][0][0] == Lk - 1 >= 384
    lim = li.limits(Lq, Lk, True, 0)[1]
    assert lim[110] - 1 == kinds[6][3][0][0] >= 384 and lim[60] == kinds[7][3][0][0] and lim[10] <= Lk - 1 and lim[129] == Lk
    # hostile rows in two (in fact three) different 32-row waves of block 0; sequence 1 is a block without a hostile row
    assert len({i // 32 for i, _ in rows if i < vi.BM}) >= 2 and any(i >= vi.BM for i, _ in rows)
    if feature == "sinks":
        for g, sign in ((0, 1.0), (1, -1.0)):
            for (sq, eq), (sk, ek) in zip(vi.bounds(c["cu_q"], sum(c["lq"])), vi.bounds(c["cu_k"], sum(c["lk"]))):
                nat = (c["q"][sq:eq, g].astype(np.float64) @ c["k"][sk:ek, 0].astype(np.float64).T) * c["scale"]
                assert (sign * (c["sinks"][g] - nat) >= sr.SINK_GAP - 0.01).all()
        want, want_lse = sr.varlen_reference(d, fmt, feature, True)
        assert np.abs(want[:sum(c["lq"]), 0]).max() < 1e-20 and np.abs(want_lse[0, :sum(c["lq"])] - c["sinks"][0]).max() < 1e-6


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
def test_varlen_benign_scores_never_vote(d, fmt):
    """plain case: every row meets its first key in tile 0, and with the keys rebuilt for it left out no later tile's maximum lies
    kThr - 1 above tile 0's"""
    c = sr.varlen_case(d, fmt, "plain")
    worst = 0.0
    for b, ((sq, eq), (sk, ek)) in enumerate(zip(vi.bounds(c["cu_q"], sum(c["lq"])), vi.bounds(c["cu_k"], sum(c["lk"])))):
        hostile = {(i, g): [key for key, _ in keys] for _, i, g, keys, _ in sr.VARLEN_KINDS} if b == 0 else {}
        lim = li.limits(eq - sq, ek - sk, True, 0)[1]
        assert lim.min() >= cm.TILE or b == 1
        for i in range(eq - sq):
            for g in range(c["G"]):
                s = sr.varlen_scores(c["q"], c["k"], sq + i, g, d, sk, ek).copy()
                s[hostile.get((i, g), [])] = -np.inf
                for causal_lim in (lim[i], ek - sk):
                    tmax = [s[t:min(t + cm.TILE, causal_lim)].max() for t in range(0, causal_lim, cm.TILE)]
                    worst = max(worst, max(tmax) - tmax[0])
    print(f"varlen d={d} {cm.FMT_NAME[fmt]}: a benign tile maximum lies at most {worst:.2f} log2 units above tile 0's")
    assert worst < sr.KTHR - 1.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
def test_fp8_lifts_survive_the_quantisation(d, fmt):
    c = sr.varlen_fp8_case(d, fmt)
    by_kind = {}
    for (kind, i, g, key, lift, got, _) in c["spikes"]:
        print(f"fp8 d={d} {cm.FMT_NAME[fmt]} {kind}: key {key}: built {lift} measured on the decoded codes {got:.2f}")
        by_kind[kind] = max(by_kind.get(kind, -np.inf), got)
        if lift >= 40.0:
            assert got > sr.FP8_MIN_LIFT, (kind, got)
    assert all(x > sr.FP8_MIN_LIFT for x in by_kind.values()), by_kind


# ---- 2. the references and the events of the correct model ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_references_are_finite(fmt):
    for causal in (True, False):
        want, want_lse = sr.mla_reference(fmt, causal)
        assert np.isfinite(want).all() and np.isfinite(want_lse[np.repeat(sr.mla_layout().tok >= 0, sr.MLA["Hq"], axis=0)]).all()
        Hq = sr.MLA["Hq"]
        assert abs(want_lse[2 * Hq].mean() + sr.SHIFT * sr.LN2) < 10 and abs(want_lse[2 * Hq + 1].mean() - sr.SHIFT * sr.LN2) < 10
        for d in sr.VARLEN_D:
            for feature in sr.FEATURES:
                c = sr.varlen_case(d, fmt, feature)
                want, want_lse = sr.varlen_reference(d, fmt, feature, causal)
                own = vi.owned(c["cu_q"], want.shape[0])
                assert np.isfinite(want[own]).all() and np.isfinite(want_lse[:, own]).all(), (d, feature, causal)


@pytest.mark.parametrize("S", sr.MLA_SPLITS)
@pytest.mark.parametrize("fmt", FMTS)
def test_mla_model_shows_each_event(fmt, S):
    case, lay, f = sr.mla_case(fmt), sr.mla_layout(), sr.MLA
    for causal in (True, False):
        ev = {}
        sr.mla_model(case["q"], case["c"], f["lens"], lay, f["Hq"], fmt, causal, S, None, ev)
        rise = {k: np.concatenate(v) for k, v in ev.items()}
        first = {k: np.array([r[0] if len(r) else np.nan for r in v]) for k, v in ev.items()}   # what a split's first tile met: nothing
        assert all(np.isnan(x).all() for x in first.values()), "a split starts without a reference"
        kinds = {kind: (0, i, h) for kind, i, h, _ in sr.MLA_KINDS}
        kinds.update({kind: (1, i, h) for kind, i, h, _ in sr.MLA_SEQ1})
        stair = rise[kinds["staircase"]]
        if S in (1, 2, 0):   # the staircase (keys 5 .. 203) lies inside one split: two moves at least, and a step without one
            assert _votes(stair) >= 2 and _quiet_steps(stair) >= 1, stair
        else:                # S = 3: split 0 holds steps 0 .. 5; S = 8: every split two tiles, one step each, none moves the reference
            assert (_votes(stair) >= 2 and _quiet_steps(stair) >= 1) if S == 3 else (_votes(stair) == 0 and _quiet_steps(stair) >= 3), stair
        # a jump moves the reference, by about its lift, unless its tile is the first of its split: then the merge has to carry it
        jumps = [(kind, b, keys[0]) for b, table in ((0, sr.MLA_KINDS[1:3] + sr.MLA_KINDS[4:5]), (1, sr.MLA_SEQ1)) for kind, _, _, keys in table]
        for kind, b, (key, lift) in jumps:
            r = rise[kinds[kind]]
            if _opens_a_split(f["lens"][b], S, key):
                assert _votes(r) == 0, (kind, S, r)
            else:
                assert _votes(r) == 1 and abs(np.nanmax(r) - lift) < 6.0, (kind, S, r)
        r = rise[kinds["all but tile 0 below -200"]]
        assert _votes(r) == 0 and np.nanmax(r[:len(ev[kinds["all but tile 0 below -200"]][0])]) < -200.0, "nothing moves after tile 0"
        r = rise[kinds["masked 150 on the last key"]]
        assert _votes(r) == (0 if causal else 1), ("masked spike", causal, r)
    assert _opens_a_split(421, 8, 390) and not _opens_a_split(421, 2, 390) and _opens_a_split(66, 2, 64) and not _opens_a_split(66, 1, 64)


def _opens_a_split(L, S, key):
    """the 32-key tile of `key` is the first tile of a split of a sequence of L keys"""
    S = S or sr.mla_split_count(sr.MLA["B"], sr.MLA["Hq"], sr.MLA["max_q"], sr.MLA["Ncap"])
    chunk = -(-(-(-L // 64)) // S) * 64
    return (key // sr.MLA_TILE * sr.MLA_TILE) % chunk == 0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
def test_varlen_model_shows_each_event(d, fmt):
    c = sr.varlen_case(d, fmt, "plain")
    for causal in (True, False):
        ev = {}
        sr.varlen_model(c, causal, events=ev)
        rise = {kind: ev[0, i, g] for kind, i, g, _, _ in sr.VARLEN_KINDS}
        assert _votes(rise["staircase"]) >= 2 and _quiet_steps(rise["staircase"]) >= 1, rise["staircase"]
        for kind, lift in (("jump 40 in the last whole tile", 40.0), ("jump 150 in the last whole tile", 150.0), ("jump 40 on the last key", 40.0),
                           ("jump 40 on the diagonal", 40.0)):
            assert _votes(rise[kind]) == 1 and abs(np.nanmax(rise[kind]) - lift) < 6.0, (kind, causal, rise[kind])
        assert _votes(rise["all but tile 0 below -200"]) == 0 and np.nanmax(rise["all but tile 0 below -200"]) < -200.0
        for kind in ("masked 150 on the last key", "masked 150 one past the diagonal"):
            assert _votes(rise[kind]) == (0 if causal else 1), (kind, causal, rise[kind])
        # sequence 1 and every row that is not hostile: no vote of its own
        hostile = {(0, i, g) for _, i, g, _, _ in sr.VARLEN_KINDS}
        assert all(_votes(r) == 0 for key, r in ev.items() if key not in hostile)
    cw = sr.varlen_case(d, fmt, "window")
    for causal in (True, False):
        ev = {}
        sr.varlen_model(cw, causal, events=ev)
        rise = {kind: ev[0, i, g] for kind, i, g, _, _ in sr.VARLEN_WINDOW_KINDS}
        assert _votes(rise["masked 150 just below the window"]) == 0, "the key below the lower limit moves nothing"
        assert np.nanmax(rise["jump 40 on the window's first key"]) < 0.0, "the row meets its spike first: everything after lies below"
        assert _votes(rise["jump 40 on the diagonal"]) == 1
        assert _votes(rise["staircase"]) == 1 and _quiet_steps(rise["staircase"]) == 1


# ---- 3. the check: the correct model with headroom, every defect rejected -----------------------------------------------------------------
def _mla_run(oracle, fmt, causal, S, defect=None):
    """-> the figures of check_packed, which asserts"""
    case, lay, f = sr.mla_case(fmt), sr.mla_layout(), sr.MLA
    po, pl = sr.mla_model(case["q"], case["c"], f["lens"], lay, f["Hq"], fmt, causal, S, defect)
    want, want_lse = sr.mla_reference(fmt, causal)
    return sr.check_packed(oracle, lay, po, pl, want, want_lse, fmt, sr.mla_vmax(fmt), "model:fa_mla_decode",
                           f"{cm.FMT_NAME[fmt]} causal={int(causal)} S={S} {defect or 'correct'}")


def _varlen_run(d, fmt, feature, causal, out_same=False, defect=None):
    c = sr.varlen_case(d, fmt, feature)
    o, lse = sr.varlen_model(c, causal, defect, out_same=out_same)
    want, want_lse = sr.varlen_reference(d, fmt, feature, causal)
    return sr.check_varlen(c, o, lse, want, want_lse, "model:fa_forward_varlen",
                           f"d{d} {cm.FMT_NAME[fmt]} {feature} causal={int(causal)} o16={int(out_same)} {defect or 'correct'}")


def _headroom(figs, fmt, vmax, out_same=False):
    ma_b, rl_b = sr.bounds(fmt, vmax, out_same)
    return min(ma_b / max(figs[0], 1e-300), rl_b / max(figs[1], 1e-300), 2 * cm.P_EPS[fmt] / max(figs[2], 1e-300))


@pytest.mark.parametrize("fmt", FMTS)
def test_correct_model_passes_with_headroom_mla(oracle, fmt):
    worst = np.inf
    for causal in (True, False):
        for S in sr.MLA_SPLITS:
            worst = min(worst, _headroom(_mla_run(oracle, fmt, causal, S), fmt, sr.mla_vmax(fmt)))
    print(f"HEADROOM|fa_mla_decode|{cm.FMT_NAME[fmt]}|{worst:.1f}x on the tightest bound")
    assert worst >= HEADROOM


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", sr.VARLEN_D)
def test_correct_model_passes_with_headroom_varlen(d, fmt):
    worst = np.inf
    for feature in sr.FEATURES:
        for causal in (True, False):
            figs = _varlen_run(d, fmt, feature, causal)
            worst = min(worst, _headroom(figs, fmt, sr.varlen_vmax(sr.varlen_case(d, fmt, feature))))
            _varlen_run(d, fmt, feature, causal, out_same=True)   # a 16-bit output: rounding O once more stays inside its bounds
    print(f"HEADROOM|fa_forward_varlen|d{d} {cm.FMT_NAME[fmt]}|{worst:.1f}x on the tightest bound")
    assert worst >= HEADROOM


# the case each defect is rejected on: (family, causal, S or d)
REJECTED_ON = {
    "no_alpha_o": (("mla", True, 1), ("varlen", True, 64)),
    "no_alpha_l": (("mla", True, 1), ("varlen", False, 128)),
    "vote_prev": (("mla", True, 1), ("varlen", True, 64)),
    "max_before_mask": (("mla", True, 1), ("varlen", True, 128)),
    "merge_first": (("mla", True, 3),),
    "merge_plain": (("mla", False, 2),),
    "lse_stale_m": (("mla", True, 1), ("varlen", False, 64)),
}
assert set(REJECTED_ON) == set(sr.DEFECTS)


# (vote_prev, bf16) is not a numerical defect at these shapes: test_vote_prev_is_benign_in_bf16 asserts why
@pytest.mark.parametrize("defect,fmt", [pytest.param(x, fmt, id=f"{x}-{cm.FMT_NAME[fmt]}") for x in sr.DEFECTS for fmt in sr.FMTS
                                        if (x, fmt) != ("vote_prev", 1)])
def test_every_defect_is_rejected(oracle, defect, fmt):
    for family, causal, x in REJECTED_ON[defect]:
        with pytest.raises(AssertionError):
            if family == "mla":
                _mla_run(oracle, fmt, causal, x, defect)
            else:
                _varlen_run(x, fmt, "plain", causal, defect=defect)
        print(f"REJECTED|{defect}|{cm.FMT_NAME[fmt]}|{family} causal={int(causal)} {'S' if family == 'mla' else 'd'}={x}")


def test_vote_prev_is_benign_in_bf16(oracle):
    """see the module docstring: the staircase's steps sum to 42 log2 units, a weight of 2^42 is an fp16 inf and a bf16 number, and no
    row of these shapes can collect 127"""
    assert sr.STEP * (sr.MLA_STAIR_TILES - 1) == 42.0 and 42.0 > 16.0 and sr.KTHR * 13 < 127.0
    with pytest.raises(AssertionError):
        _mla_run(oracle, 0, True, 1, "vote_prev")
    ok = _mla_run(oracle, 1, True, 1)
    bad = _mla_run(oracle, 1, True, 1, "vote_prev")
    assert _headroom(bad, 1, sr.mla_vmax(1)) >= HEADROOM, (ok, bad)


# ---- 4. the stated gap: the committed MLA families cannot tell these defects from the scheme -------------------------------------------------
def test_gap_on_the_committed_mla_family(oracle):
    """printed, not asserted: on mla_inputs' family h5 (N(0,1) logits, every key range from key 0) the model with O or l not rescaled, or
    with a merge that ignores m, passes mla_inputs.check"""
    name = "h5"
    f, lay = mi.family(name), mi.layout(name)
    for fmt in sr.FMTS:
        (q, c), _ = mi.inputs(oracle, name, fmt)
        want, want_lse = mi.reference(oracle, name, fmt, True)
        for defect in ("no_alpha_o", "no_alpha_l", "merge_first", "merge_plain"):
            for S in (1, 2):
                po, pl = sr.mla_model(q, c, f["lens"], lay, f["Hq"], fmt, True, S, defect)
                try:
                    mi.check(oracle, name, po, pl, want, want_lse, fmt, f"{defect} on {name}")
                    verdict = "passes"
                except AssertionError:
                    verdict = "is rejected"
                ma, rl, le = sr.figures_packed(lay, po, pl, want, want_lse)
                print(f"GAP|mla_inputs {name}|{cm.FMT_NAME[fmt]} S={S}|{defect} {verdict}|{ma:.3e}|{rl:.3e}|{le:.3e}")
