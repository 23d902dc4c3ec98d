"""CPU tier of tests/kv256_inputs.py: the inputs of tests/test_gpu_kv256_edges.py force what they are named for, and its checks reject
a wrong kernel.  No GPU and no library call here.

  A. census   the launch list holds every pair of (S, page size), (S, W), (W, page size); the exactness rule holds for every listed
              shape; the closed-form sums are the float64 reference's O * cnt; one key more or less is rejected
  B. range    every spike is visible or masked as named and lies where it was built; the staircase stays under kThr per tile; the
              model votes after tile 0 in both blocks; the check accepts the model for every listed launch and rejects each of the
              seven sr.DEFECTS on a named one
  C. random   the length sweep covers the categories of the d = 128 sweep; the row shapes are the block counts they are named for;
              the transcribed split rule gives the counts the automatic cases are named for
  D. far      the live heads and pages start past 2^32 and 2^33 bytes, and the units a wrapped offset lands in are other ones

As in tests/test_softmax_range_inputs.py, `vote_prev` is no numerical defect in bf16 (a weight of 2^42 is an ordinary bf16 number), so
it is rejected in fp16 alone.
"""
import numpy as np
import pytest

import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import kv256_inputs as kv
import softmax_range_inputs as sr

FMTS = [pytest.param(fmt, id=cm.FMT_NAME[fmt]) for fmt in (0, 1)]


def _votes(rise):
    return int(np.nansum(rise > sr.KTHR))


# ---- the host's arithmetic -----------------------------------------------------------------------------------------------------------
def test_split_rule_and_workspace():
    assert kv.window_span_cap(8, 1024, 70) == 192 and kv.window_span_cap(8, 1024, 1020) == 1024 and kv.window_span_cap(1, 256, 64) == 128
    for B, lens, W, want in kv.AUTO_CASES:
        assert len(lens) == B and kv.split_count(B, kv.AUTO["Hkv"], kv.AUTO["G"], kv.AUTO["max_q"], kv.AUTO["Ncap"], W) == want
    assert kv.split_count(8, 2, 4, 5, 256) == 1, "Ncap = 256: four tiles, one split -- what tests/test_gpu_kv256.py can reach"
    f = kv.CENSUS
    assert [kv.split_count(len(f["lens"]), f["Hkv"], f["G"], f["max_q"], f["Ncap"], W) for W in kv.CENSUS_W] == [4, 1, 1, 1]
    assert kv.split_count(kv.RANGE["B"], 1, kv.RANGE["G"], kv.RANGE["max_q"], kv.RANGE["Ncap"]) == 4
    assert kv.workspace_bytes(1, 1, 4, 8, 4) == 4 * 32 * 260 * 4 and kv.workspace_bytes(3, 2, 5, 8, 1) == 0
    assert kv.start_of(933, 4, 100) == (830, 768) and kv.start_of(933, 4, 0) == (0, 0) and kv.chunk_of(933, 4, 0, 2) == 512


# ---- A. census -------------------------------------------------------------------------------------------------------------------------
def test_census_launches_hold_every_pair():
    runs = kv.census_launches()
    for a, b, A, B in ((0, 2, kv.CENSUS_S, kv.CENSUS_PAGES), (0, 1, kv.CENSUS_S, kv.CENSUS_W), (1, 2, kv.CENSUS_W, kv.CENSUS_PAGES),
                       (0, 3, kv.CENSUS_S, (0, 1)), (1, 3, kv.CENSUS_W, (0, 1)), (2, 3, kv.CENSUS_PAGES, (0, 1))):
        assert {(r[a], r[b]) for r in runs} == {(x, y) for x in A for y in B}, (a, b)
    for S, W, ps, causal in runs:
        if ps:
            assert (S, W, 0, causal) in runs, "every paged launch has its contiguous launch"
    f = kv.CENSUS
    n = [min(s, f["max_q"]) for s in f["spans"]]
    assert {0, 1, 3, 8} <= set(f["spans"]) and max(f["spans"]) > f["max_q"] and f["G"] * f["max_q"] == 40
    assert any(L < x for L, x in zip(f["lens"], n) if L > 0), "rows below their first key beside rows with keys"
    assert f["Ncap"] // kv.TILE == 16 == max(kv.CENSUS_S)


@pytest.mark.parametrize("coding", ci.CODINGS)
@pytest.mark.parametrize("fmt", FMTS)
def test_census_is_exact_and_closed_form(oracle, fmt, coding):
    p, m = kv.census_problem(oracle, fmt, coding)
    assert not p.k.any() and p.lay.n == [3, 8, 8, 1, 8, 0, 8, 8, 5, 8]
    worst_count = 0.0
    for causal in (0, 1):
        for W in kv.CENSUS_W:
            S, cnt, m_q = kv.census_expected(p, m, coding, causal, W)
            assert ci.z_exact(fmt, S.max()), (causal, W, S.max())
            worst_count = max(worst_count, float((S / m_q[:, None, None]).max()))
            want, want_lse = p.reference(causal, W, softcap=kv.CENSUS_SOFTCAP if W == 70 else 0.0)
            assert np.abs(want * cnt[:, :, None] - S).max() < 1e-9, (causal, W)
            assert ci.census_check(want, S, cnt, m_q) < 1e-9
            live = cnt > 0
            assert np.array_equal(np.isfinite(want_lse), live) and np.abs(want_lse[live] - kv.census_lse(cnt)[live]).max() < 1e-12
            # one key more in every sequence: the check decides against it
            with pytest.raises(AssertionError):
                longer = kv.Problem((p.q, p.k, p.v), (p.qb, p.kb, p.vb), [L + 1 for L in p.lens], p.spans, p.Hkv, p.G, p.max_q, p.Ncap, fmt)
                ci.census_check(longer.reference(causal, W)[0], S, cnt, m_q)
    assert worst_count == (4 if coding == "residue" else 64)
    assert ci.out16_exact(fmt, worst_count) == (coding == "residue" or fmt == 0)


# ---- B. range --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", kv.RANGE_VARIANTS)
@pytest.mark.parametrize("fmt", FMTS)
def test_range_spikes_lie_where_they_were_built(oracle, fmt, variant):
    p, spikes = kv.range_case(oracle, fmt, variant)
    f = kv.RANGE
    W, _ = kv.range_options(variant)
    assert p.lay.n == [4, 2, 4] and f["G"] * 4 == 40 <= kv.D, "sequence 0: 40 orthogonal rows, two blocks of 32"
    for (b, kind, i, h, key, lift, got) in spikes:
        print(f"kv256 {cm.FMT_NAME[fmt]} {variant} seq {b} {kind}: token {i} head {h} key {key}: built {lift} measured {got:.3f}")
        assert abs(got - lift) < 1.0, (kind, key, got)
        for causal in (True, False):
            lo, c, _ = cm.row_limits(f["lens"][b], p.lay.n[b], f["max_q"], causal, W)
            seen = lo[i] <= key < c[i]
            if kind.startswith("masked"):
                assert seen == (not causal and "window" not in kind), (kind, causal)
            else:
                assert seen, (kind, causal)
    assert np.abs(p.v).max() < 6.0
    by_kind = {kind: [(key, got) for (b, k2, _, _, key, _, got) in spikes if k2 == kind and b == 0] for kind, _, _, _ in kv.range_kinds(variant)}
    stair = by_kind["staircase"]
    steps = np.diff([got for _, got in stair])
    assert (steps < sr.KTHR).all() and (steps > sr.KTHR - 2.0).all(), steps
    assert len({key // kv.TILE for key, _ in stair}) == len(stair), "one step per tile"
    kinds = kv.range_kinds(variant)
    blocks = {(h * 4 + i) // kv.ROWS for _, i, h, _ in kinds}
    assert blocks == {0, 1}, "hostile rows in both blocks"
    hostile = {(i, h) for _, i, h, _ in kinds}
    for blk in (0, 1):
        assert any((x % 4, x // 4) not in hostile for x in range(blk * 32, min(blk * 32 + 32, 40))), "an all-benign row in each block"
    L = f["lens"][0]
    if variant == "window":
        lo, c, _ = cm.row_limits(L, 4, 4, True, W)
        assert kv.start_of(L, 4, W) == (830, 768) and lo[1] - 1 == 830 and lo[2] == 832 and c[1] - 1 == 930
        return
    assert stair[-1][1] - stair[0][1] > 20.0 and [key // kv.TILE for key, _ in stair] == list(range(kv.RANGE_STAIR_TILES))
    assert L == 14 * 64 + 37 and by_kind["all but tile 0 below -200"][0][0] < 64 and by_kind["jump 40 on the last key"][0][0] == L - 1
    for S in kv.RANGE_SPLITS:
        chunk = kv.chunk_of(L, 4, 0, S or p.split_count())
        assert all(key // chunk == (L - 1) // chunk and 896 <= key < L - 1 for key in (900, 910)), "the last split that holds a key"
    # sequence 1: key 65 is the last token's alone; sequence 2: one head near -300, one near +300
    assert cm.row_limits(66, 2, 4, True)[1][0] == 65
    for h, level in kv.RANGE_SHIFTED:
        for i in range(4):
            assert np.abs(kv.range_scores(p.q, p.k, 2, i, h, f["lens"][2]) - level).max() < 16.0


def _opens_a_split(L, S, key):
    return (key // kv.TILE * kv.TILE) % kv.chunk_of(L, 4, 0, S) == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_range_model_shows_each_event(oracle, fmt):
    p, _ = kv.range_case(oracle, fmt, "plain")
    L = kv.RANGE["lens"][0]
    for S in kv.RANGE_SPLITS:
        S_eff = S or p.split_count()
        for causal in (True, False):
            ev = {}
            kv.model(p, causal, S=S, events=ev)
            assert all(np.isnan(r[0]) for parts in ev.values() for r in parts if len(r)), "a split starts without a reference"
            rise = {(b, i, h): np.concatenate(parts) for (b, _, i, h), parts in ev.items()}
            kinds = {kind: (0, i, h) for kind, i, h, _ in kv.RANGE_KINDS}
            if S == 1:
                # a vote after tile 0 -- with O and l no longer 0 -- in both blocks of sequence 0
                for blk, heads in ((0, range(8)), (1, (8, 9))):
                    assert any(_votes(rise[0, i, h]) >= 1 for h in heads for i in range(4)), blk
                stair = rise[kinds["staircase"]]
                assert _votes(stair) >= 2 and np.nansum((stair > sr.STEP - 1.0) & (stair <= sr.KTHR)) >= 1, stair
                # every row that is not hostile: no vote of its own
                hostile = {(b, i, h) for b in (0, 1) for (i, h) in kv.range_hostile("plain", b)}
                assert all(_votes(r) == 0 for key, r in rise.items() if key not in hostile)
            for kind, key, lift in (("jump 40 in the last split", 900, 40.0), ("jump 150 in the last split", 910, 150.0)):
                r = rise[kinds[kind]]
                if _opens_a_split(L, S_eff, key):
                    assert S == 16 and _votes(r) == 0, (kind, S)
                else:
                    assert _votes(r) == 1 and abs(np.nanmax(r) - lift) < 6.0, (kind, S, r)
            r = rise[kinds["all but tile 0 below -200"]]
            first = ev[0, 0, 3, 9][0]                                  # the split of tile 0 (S = 16: that tile alone)
            assert _votes(r) == 0 and (len(first) < 2 or np.nanmax(first) < -200.0), "nothing moves after tile 0"
            assert _votes(rise[kinds["masked 150 on the last key"]]) == (0 if causal or _opens_a_split(L, S_eff, L - 1) else 1)
    pw, _ = kv.range_case(oracle, fmt, "window")
    for causal in (True, False):
        ev = {}
        kv.model(pw, causal, W=sr.WINDOW, events=ev)
        rise = {kind: ev[0, 0, i, h][0] for kind, i, h, _ in kv.RANGE_WINDOW_KINDS}
        assert all(len(r) == 3 for r in rise.values()), "three tiles from start_t = 768"
        assert _votes(rise["masked 150 just below the window"]) == 0 and _votes(rise["jump 40 on the diagonal"]) == 1
        assert np.nanmax(rise["jump 40 on the window's first key"]) < 0.0
        # tokens 2 and 3 meet their first key in tile 1 and vote there, which takes the staircase's row of the same block along: both
        # of its steps are seen, each under kThr
        assert np.nansum((rise["staircase"] > sr.STEP - 1.0) & (rise["staircase"] <= sr.KTHR)) == 2


def _range_run(oracle, fmt, variant, causal, S, out16=False, defect=None):
    p, _ = kv.range_case(oracle, fmt, variant)
    W, softcap = kv.range_options(variant)
    po, pl = kv.model(p, causal, W, softcap, S, defect, out16=out16)
    want, want_lse = kv.range_reference(oracle, fmt, variant, causal)
    return kv.range_check(oracle, p, po, pl, want, want_lse,
                          f"model {cm.FMT_NAME[fmt]} {variant} causal={int(causal)} S={S} o16={int(out16)} {defect or 'correct'}", out16)


@pytest.mark.parametrize("variant", kv.RANGE_VARIANTS)
@pytest.mark.parametrize("fmt", FMTS)
def test_check_accepts_the_model(oracle, fmt, variant):
    """the scheme alone stays inside the project's bounds on every listed launch: what fixes the inputs"""
    for v, causal, S, out16 in kv.range_launches():
        if v == variant:
            _range_run(oracle, fmt, variant, causal, S, out16)


# the launch each defect is rejected on: (variant, causal, S)
REJECTED_ON = {
    "no_alpha_o": ("plain", True, 1),
    "no_alpha_l": ("plain", True, 1),
    "vote_prev": ("plain", True, 1),
    "max_before_mask": ("plain", True, 1),
    "merge_first": ("plain", True, 3),
    "merge_plain": ("plain", True, 2),
    "lse_stale_m": ("plain", True, 1),
}
assert set(REJECTED_ON) == set(sr.DEFECTS)


@pytest.mark.parametrize("defect,fmt", [pytest.param(x, fmt, id=f"{x}-{cm.FMT_NAME[fmt]}") for x in sr.DEFECTS for fmt in (0, 1)
                                        if (x, fmt) != ("vote_prev", 1)])
def test_check_rejects_every_defect(oracle, defect, fmt):
    variant, causal, S = REJECTED_ON[defect]
    assert (variant, causal, S, False) in kv.range_launches()
    with pytest.raises(AssertionError):
        _range_run(oracle, fmt, variant, causal, S, defect=defect)
    print(f"REJECTED|{defect}|{cm.FMT_NAME[fmt]}|{variant} causal={int(causal)} S={S}")


# ---- C. random ---------------------------------------------------------------------------------------------------------------------------
def test_sweep_and_row_shapes():
    lens, spans = di.c_lens(), kv.sweep_spans()
    assert len(lens) == len(spans) == 48 and set(spans) == set(range(kv.SWEEP["max_q"] + 3))
    assert di.length_categories(lens, kv.SWEEP["Ncap"], di.C_SPLITS, di.C_PAGES) >= di.c_categories_wanted(di.C_PAGES)
    assert {cm.INT_MIN, cm.INT_MAX, -1, 1025} <= set(lens)
    assert [(-(-G * n // 32), G * n % 32) for G, n in kv.ROW_CASES] == [(4, 0), (2, 3), (1, 3)]
    assert kv.ROW_NCAP % 64 and {1, 2, 3} <= set(kv.ROW_LENS) and kv.ROW_CASES[1][1] == 5
    lo, c, _ = cm.row_limits(3, 5, 5, True)
    assert list(c) == [0, 0, 1, 2, 3], "n_b = 5 rows on 3 keys: two rows below their first key"
    assert all(min(s, di.D_SHAPE["Nq"]) == di.D_SHAPE["Nq"] for s in kv.SCALE_SPANS) and len(kv.SCALE_SPANS) == len(di.D_LENS)
    assert kv.AUTO["G"] * kv.AUTO["max_q"] <= 32


# ---- D. far ------------------------------------------------------------------------------------------------------------------------------
def test_far_offsets_lie_past_4_and_8_gib():
    f = kv.FAR_CONTIG
    head = f["Ncap"] * kv.D * 2
    offs = [b * head for b, _ in kv.FAR_CONTIG_LIVE]
    assert offs[0] == 0 and 2 ** 32 < offs[1] < 2 ** 32 + 4 * head and 2 ** 33 < offs[2] < 2 ** 33 + 4 * head and offs[3] == (f["B"] - 1) * head
    live = [b for b, _ in kv.FAR_CONTIG_LIVE]
    alias = di.wrap_aliases(live, f["Ncap"] * kv.D, f["B"])
    assert alias and not set(alias) & set(live) and {1, 7} <= set(alias)
    g = kv.FAR_PAGED
    unit = g["ps"] * kv.D * 2
    named = [x for row in kv.FAR_PAGED_TABLE for x in row]
    assert len(set(named)) == len(named) and max(named) < g["num_pages"] and g["S"] > 1 and g["Hkv"] == 2
    starts = sorted(page * g["Hkv"] * unit for page in named)
    assert any(2 ** 32 < s < 2 ** 32 + 64 * unit for s in starts) and any(2 ** 33 < s < 2 ** 33 + 64 * unit for s in starts)
    units = kv.far_units(named, g["Hkv"])
    alias = di.wrap_aliases(units, g["ps"] * kv.D, g["num_pages"] * g["Hkv"])
    assert alias and not set(alias) & set(units)
    assert [di.live_pages(L, g["ps"]) for L in kv.FAR_PAGED_LENS] == [len(row) for row in kv.FAR_PAGED_TABLE]
