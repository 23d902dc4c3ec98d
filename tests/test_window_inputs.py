"""CPU tier of tests/test_gpu_kvcache_window.py: the window's semantics and range arithmetic as tests/window_inputs.py restates
them, and every case of that module reaches the regime it is named for.  The split counts come from the library (the workspace
size it asks for, divided by the size of one split's rows) and are held against the restated rule; the oracle's outputs for the
cases are finite and agree with a float64 softmax.  Conditions on seeded inputs and on host arithmetic: nothing here launches a
kernel."""
import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di
import window_inputs as wi

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
LAUNCHES = [pytest.param(name, W, causal, id=f"{name}-W{W}-{'causal' if causal else 'full'}")
            for name, c in wi.CASES.items() for W in c["windows"] for causal in c["causal"]]


def test_lows_and_limits():
    """lo_i = max(0, L - Nq + 1 + i - W), the same with and without the mask; under the mask a row sees its own position and the
    W - 1 before it; with one row the last W keys; lo < c wherever c >= 1."""
    def lows(L, nq, W):
        return cm.row_limits(L, nq, nq, False, W)[0].tolist()

    def limits(L, nq, causal):
        return cm.row_limits(L, nq, nq, causal)[1].tolist()
    assert lows(1000, 1, 64) == [936] and limits(1000, 1, False) == [1000] and limits(1000, 1, True) == [1000]
    assert lows(1000, 5, 3) == [993, 994, 995, 996, 997] and limits(1000, 5, True) == [996, 997, 998, 999, 1000]
    assert limits(1000, 5, False) == [1000] * 5
    assert lows(4, 5, 3) == [0, 0, 0, 0, 1] and limits(4, 5, True) == [0, 1, 2, 3, 4]
    assert lows(700, 1, 1024) == [0] and lows(0, 3, 7) == [0, 0, 0] and lows(1000, 2, 0) == [0, 0]
    assert wi.start_of(1500, 1, 1024) == 476 and wi.start_tile(1500, 1, 1024) == 448
    for L in range(0, 200, 7):
        for nq in (1, 2, 5):
            for W in (1, 2, 3, 63, 64, 65, 500):
                lo = lows(L, nq, W)
                assert lo == sorted(lo) and wi.start_of(L, nq, W) == min(lo)
                for causal in (False, True):
                    lim = limits(L, nq, causal)
                    assert cm.row_limits(L, nq, nq, causal, W)[0].tolist() == lo   # the same with and without the mask
                    assert all(l < c for l, c in zip(lo, lim) if c >= 1)
                    if causal:   # flash-attn's window_size = (W - 1, 0): at most W keys, ending at the row's own position
                        assert all(c - l == min(W, c) for l, c in zip(lo, lim))


def test_span_cap_and_split_rule():
    """span_cap = min(Ncap, roundup64(W + Nq - 1) + 64), the capacity when the window covers it; the split rule is not monotone in
    the key count (24 tiles: 6 splits, 25 tiles: 5), so the windowed workspace can exceed the unwindowed one."""
    assert wi.span_cap(1, 512, 1) == 128 and wi.span_cap(1, 512, 64) == 128 and wi.span_cap(1, 512, 65) == 192
    assert wi.span_cap(1, 512, 200) == 320 and wi.span_cap(1, 4096, 1024) == 1088 and wi.span_cap(5, 1024, 130) == 256
    assert wi.span_cap(1, 4096, 4096) == 4096 and wi.span_cap(1, 4096, 4095) == 4096 and wi.span_cap(5, 1024, 1020) == 1024
    assert wi.span_cap(1, 4096, 4000) == 4096 and wi.span_cap(1, 100, 10) == 100
    assert wi.split_count(4, 1, 24 * 64) == 6 and wi.split_count(4, 1, 25 * 64) == 5
    assert wi.split_count(4, 1, 1088) == 4 and wi.split_count(8, 2, 320) == 1


@pytest.mark.parametrize("d", [64, 128])
def test_split_counts_are_the_librarys(fa, d):
    """the restated rule against the library, for every case and over a sweep of shapes and windows"""
    for name, c in wi.CASES.items():
        B, Hkv, G, Nq, Ncap = (c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
        for W in c["windows"]:
            S = di.splits_of(fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W), B * Hkv, G * Nq, d)
            assert S == c["S"] == wi.splits(B * Hkv, G * Nq, Nq, Ncap, W), (name, W)
            for ps in wi.PAGES:
                assert fa.kvcache_paged_window_workspace_bytes(B, Hkv, G, Nq, Ncap // ps, ps, d, W) == \
                    fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W)
    for (B, Hkv, G, Nq, Ncap) in ((1, 1, 1, 1, 32768), (8, 16, 1, 1, 32768), (2, 2, 4, 5, 4096), (64, 4, 1, 1, 2000), (3, 1, 1, 200, 8192)):
        for W in (1, 64, 200, 1000, 1024, 1472, 1536, 4096, 5000, 32767, 32768, 1 << 30, 2 ** 31 - 1):
            S = wi.splits(B * Hkv, G * Nq, Nq, Ncap, W)
            got = fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W)
            assert got == (0 if S == 1 else B * Hkv * S * G * Nq * (d + 2) * 4), (B, Hkv, G, Nq, Ncap, W)


def test_case_ranges():
    """the chunk and the live splits per length, from the restated kernel arithmetic"""
    S = wi.CASES["split"]["S"]
    assert S == 4
    # 4096: start 3072 on a tile and a page edge, 16 tiles, 4 per split
    assert wi.start_of(4096, 1, 1024) == 3072 and wi.chunk_of(4096, 1, 1024, S) == 256 and wi.live_splits(4096, 1, 1024, S) == 4
    # 1500: start 476 inside the tile at 448 (rows 448..475 are poisoned and loaded), 17 tiles, 5 per split, 4 live splits
    assert wi.start_tile(1500, 1, 1024) == 448 and wi.chunk_of(1500, 1, 1024, S) == 320 and wi.live_splits(1500, 1, 1024, S) == 4
    # 700: shorter than the window, 11 tiles from key 0, 3 per split
    assert wi.start_of(700, 1, 1024) == 0 and wi.chunk_of(700, 1, 1024, S) == 192 and wi.live_splits(700, 1, 1024, S) == 4
    # 100: two tiles, one per split: two live splits and two empty ones
    assert wi.chunk_of(100, 1, 1024, S) == 64 and wi.live_splits(100, 1, 1024, S) == 2
    # no sequence of any case streams more tiles than span_cap allows
    for name, c in wi.CASES.items():
        for W in c["windows"]:
            for L in c["lens"]:
                assert L - wi.start_tile(L, c["Nq"], W) <= wi.span_cap(c["Nq"], c["Ncap"], W), (name, W, L)
    s = wi.SHIFT
    assert all((L - s["W"]) % 64 == 0 and L >= s["W"] for L in s["lens"])
    assert wi.splits(s["B"], 1, 1, s["Ncap"], s["W"]) == wi.split_count(s["B"], 1, s["W"] + 64) == 4
    g = wi.GRAPH
    lens0 = [g["start"][0] + 1 + t for t in range(g["steps"])]
    assert lens0[0] < g["W"] < lens0[-1] and g["W"] in lens0 and 64 in lens0 and 65 in lens0 and max(lens0) + 1 <= g["Ncap"]


@pytest.mark.parametrize("name,W,causal", LAUNCHES)
def test_case_categories(name, W, causal):
    c = wi.CASES[name]
    S = wi.splits(c["B"] * c["Hkv"], c["G"] * c["Nq"], c["Nq"], c["Ncap"], W)
    assert S == c["S"]
    cats = wi.categories(c["lens"], c["Nq"], c["Ncap"], W, S, causal, wi.PAGES)
    assert cats >= wi.wanted(name, W, causal), wi.wanted(name, W, causal) - cats


def test_cases_cover_every_regime():
    seen = set()
    for name, c in wi.CASES.items():
        for W in c["windows"]:
            for causal in c["causal"]:
                seen |= wi.categories(c["lens"], c["Nq"], c["Ncap"], W, c["S"], causal, wi.PAGES)
    assert seen >= wi.WANTED_TOGETHER, wi.WANTED_TOGETHER - seen


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_references(oracle, fmt, d):
    """cm.expected() (the oracle) against cm.expected_f64 (the plain float64 softmax), for every window case: O within 1e-5 of the value scale, lse within 1e-9; zeros and -inf exactly on
    the rows without a key; at scale 0 the mean of the visible V rows and ln(their number)."""
    for name, c in wi.CASES.items():
        B, Hkv, G, Nq, Ncap = (c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
        (q, k, v), _ = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"])
        for W in c["windows"]:
            for causal in c["causal"]:
                out, lse = wi.reference(oracle, name, d, fmt, W, causal)
                ref, ref_lse = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, causal, W)
                assert np.isfinite(out).all() and not np.isnan(lse).any()
                assert np.abs(out - ref).max() <= 1e-5 * max(1.0, np.abs(v).max())
                dead = np.array([cm.row_limits(L, Nq, Nq, causal)[1] == 0 for L in c["lens"]])
                dead = np.repeat(dead, Hkv * G, axis=0)
                assert np.array_equal(np.isneginf(lse), dead) and (out[dead] == 0.0).all()
                assert np.array_equal(np.isneginf(ref_lse), dead) and np.abs(lse[~dead] - ref_lse[~dead]).max() < 1e-9
                if name == "rows":
                    uo, ul = cm.uniform_expected(v, c["lens"], B, Hkv, G, Nq, causal, W)
                    zo, zl = cm.expected(oracle, q, k, v, c["lens"], B, Hkv, G, Nq, causal, W, scale=0.0)
                    assert np.abs(zo - uo).max() < 1e-6 and np.array_equal(np.isfinite(ul), ~dead)
                    assert np.abs(zl[~dead] - ul[~dead]).max() < 1e-12
    # a window of one key returns that key's V row
    out, _ = wi.reference(oracle, "one_pass", d, fmt, 1, False)
    c = wi.CASES["one_pass"]
    (_, _, v), _ = wi.inputs(oracle, c["B"], c["Hkv"], c["G"], c["Nq"], c["Ncap"], d, fmt, c["seed"])
    assert np.abs(out[0, 0] - v[0, c["lens"][0] - 1]).max() < 1e-6


def test_poison_and_scatter(oracle):
    """the hygiene helpers: NaN at and past the length AND below start_b, the keys in between untouched; garbage exactly in the table
    entries past the last live page or wholly below start_b; every page no table names holds NaN"""
    for name, c in wi.CASES.items():
        B, Hkv, G, Nq, Ncap = (c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
        _, (_, kb, vb) = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, 64, 0, c["seed"])
        for W in c["windows"]:
            k4, v4 = kb.reshape(B, Hkv, Ncap, 64), vb.reshape(B, Hkv, Ncap, 64)
            kc, vc = cm.poisoned(k4, c["lens"], Nq, W), cm.poisoned(v4, c["lens"], Nq, W)
            for ps in wi.PAGES:
                kp, vp, table = cm.scatter(kc, vc, c["lens"], ps, ps, Nq, W)
                named = set()
                for b, L in enumerate(c["lens"]):
                    sb = wi.start_of(L, Nq, W)
                    assert (kc[b, :, L:] == cm.NAN16).all() and (kc[b, :, :sb] == cm.NAN16).all()
                    assert np.array_equal(kc[b, :, sb:L], k4[b, :, sb:L])
                    for pi in range(Ncap // ps):
                        live = pi < di.live_pages(L, ps) and (pi + 1) * ps > sb
                        assert (table[b, pi] in cm.GARBAGE) != live
                        if live:
                            named.add(int(table[b, pi]))
                            assert np.array_equal(kp[table[b, pi]], kc[b, :, pi * ps:(pi + 1) * ps])
                            assert np.array_equal(vp[table[b, pi]], vc[b, :, pi * ps:(pi + 1) * ps])
                unnamed = sorted(set(range(kp.shape[0])) - named)
                assert unnamed and (kp[unnamed] == cm.NAN16).all() and (vp[unnamed] == cm.NAN16).all()
