"""CPU tier of tests/test_gpu_decode_edges.py: every input of tests/decode_inputs.py reaches the regime it is named for.  The split
counts come from the library (the workspace size it asks for, divided by the size of one split's rows), everything else from
float64 numpy on the 16-bit-rounded values; the oracle's outputs for the cases are finite and agree with a float64 softmax.
These are conditions on seeded inputs and on host arithmetic, not measurements of a kernel: nothing here launches one."""
import numpy as np
import pytest

import common_inputs as cm
import decode_inputs as di

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]


def _kv_splits(fa, shape, d):
    B, Hkv, G, Nq, Ncap = (shape[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
    return di.splits_of(fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d), B * Hkv, G * Nq, d)


def _self_consistent(oracle, q, k, v, lens, shape, causal, scale=None):
    """the oracle's O is finite, agrees with the float64 softmax, and is zero with lse = -inf exactly on the rows without a key"""
    B, Hkv, G, Nq = (shape[x] for x in ("B", "Hkv", "G", "Nq"))
    out, lse = cm.expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal, scale=scale)
    assert np.isfinite(out).all() and not np.isnan(lse).any()
    ref = cm.expected_f64(q, k, v, lens, B, Hkv, G, Nq, causal, scale=scale)[0]
    assert np.abs(out - ref).max() <= 1e-5 * max(1.0, np.abs(v).max())
    dead = np.array([[c == 0 for c in cm.row_limits(cm.clamp(lens[b], k.shape[1]), Nq, Nq, causal)[1]] for b in range(B)])
    dead = np.repeat(dead, Hkv * G, axis=0)
    assert np.array_equal(np.isneginf(lse), dead) and (out[dead] == 0.0).all()
    return out, lse


@pytest.mark.parametrize("d", [64, 128])
def test_split_counts(fa, d):
    """S = 129, 5, 4, 4 and 8 for the shapes of cases A to E, the paged entry's equal to the contiguous one's, and the plain
    split-KV shapes of A and D."""
    assert _kv_splits(fa, di.A_SHAPE, d) == di.A_SPLITS == 129
    assert _kv_splits(fa, di.B_SHAPE, d) == di.B_SPLITS == 5
    assert _kv_splits(fa, di.C_SHAPE, d) == di.C_SPLITS == 4
    assert _kv_splits(fa, di.D_SHAPE, d) == 4
    for shape, pages in ((di.A_SHAPE, (di.A_PAGE,)), (di.B_SHAPE, di.B_PAGES), (di.C_SHAPE, di.C_PAGES), (di.D_SHAPE, (di.D_PAGE,))):
        B, Hkv, G, Nq, Ncap = (shape[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
        for ps in pages:
            assert Ncap % ps == 0
            assert fa.kvcache_paged_workspace_bytes(B, Hkv, G, Nq, Ncap // ps, ps, d) == fa.kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
    s = di.A_SPLITKV
    assert di.splits_of(fa.splitkv_workspace_bytes(1, s["bh"], s["nq"], s["nk"], d), s["bh"], s["nq"], d) == 129
    assert fa.splitkv_workspace_bytes(1, 2, 5, 100, d) == 0
    assert di.splits_of(fa.splitkv_workspace_bytes(1, 2, 3, 8229, d), 2, 3, d) > 1
    if d == 128:
        e = di.E_CONTIG
        assert fa.kvcache_workspace_bytes(e["B"], 1, 1, 1, e["Ncap"], d) == 0   # 8200 heads fill the machine: one pass
        p = di.E_PAGED
        assert di.splits_of(fa.kvcache_paged_workspace_bytes(p["B"], 1, 1, 1, p["max_pages"], p["ps"], d), p["B"], 1, d) == 8


def test_case_a_lengths():
    """33024 keys: 129 splits of four tiles, all live; 20001 keys: 313 tiles, three per split, 105 live splits and 24 empty."""
    S = di.A_SPLITS
    assert di.A_SHAPE["Ncap"] == 129 * di.A_PAGE
    assert di.chunk_of(33024, S) == 256 and di.live_splits(33024, S) == 129
    assert -(-20001 // 64) == 313 and di.chunk_of(20001, S) == 192 and di.live_splits(20001, S) == 105
    assert di.chunk_of(33000, S) == 256 and di.live_splits(33000, S) == 129 and 33000 % 64 != 0


@pytest.mark.parametrize("entry", ["kvcache", "splitkv"])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_case_a_spikes(oracle, fmt, d, entry):
    """The +150 keys fall into splits 100, 80 and 128 (past the first trip of the merge's max loop), the +40 key into split 10."""
    shape = dict(di.A_SHAPE, Ncap=di.A_SPLITKV["nk"]) if entry == "splitkv" else di.A_SHAPE
    for spiked in (False, True):
        case = di.case_a(oracle, d, fmt, entry, spiked)
        di.assert_case_a(case, di.A_SPLITS)
        out, lse = _self_consistent(oracle, case["q"], case["k"], case["v"], case["lens"], shape, False)
        if spiked:
            assert [di.split_of(key, case["lens"][b], di.A_SPLITS) for (b, key, _) in case["spikes"]] == \
                [100, 10, 80 if entry == "kvcache" else 128]
            for b in range(2):   # one-hot rows: O is the V row of the highest key
                key = max((lift, key) for (bb, key, lift) in case["spikes"] if bb == b)[1]
                assert np.abs(out[b, 0] - case["v"][b, key]).max() < 1e-6


def test_case_b_rows():
    """160 folded rows in two query blocks with head edges inside waves; at 1030 keys rows 0-13 of every folded head are dead in
    split 4 and live in splits 0-3; at 7 keys rows 0-12 see nothing."""
    G, Nq = di.B_SHAPE["G"], di.B_SHAPE["Nq"]
    rows = G * Nq
    assert rows == 160 and cm.ROWS < rows <= 2 * cm.ROWS
    edges = [h * Nq for h in range(1, G)]
    assert any(e % 32 for e in edges) and any(e < cm.ROWS < e + Nq for e in [0] + edges)   # inside a wave; across the blocks
    S, L = di.B_SPLITS, di.B_LENS[0]
    assert di.chunk_of(L, S) == 256 and di.live_splits(L, S) == 5
    key0 = 4 * 256
    lim = cm.row_limits(L, Nq, Nq, True)[1]
    assert [c > key0 for c in lim] == [False] * 14 + [True] * 6 and min(lim) > 3 * 256 + 64
    assert [c == 0 for c in cm.row_limits(di.B_LENS[1], Nq, Nq, True)[1]] == [True] * 13 + [False] * 7
    assert di.B_LENS[1] < Nq and all(c == L for c in cm.row_limits(L, Nq, Nq, False)[1])


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_case_b_reference(oracle, fmt, d):
    s = di.B_SHAPE
    (q, k, v), _ = di.inputs(oracle, s["B"], s["Hkv"], s["G"], s["Nq"], s["Ncap"], d, fmt, 3300)
    for causal in (False, True):
        _self_consistent(oracle, q, k, v, di.B_LENS, s, causal)


def test_case_c_lengths():
    """One length per sequence; every category is there: below, at and above a tile edge, a chunk edge and a page edge of both
    page sizes, an empty split, an empty sequence, and both clamp directions with their extremes."""
    lens = di.c_lens()
    s = di.C_SHAPE
    assert len(lens) == s["B"] and set(di.C_FIXED) <= set(lens) and lens == di.c_lens()
    for k in range(1, 6):
        assert {64 * k - 1, 64 * k, 64 * k + 1} <= set(lens)
    cats = di.length_categories(lens, s["Ncap"], di.C_SPLITS, di.C_PAGES)
    assert cats >= di.c_categories_wanted(di.C_PAGES), di.c_categories_wanted(di.C_PAGES) - cats
    assert [cm.clamp(x, s["Ncap"]) for x in (-1, cm.INT_MIN, 1025, cm.INT_MAX)] == [0, 0, 1024, 1024]
    assert np.array(lens, dtype=np.int64).astype(np.int32).tolist() == list(lens)   # every one is an int32


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_case_c_reference(oracle, fmt, d):
    s = di.C_SHAPE
    (q, k, v), (_, kb, vb) = di.inputs(oracle, s["B"], s["Hkv"], s["G"], s["Nq"], s["Ncap"], d, fmt, 3400)
    lens = di.c_lens()
    for causal in (False, True):
        _self_consistent(oracle, q, k, v, lens, s, causal)
    # the hygiene helpers: NaN at and past the clamped length and nowhere else; garbage exactly in the dead table entries
    kc, vc = (x.reshape(s["B"], s["Hkv"], s["Ncap"], d) for x in (kb, vb))
    cache = cm.poisoned(kc, lens)
    for ps in di.C_PAGES:
        kp, vp, table = cm.scatter(kc, vc, lens, ps, seed=ps)
        named = set()
        for b, raw in enumerate(lens):
            L = cm.clamp(raw, s["Ncap"])
            assert (cache[b, :, L:] == cm.NAN16).all() and np.array_equal(cache[b, 0, :L], kb[b, :L])
            n = di.live_pages(L, ps)
            assert all(x in cm.GARBAGE for x in table[b, n:]) and all(0 <= x < kp.shape[0] for x in table[b, :n])
            named |= set(int(x) for x in table[b, :n])
            for pi in range(n):
                r = min(ps, L - pi * ps)
                assert np.array_equal(kp[table[b, pi], 0, :r], kb[b, pi * ps:pi * ps + r]) and (vp[table[b, pi], 0, r:] == cm.NAN16).all()
        unnamed = sorted(set(range(kp.shape[0])) - named)
        assert unnamed and (kp[unnamed] == cm.NAN16).all() and (vp[unnamed] == cm.NAN16).all()


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_case_d_reference(oracle, fmt, d):
    """At scale 0 the oracle gives the mean of the visible V rows and ln(their number); at 0.3 and -0.2 a finite softmax."""
    s = di.D_SHAPE
    assert set((0, 2, 66, 200, 1024)) <= set(di.D_LENS) and len(di.D_LENS) == s["B"] and set(di.D_SCALES) == {0.3, -0.2, 0.0}
    (q, k, v), _ = di.inputs(oracle, s["B"], s["Hkv"], s["G"], s["Nq"], s["Ncap"], d, fmt, 3500)
    for causal in (False, True):
        for scale in di.D_SCALES:
            out, lse = _self_consistent(oracle, q, k, v, di.D_LENS, s, causal, scale)
            if scale == 0.0:
                uo, ul = cm.uniform_expected(v, di.D_LENS, s["B"], s["Hkv"], s["G"], s["Nq"], causal)
                live = np.isfinite(ul)
                assert np.abs(out - uo).max() < 1e-6 and np.array_equal(live, np.isfinite(lse)) and np.abs(lse[live] - ul[live]).max() < 1e-12
    f = di.D_FORWARD
    (q, k, v), _ = oracle.make_qkv(f["bh"], f["n"], f["d"], fmt=fmt, seed=3600)
    for causal in (False, True):
        want = oracle.forward(q, k, v, scale=0.0, accum=1, nthreads=4, causal=causal)
        mean = np.cumsum(v.astype(np.float64), 1) / np.arange(1, f["n"] + 1)[None, :, None] if causal else \
            np.broadcast_to(v.astype(np.float64).mean(1, keepdims=True), v.shape)
        assert np.abs(want - mean).max() < 1e-6
    for (nq, nk) in di.D_SPLITKV:
        assert nk % 64 != 0   # a ragged last tile: the plain kernel masks keys there


def test_case_e_aliases():
    """Both tensors hold just over 2^32 elements; live heads and pages lie past 2^31 and past 2^32 elements, and the places a
    wrapped offset would land in are known, low and not live."""
    e = di.E_CONTIG
    head = e["Ncap"] * e["d"]
    assert e["B"] * e["Hkv"] * head > 2 ** 32 and (e["B"] - 8) * head <= 2 ** 32
    live = [b for (b, _) in di.E_CONTIG_LIVE]
    assert any(2 ** 31 <= b * head < 2 ** 32 for b in live) and any(b * head >= 2 ** 32 for b in live) and 0 in live
    assert di.wrap_aliases(live, head, e["B"]) == [1, 7]
    assert all(0 < L <= e["Ncap"] for (_, L) in di.E_CONTIG_LIVE)
    p = di.E_PAGED
    page = p["ps"] * p["d"] * p["Hkv"]
    assert p["num_pages"] * page > 2 ** 32 and (p["num_pages"] - 28) * page <= 2 ** 32
    pages = [x for row in di.E_PAGED_TABLE for x in row]
    assert len(set(pages)) == len(pages) and all(0 <= x < p["num_pages"] for x in pages)
    assert [len(row) for row in di.E_PAGED_TABLE] == [di.live_pages(L, p["ps"]) for L in di.E_PAGED_LENS]
    assert any(2 ** 31 <= x * page < 2 ** 32 for x in pages) and any(x * page >= 2 ** 32 for x in pages) and any(x < 8 for x in pages)
    al = di.wrap_aliases(pages, page, p["num_pages"])
    assert al == [7, 8, 9, 10, 11, 25, 26, 27] and not set(al) & set(pages)
