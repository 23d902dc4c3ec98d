"""Seeded inputs for tests/test_gpu_decode_edges.py -- the decode family (fa_forward_splitkv, fa_forward_kvcache,
fa_forward_kvcache_paged) at split-count, folded-mask, length, scale and addressing edges -- with the helpers that show each
input reaches the regime it is named for (tests/test_decode_inputs.py asserts them without a GPU).  Pure numpy plus the `oracle`
fixture (tests/conftest.py); nothing here touches a GPU.

Method of tests/test_gpu_kvcache.py and tests/test_gpu_kvcache_paged.py: inputs from oracle.make_qkv, expected O from
oracle.forward_cross on the keys a row sees (zeros for a row that sees none), expected log-sum-exps from float64 numpy on the same
16-bit-rounded inputs.  The bounds, the row limits, the references, the poison and the page scatter are tests/common_inputs.py's;
here are the cases, and the host's and the kernel's split arithmetic restated.
"""
import functools

import numpy as np

import common_inputs as cm
import fallback_inputs as fi

# ---- the arithmetic of the host and of the kernel, restated ---------------------------------------------------------------------
def splits_of(ws_bytes, bh, rows, d):
    """the split count S a workspace size stands for: S * BH * rows rows of d + 2 floats (0 bytes: one pass)"""
    row = bh * rows * (d + 2) * 4
    assert ws_bytes % row == 0
    return max(ws_bytes // row, 1)


def chunk_of(L, S):
    """keys per split of a sequence of L keys: its tiles dealt out to S splits"""
    return -(-(-(-L // cm.TILE)) // S) * cm.TILE


def live_splits(L, S):
    return -(-L // chunk_of(L, S)) if L > 0 else 0


def split_of(key, L, S):
    return key // chunk_of(L, S)


def live_pages(L, ps):
    return (max(int(L), 0) + ps - 1) // ps


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, seed):
    """-> (q [B*Hkv*G, Nq, d], k, v [B*Hkv, Ncap, d]) fp32 16-bit-rounded, and their encodings; drawn once, read-only."""
    (q, _, _), (qb, _, _) = oracle.make_qkv(B * Hkv * G, Nq, d, fmt=fmt, seed=seed)
    (_, k, v), (_, kb, vb) = oracle.make_qkv(B * Hkv, Ncap, d, fmt=fmt, seed=seed + 1)
    for a in (q, k, v, qb, kb, vb):
        a.setflags(write=False)
    return (q, k, v), (qb, kb, vb)


# ---- A. more than 64 splits -----------------------------------------------------------------------------------------------------
A_SHAPE = dict(B=2, Hkv=1, G=1, Nq=1, Ncap=33024)
A_LENS = (33024, 20001)           # 516 tiles in 129 splits of 4; 313 tiles in 105 splits of 3 and 24 empty ones
A_PAGE = 256
A_SPLITS = 129
A_SPLITKV = dict(bh=2, nq=1, nk=33000)
# (sequence, key, lift in log2 units over the row's largest benign score).  Sequence 0 is the pair the case is named for: the row's
# maximum lies in a split the first trip of the merge's max loop does not read (index >= 64) and a second peak, 110 below it, in one
# it does.  2^110 is finite in fp32, so a merge whose M stops at split 63 still gets sequence 0 right (M cancels); sequence 1 has
# the high key ALONE: there such a merge weighs the split by 2^150 = inf.
A_SPIKES = {"kvcache": ((0, 100 * 256 + 37, 150.0), (0, 10 * 256 + 5, 40.0), (1, 80 * 192 + 11, 150.0)),
            "splitkv": ((0, 100 * 256 + 37, 150.0), (0, 10 * 256 + 5, 40.0), (1, 128 * 256 + 222, 150.0))}


@functools.lru_cache(maxsize=None)
def case_a(oracle, d, fmt, entry, spiked):
    """entry "kvcache": the A_SHAPE cache with lengths A_LENS; "splitkv": two heads of one query row against 33000 keys.
    -> dict q [2, 1, d], k, v [2, N, d], bits, lens, spikes"""
    n = A_SHAPE["Ncap"] if entry == "kvcache" else A_SPLITKV["nk"]
    lens = A_LENS if entry == "kvcache" else (n, n)
    (q, k, v), bits = inputs(oracle, 2, 1, 1, 1, n, d, fmt, 3100 + d + fmt)
    if not spiked:
        return dict(q=q, k=k, v=v, bits=bits, lens=lens, spikes=())
    k = k.copy()
    base = [fi.scores_log2(q, k[:, :lens[b]], b)[0].max() for b in range(2)]   # benign maxima, before any key is replaced
    for (b, key, lift) in A_SPIKES[entry]:
        fi._set_key(q, k, b, 0, b, key, base[b] + lift)
    (q, k, v), bits = fi._round(oracle, fmt, q, k, v)
    return dict(q=q, k=k, v=v, bits=bits, lens=lens, spikes=A_SPIKES[entry])


def assert_case_a(case, S):
    """every spiked key is visible, lies as far above the row's other keys as it was built to, and falls into a split on the side
    of index 64 it was built for; sequence 0 has one on each side, sequence 1 the high one alone"""
    q, k, lens = case["q"], case["k"], case["lens"]
    assert S == A_SPLITS and S > 64 and S % 4 == 1 and S % 2 == 1   # a remainder for four slices (d = 64) and for two (d = 128)
    side = {}
    for (b, key, lift) in case["spikes"]:
        L = lens[b]
        assert 0 <= key < L
        s = fi.scores_log2(q, k[:, :L], b)[0]
        others = [kk for (bb, kk, _) in case["spikes"] if bb == b]
        rest = np.delete(s, others).max()
        assert abs(s[key] - rest - lift) < 1.0, (b, key, s[key] - rest)
        sp = split_of(key, L, S)
        assert sp < live_splits(L, S)
        assert (sp >= 64) == (lift > 100.0), (b, key, sp)
        side.setdefault(b, []).append(sp >= 64)
    if case["spikes"]:
        assert sorted(side[0]) == [False, True] and side[1] == [True]


# ---- B. the causal mask on folded heads -----------------------------------------------------------------------------------------
B_SHAPE = dict(B=2, Hkv=2, G=8, Nq=20, Ncap=1280)
B_LENS = (1030, 7)
B_SPLITS = 5
B_PAGES = (16, 256)


# ---- C. a sweep of lengths in one launch ----------------------------------------------------------------------------------------
C_SHAPE = dict(B=48, Hkv=1, G=2, Nq=3, Ncap=1024)
C_SPLITS = 4
C_PAGES = (16, 256)
C_FIXED = ((0, 1, 2, 15, 16, 17) + tuple(64 * k + e for k in range(1, 6) for e in (-1, 0, 1))
           + (511, 512, 513, 767, 768, 769, 1023, 1024) + (-1, cm.INT_MIN, 1025, cm.INT_MAX))


def c_lens():
    rest = np.random.default_rng(4242).integers(3, 1023, C_SHAPE["B"] - len(C_FIXED))
    return C_FIXED + tuple(int(x) for x in rest)


def length_categories(lens, ncap, S, pages):
    """the set of edge categories a list of raw lengths covers"""
    cats = set()
    edge = {0: "at", 1: "above"}
    for raw in lens:
        if raw < 0:
            cats.add("clamped up" + (" from INT_MIN" if raw == cm.INT_MIN else ""))
            continue
        if raw > ncap:
            cats.add("clamped down" + (" from INT_MAX" if raw == cm.INT_MAX else ""))
            continue
        L = raw
        if L == 0:
            cats.add("empty")
            continue
        if live_splits(L, S) < S:
            cats.add("empty split")
        for name, unit in [("tile", cm.TILE), ("chunk", chunk_of(L, S))] + [(f"page{ps}", ps) for ps in pages]:
            if L % unit in edge and (L > unit or L % unit == 0):
                cats.add(f"{edge[L % unit]} {name} edge")
            if L % unit == unit - 1:
                cats.add(f"below {name} edge")
    return cats


def c_categories_wanted(pages):
    want = {"clamped up", "clamped up from INT_MIN", "clamped down", "clamped down from INT_MAX", "empty", "empty split"}
    for name in ["tile", "chunk"] + [f"page{ps}" for ps in pages]:
        want |= {f"{e} {name} edge" for e in ("below", "at", "above")}
    return want


# ---- D. scale -------------------------------------------------------------------------------------------------------------------
D_SHAPE = dict(C_SHAPE, B=8)
D_LENS = (0, 2, 66, 200, 1024, 1, 513, 777)
D_SCALES = (0.3, -0.2, 0.0)
D_PAGE = 16
D_SPLITKV = ((5, 100), (3, 8229))     # (nq, nk), two heads each: one pass with a ragged last tile; 26 splits and the merge
D_FORWARD = dict(bh=2, n=100, d=64)   # fa_forward at scale 0: ragged N, with and without the mask


# ---- E. addresses past 2^32 elements --------------------------------------------------------------------------------------------
E_CONTIG = dict(B=8200, Hkv=1, G=1, Nq=1, Ncap=4096, d=128)
E_CONTIG_LIVE = ((0, 4096), (4097, 100), (8193, 77), (8199, 4096))   # (sequence, length); every other length is 0
E_PAGED = dict(B=2, Hkv=1, G=1, Nq=1, ps=256, max_pages=8, num_pages=131100, d=128)
E_PAGED_LENS = (2048, 3 * 256 + 77)
E_PAGED_TABLE = ((5, 65543, 131081, 131099, 6, 65544, 131082, 131098), (131097, 65545, 4, 131083))   # live entries


def wrap_aliases(live, unit_elems, total_units):
    """Where a wrapped offset would land: for every live unit (a K/V head, or a page: unit_elems 16-bit elements each) the units
    u mod W for W = 2^31 bytes, 2^32 bytes (= 2^31 elements) and 2^32 elements, where that is another unit and not a live one."""
    out = set()
    for w_elems in (2 ** 30, 2 ** 31, 2 ** 32):
        W = w_elems // unit_elems
        assert W * unit_elems == w_elems
        for u in live:
            assert 0 <= u < total_units
            if u % W != u and u % W not in live:
                out.add(u % W)
    return sorted(out)
