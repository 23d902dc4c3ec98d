"""Seeded inputs for tests/test_gpu_kvcache_window.py -- the sliding-window decode entries (fa_forward_kvcache_window and its paged,
fp8 and paged-fp8 forms) -- with the host's and the kernel's range arithmetic restated, and the helpers
that show each case reaches the regime it is named for (tests/test_window_inputs.py asserts them without a GPU).  Pure numpy plus
the `oracle` fixture (tests/conftest.py); nothing here touches a GPU.

Method of tests/decode_inputs.py.  The lower limit of a row itself, the references, the poison and the page scatter under a window
are tests/common_inputs.py's (the `W` argument); here is what follows from the lower limit on the host and in the kernel: where a
sequence's stream starts, which rows and pages are never used, and the split count that follows from the window in place of the
capacity.
"""
import functools

import common_inputs as cm
import decode_inputs as di

NAN8 = 0x7F        # the e4m3fn NaN code the fp8 caches are poisoned with
MIN_TILES = 4      # fewest tiles per split, and
TARGET = 1024      # the workgroup target of the library's split rule (split_count, restated below)


def start_of(L, nq, W):
    """start_b: row 0's lower limit -- no row of the sequence sees a key below it (W = 0: no window)"""
    return int(cm.row_limits(L, nq, nq, False, W)[0][0])


# ---- the host's and the kernel's arithmetic, restated -----------------------------------------------------------------------------
def span_cap(nq, ncap, W):
    """the longest range a sequence can stream, in keys: what takes the capacity's place in the split rule"""
    need = W + nq - 1
    return ncap if need >= ncap else min(ncap, -(-need // cm.TILE) * cm.TILE + cm.TILE)


def split_count(bh, rows, nk):
    """the library's split rule for `nk` keys (from the shape alone)"""
    base = bh * -(-rows // cm.ROWS)
    tiles = -(-nk // cm.TILE)
    s = max(min(-(-TARGET // base), tiles // MIN_TILES), 1)
    chunk_tiles = -(-tiles // s)
    return -(-tiles // chunk_tiles)


def splits(bh, rows, nq, ncap, W):
    return split_count(bh, rows, span_cap(nq, ncap, W))


def start_tile(L, nq, W):
    return start_of(L, nq, W) // cm.TILE * cm.TILE


def chunk_of(L, nq, W, S):
    """keys per split: the tiles from the start tile to the length, dealt out to S splits"""
    return -(-(-(-(L - start_tile(L, nq, W)) // cm.TILE)) // S) * cm.TILE


def live_splits(L, nq, W, S):
    """splits with key0 < L"""
    if L == 0:
        return 0
    return -(-(L - start_tile(L, nq, W)) // chunk_of(L, nq, W, S))


def categories(lens, nq, ncap, W, S, causal, pages=()):
    """the set of regimes the sequences of one launch reach"""
    cats = {"split" if S > 1 else "one pass"}
    for raw in lens:
        L = cm.clamp(raw, ncap)
        sb = start_of(L, nq, W)
        lo, lim, _ = cm.row_limits(L, nq, nq, causal, W)
        assert all(l < c for l, c in zip(lo, lim) if c >= 1)
        if any(c == 0 for c in lim):
            cats.add("row without keys")
        if L == 0:
            continue
        if W > L:
            cats.add("window longer than the sequence")
        if live_splits(L, nq, W, S) < S:
            cats.add("empty split")
        if sb > 0:
            cats.add("start on a tile edge" if sb % cm.TILE == 0 else "start inside a tile")
            if sb % cm.TILE:
                cats.add("first tile holds rows below the start")
            for ps in pages:
                cats.add(f"start on a page{ps} edge" if sb % ps == 0 else f"start inside a page{ps}")
                if sb >= ps:
                    cats.add(f"dead page{ps} below the start")
        if len(set(lo)) > 1 and max(lo) // cm.TILE == min(lo) // cm.TILE and max(lim) - min(lo) <= cm.TILE:
            cats.add("rows with different lower limits in one tile")
    return cats


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
inputs = di.inputs


# ---- references -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(oracle, case, d, fmt, W, causal):
    """cm.expected() of a case of CASES, computed once and read-only"""
    c = CASES[case]
    (q, k, v), _ = inputs(oracle, c["B"], c["Hkv"], c["G"], c["Nq"], c["Ncap"], d, fmt, c["seed"])
    out, lse = cm.expected(oracle, q, k, v, c["lens"], c["B"], c["Hkv"], c["G"], c["Nq"], causal, W)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
PAGES = (16, 256)
CASES = {
    # 1. one pass: span_cap <= 320 keys = 5 tiles, so S = 1; an empty sequence; windows below, at and above a tile
    "one_pass": dict(B=4, Hkv=2, G=2, Nq=1, Ncap=512, lens=(512, 300, 65, 0), windows=(1, 63, 64, 65, 200), causal=(False,),
                     S=1, seed=5100),
    # 2. split and merge: 17 tiles in S = 4; 1500: start 476 inside a tile; 700: shorter than the window; 100: two live splits
    "split": dict(B=4, Hkv=1, G=1, Nq=1, Ncap=4096, lens=(4096, 1500, 700, 100), windows=(1024,), causal=(False,), S=4, seed=5200),
    # 3. several rows, folded heads, both masks: at 4 keys under the mask row 0 sees nothing; W = 3: one tile, rows' limits differ
    "rows": dict(B=2, Hkv=2, G=4, Nq=5, Ncap=1024, lens=(1000, 4), windows=(3, 64, 130), causal=(False, True), S=1, seed=5300),
}


# what a launch of a case must reach (tests/test_window_inputs.py holds categories() against it), and what the cases reach together
def wanted(case, W, causal):
    if case == "one_pass":
        extra = {64: {"start on a tile edge", "start on a page16 edge"}, 200: {"window longer than the sequence"}}
        return {"one pass", "row without keys", "first tile holds rows below the start", "start inside a tile",
                "dead page16 below the start", "dead page256 below the start"} | extra.get(W, set())
    if case == "split":
        return {"split", "empty split", "first tile holds rows below the start", "start inside a tile", "start on a tile edge",
                "start on a page16 edge", "start on a page256 edge", "start inside a page16", "start inside a page256",
                "window longer than the sequence", "dead page16 below the start", "dead page256 below the start"}
    return {"one pass", "first tile holds rows below the start"} | ({"row without keys"} if causal else set()) \
        | ({"rows with different lower limits in one tile"} if W == 3 else {"window longer than the sequence"})


WANTED_TOGETHER = {"one pass", "split", "empty split", "first tile holds rows below the start", "start on a tile edge",
                   "start inside a tile", "row without keys", "window longer than the sequence",
                   "rows with different lower limits in one tile"} \
    | {f"start {w} page{ps}{e}" for ps in PAGES for (w, e) in (("on a", " edge"), ("inside a", ""))}

# 6. the shift tie: a window of 1024 over a cache of 4096 against fa_forward_kvcache on a cache of 1088 that holds the last 1024 keys
SHIFT = dict(B=2, Hkv=1, G=1, Nq=1, Ncap=4096, W=1024, lens=(4096, 1792), seed=5400)
# 7. the graph: one sequence steps from below W across L = W and across a tile edge (Ncap 256, W = 60: lengths 58 -> 66)
GRAPH = dict(B=2, Hkv=2, G=2, Ncap=256, W=60, start=(57, 130), steps=9, seed=5500)
