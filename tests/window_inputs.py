"""Seeded inputs for tests/test_gpu_kvcache_window.py -- the sliding-window decode entries (fa_forward_kvcache_window and its paged,
fp8 and paged-fp8 forms) -- with the window's semantics and the host's and the kernel's range arithmetic restated, and the helpers
that show each case reaches the regime it is named for (tests/test_window_inputs.py asserts them without a GPU).  Pure numpy plus
the `oracle` fixture (tests/conftest.py); nothing here touches a GPU.

Method of tests/decode_inputs.py: inputs from oracle.make_qkv, expected O from oracle.forward_cross on the keys a row sees (zeros
for a row that sees none), expected log-sum-exps from float64 numpy on the same 16-bit-rounded inputs.  What is new here is the
lower limit of a row and what follows from it: where a sequence's stream starts, which rows and pages are never used, and the
split count that follows from the window in place of the capacity.
"""
import functools

import numpy as np

import decode_inputs as di

TILE = di.TILE
NAN8 = 0x7F        # the e4m3fn NaN code the fp8 caches are poisoned with
MIN_TILES = 4      # fewest tiles per split, and
TARGET = 1024      # the workgroup target of the library's split rule (split_count, restated below)


# ---- the semantics ----------------------------------------------------------------------------------------------------------------
def limits(L, nq, causal):
    """c_i: first key row i does not see (the base entries' limit)"""
    return di.limits(L, nq, causal)


def lows(L, nq, W):
    """lo_i: first key row i sees; the same with and without the causal mask.  W = 0: no window."""
    return [max(0, L - nq + 1 + i - W) if W else 0 for i in range(nq)]


def start_of(L, nq, W):
    """start_b: row 0's lower limit -- no row of the sequence sees a key below it"""
    return lows(L, nq, W)[0]


# ---- the host's and the kernel's arithmetic, restated -----------------------------------------------------------------------------
def span_cap(nq, ncap, W):
    """the longest range a sequence can stream, in keys: what takes the capacity's place in the split rule"""
    need = W + nq - 1
    return ncap if need >= ncap else min(ncap, -(-need // TILE) * TILE + TILE)


def split_count(bh, rows, nk):
    """the library's split rule for `nk` keys (from the shape alone)"""
    base = bh * -(-rows // di.ROWS)
    tiles = -(-nk // TILE)
    s = max(min(-(-TARGET // base), tiles // MIN_TILES), 1)
    chunk_tiles = -(-tiles // s)
    return -(-tiles // chunk_tiles)


def splits(bh, rows, nq, ncap, W):
    return split_count(bh, rows, span_cap(nq, ncap, W))


def start_tile(L, nq, W):
    return start_of(L, nq, W) // TILE * TILE


def chunk_of(L, nq, W, S):
    """keys per split: the tiles from the start tile to the length, dealt out to S splits"""
    return -(-(-(-(L - start_tile(L, nq, W)) // TILE)) // S) * TILE


def live_splits(L, nq, W, S):
    """splits with key0 < L"""
    if L == 0:
        return 0
    return -(-(L - start_tile(L, nq, W)) // chunk_of(L, nq, W, S))


def categories(lens, nq, ncap, W, S, causal, pages=()):
    """the set of regimes the sequences of one launch reach"""
    cats = {"split" if S > 1 else "one pass"}
    for raw in lens:
        L = di.clamp(raw, ncap)
        sb = start_of(L, nq, W)
        lim, lo = limits(L, nq, causal), lows(L, nq, W)
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
            cats.add("start on a tile edge" if sb % TILE == 0 else "start inside a tile")
            if sb % TILE:
                cats.add("first tile holds rows below the start")
            for ps in pages:
                cats.add(f"start on a page{ps} edge" if sb % ps == 0 else f"start inside a page{ps}")
                if sb >= ps:
                    cats.add(f"dead page{ps} below the start")
        if len(set(lo)) > 1 and max(lo) // TILE == min(lo) // TILE and max(lim) - min(lo) <= TILE:
            cats.add("rows with different lower limits in one tile")
    return cats


# ---- inputs and poison --------------------------------------------------------------------------------------------------------------
inputs = di.inputs


def poisoned(bits, lens, nq, W, nan=di.NAN16):
    """[B, Hkv, Ncap, d] (or [B*Hkv, Ncap, d] with B given by len(lens)) encodings -> a copy [B, Hkv, Ncap, d] with NaN in every row at
    and past the sequence's length AND in every row below start_b"""
    B = len(lens)
    out = np.array(bits).reshape(B, -1, bits.shape[-2], bits.shape[-1]).copy()
    for b in range(B):
        L = di.clamp(lens[b], out.shape[2])
        out[b, :, L:] = nan
        out[b, :, :start_of(L, nq, W)] = nan
    return out


def scatter(kc, vc, lens, nq, W, ps, seed, nan=di.NAN16, spare=3):
    """K and V caches [B, Hkv, Ncap, d] (16-bit encodings or fp8 codes) -> (K pool, V pool [num_pages, Hkv, ps, d], table
    [B, max_pages] int32).  tests/decode_inputs.py::scatter with the window's contract: a page that lies wholly below start_b gets
    no pool page -- its table entry holds garbage, like the entries past the last live page -- and the rows below start_b of the
    page that straddles it hold NaN, like the rows at and past the length.  Pages no table names hold NaN."""
    B, Hkv, Ncap, d = kc.shape
    max_pages = Ncap // ps
    assert max_pages * ps == Ncap
    num_pages = B * max_pages + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    pools = [np.full((num_pages, Hkv, ps, d), nan, kc.dtype) for _ in range(2)]
    table = np.empty((B, max_pages), np.int32)
    nxt = 0
    for b in range(B):
        L = di.clamp(lens[b], Ncap)
        sb = start_of(L, nq, W)
        for pi in range(max_pages):
            if pi >= di.live_pages(L, ps) or (pi + 1) * ps <= sb:
                table[b, pi] = di.GARBAGE[pi % 2]
                continue
            page = int(perm[nxt])
            nxt += 1
            table[b, pi] = page
            r0, r1 = max(sb - pi * ps, 0), min(ps, L - pi * ps)   # the page's rows inside [start_b, L); the rest stay NaN
            for pool, src in zip(pools, (kc, vc)):
                pool[page, :, r0:r1] = src[b, :, pi * ps + r0:pi * ps + r1]
    return pools[0], pools[1], table


# ---- references -------------------------------------------------------------------------------------------------------------------
def expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal, W, scale=None):
    """q [B*Hkv*G, Nq, d], k/v [B*Hkv, Ncap, d] fp32 (16-bit-rounded) -> (O [B*Hq, Nq, d] fp32, lse [B*Hq, Nq] float64).
    O from oracle.forward_cross (float64 accumulators) on k[:, lo:c], grouped by the distinct (lo, c) of a sequence's rows, lse from
    float64 numpy; a row without a key is zeros and -inf."""
    Hq, d, Ncap = Hkv * G, q.shape[2], k.shape[1]
    out = np.zeros(q.shape, np.float32)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b in range(B):
        qs = slice(b * Hq, (b + 1) * Hq)
        kb, vb = (np.repeat(x[b * Hkv:(b + 1) * Hkv], G, axis=0) for x in (k, v))   # K/V head of every query head
        L = di.clamp(lens[b], Ncap)
        rng = list(zip(lows(L, Nq, W), limits(L, Nq, causal)))
        for (lo, c) in sorted(set(rng)):
            if c == 0:
                continue
            rows = [i for i in range(Nq) if rng[i] == (lo, c)]
            qr = np.ascontiguousarray(q[qs][:, rows])
            out[qs, rows] = oracle.forward_cross(qr, np.ascontiguousarray(kb[:, lo:c]), np.ascontiguousarray(vb[:, lo:c]), scale=sc,
                                                 accum=1, nthreads=8)
            s = np.einsum("hid,hjd->hij", qr.astype(np.float64), kb[:, lo:c].astype(np.float64)) * sc
            m = s.max(-1)
            lse[qs, rows] = m + np.log(np.exp(s - m[..., None]).sum(-1))
    return out, lse


def expected_f64(q, k, v, lens, B, Hkv, G, Nq, causal, W, scale=None):
    """expected() without the oracle: softmax(q k^T scale) v over [lo_i, c_i) in float64 numpy, row by row"""
    Hq, d, Ncap = Hkv * G, q.shape[2], k.shape[1]
    out = np.zeros(q.shape, np.float64)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b in range(B):
        L = di.clamp(lens[b], Ncap)
        lim, lo = limits(L, Nq, causal), lows(L, Nq, W)
        for h in range(Hq):
            kk, vv = (x[b * Hkv + h // G].astype(np.float64) for x in (k, v))
            for i in range(Nq):
                if lim[i]:
                    s = (kk[lo[i]:lim[i]] @ q[b * Hq + h, i].astype(np.float64)) * sc
                    p = np.exp(s - s.max())
                    out[b * Hq + h, i] = (p / p.sum()) @ vv[lo[i]:lim[i]]
                    lse[b * Hq + h, i] = s.max() + np.log(p.sum())
    return out, lse


def uniform_expected(v, lens, B, Hkv, G, Nq, causal, W):
    """what scale 0 must give: O is the mean of the V rows in [lo_i, c_i), lse = ln(their number)"""
    Hq, Ncap = Hkv * G, v.shape[1]
    out = np.zeros((B * Hq, Nq, v.shape[2]), np.float64)
    lse = np.full((B * Hq, Nq), -np.inf, np.float64)
    for b in range(B):
        L = di.clamp(lens[b], Ncap)
        for i, (lo, c) in enumerate(zip(lows(L, Nq, W), limits(L, Nq, causal))):
            if c:
                for h in range(Hq):
                    out[b * Hq + h, i] = v[b * Hkv + h // G, lo:c].astype(np.float64).mean(0)
                lse[b * Hq:(b + 1) * Hq, i] = np.log(c - lo)
    return out, lse


@functools.lru_cache(maxsize=None)
def reference(oracle, case, d, fmt, W, causal):
    """expected() of a case of CASES, computed once and read-only"""
    c = CASES[case]
    (q, k, v), _ = inputs(oracle, c["B"], c["Hkv"], c["G"], c["Nq"], c["Ncap"], d, fmt, c["seed"])
    out, lse = expected(oracle, q, k, v, c["lens"], c["B"], c["Hkv"], c["G"], c["Nq"], causal, W)
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
