"""Seeded inputs for tests/test_gpu_decode_edges.py -- the decode family (fa_forward_splitkv, fa_forward_kvcache,
fa_forward_kvcache_paged) at split-count, folded-mask, length, scale and addressing edges -- with the helpers that show each
input reaches the regime it is named for (tests/test_decode_inputs.py asserts them without a GPU).  Pure numpy plus the `oracle`
fixture (tests/conftest.py); nothing here touches a GPU.

Method of tests/test_gpu_kvcache.py and tests/test_gpu_kvcache_paged.py: inputs from oracle.make_qkv, expected O from
oracle.forward_cross on the keys a row sees (zeros for a row that sees none), expected log-sum-exps from float64 numpy on the same
16-bit-rounded inputs.  What is new here is the `scale` argument and the clamp of a bad length: the reference of a length outside
[0, Ncap] is the one of min(max(L, 0), Ncap).
"""
import functools

import numpy as np

import fallback_inputs as fi

# The project's bounds.  Copies: tests/test_gpu_parity.py (the origin), tests/test_gpu_kvcache.py, tests/test_gpu_kvcache_paged.py and
# tests/test_gpu_fallback_paths.py define the same values; a change to the bounds has to be made in all of them.
MAX_ABS = 1e-2                          # the project's north-star tolerance (tests/test_gpu_parity.py)
REL_L2 = {0: 2e-3, 1: 1.2e-2}           # fp16 / bf16 inputs
P_EPS = {0: 2.0 ** -11, 1: 2.0 ** -8}   # largest relative rounding error of one weight in the format P is packed to
NAN16 = 0x7FFF                          # a NaN in fp16 and in bf16
GARBAGE = (-1, 1 << 30)                 # what a table holds past a sequence's last live page
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
TILE = 64                               # kBlockN
ROWS = 128                              # split::kRows, query rows per workgroup
FMT_NAME = {0: "fp16", 1: "bf16"}


def peaked_tol(fmt, vmax, kernels=1):
    """tests/test_gpu_parity.py::_peaked_tol: the north-star bar plus what the 16-bit format of P imposes on a peaked row."""
    return MAX_ABS + kernels * float(vmax) * P_EPS[fmt]


# ---- the arithmetic of the host and of the kernel, restated ---------------------------------------------------------------------
def clamp(L, ncap):
    """the kernel's min(max(L, 0), Ncap)"""
    return min(max(int(L), 0), ncap)


def limits(L, nq, causal):
    """c_i: the number of keys row i of a head sees (the mask is aligned to the end of the sequence)."""
    return [max(0, L - nq + 1 + i) if causal else L for i in range(nq)]


def splits_of(ws_bytes, bh, rows, d):
    """the split count S a workspace size stands for: S * BH * rows rows of d + 2 floats (0 bytes: one pass)"""
    row = bh * rows * (d + 2) * 4
    assert ws_bytes % row == 0
    return max(ws_bytes // row, 1)


def chunk_of(L, S):
    """keys per split of a sequence of L keys: its tiles dealt out to S splits"""
    return -(-(-(-L // TILE)) // S) * TILE


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


def scatter(kb, vb, lens, B, Hkv, ps, seed, spare=3):
    """K and V encodings [B*Hkv, Ncap, d] -> (K pool, V pool [num_pages, Hkv, ps, d] uint16, table [B, max_pages] int32).
    Pages are dealt out by a seeded permutation of a pool with `spare` pages more than B * max_pages.  Every page no table names
    and every row at or past a (clamped) length holds NaN; every table entry past the last live page holds garbage.  A sequence
    whose raw length exceeds the capacity is full: all its entries are live and all its rows valid."""
    Ncap, d = kb.shape[1], kb.shape[2]
    max_pages = Ncap // ps
    assert max_pages * ps == Ncap
    num_pages = B * max_pages + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    pools = [np.full((num_pages, Hkv, ps, d), NAN16, np.uint16) for _ in range(2)]
    table = np.empty((B, max_pages), np.int32)
    nxt = 0
    for b in range(B):
        L = clamp(lens[b], Ncap)
        for pi in range(max_pages):
            if pi >= live_pages(L, ps):
                table[b, pi] = GARBAGE[pi % 2]
                continue
            page = int(perm[nxt])
            nxt += 1
            table[b, pi] = page
            n = min(ps, L - pi * ps)   # rows of the page below the length; the rest stay NaN
            for pool, src in zip(pools, (kb, vb)):
                pool[page, :, :n] = src[b * Hkv:(b + 1) * Hkv, pi * ps:pi * ps + n]
    return pools[0], pools[1], table


def poisoned(bits, lens, B, Hkv):
    """[B*Hkv, Ncap, d] encodings -> cache [B, Hkv, Ncap, d] with NaN in every row at and past the sequence's (clamped) length"""
    bits = bits.reshape(B, Hkv, bits.shape[1], bits.shape[2]).copy()
    for b in range(B):
        bits[b, :, clamp(lens[b], bits.shape[2]):] = NAN16
    return bits


def expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal, scale=None):
    """q [B*Hkv*G, Nq, d], k/v [B*Hkv, Ncap, d] fp32 (16-bit-rounded) -> (O [B*Hq, Nq, d] fp32, lse [B*Hq, Nq] float64).
    O from oracle.forward_cross (float64 accumulators) on the keys a row sees, lse from float64 numpy; a row without a key is
    zeros and -inf.  A length outside [0, Ncap] counts as the clamped one."""
    Hq, d, Ncap = Hkv * G, q.shape[2], k.shape[1]
    out = np.zeros(q.shape, np.float32)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b in range(B):
        qs = slice(b * Hq, (b + 1) * Hq)
        kb, vb = (np.repeat(x[b * Hkv:(b + 1) * Hkv], G, axis=0) for x in (k, v))   # K/V head of every query head
        lim = limits(clamp(lens[b], Ncap), Nq, causal)
        for c in sorted(set(lim)):
            if c == 0:
                continue
            rows = [i for i in range(Nq) if lim[i] == c]
            qr = np.ascontiguousarray(q[qs][:, rows])
            out[qs, rows] = oracle.forward_cross(qr, np.ascontiguousarray(kb[:, :c]), np.ascontiguousarray(vb[:, :c]), scale=sc,
                                                 accum=1, nthreads=8)
            s = np.einsum("hid,hjd->hij", qr.astype(np.float64), kb[:, :c].astype(np.float64)) * sc
            m = s.max(-1)
            lse[qs, rows] = m + np.log(np.exp(s - m[..., None]).sum(-1))
    return out, lse


def expected_f64(q, k, v, lens, B, Hkv, G, Nq, causal, scale=None):
    """expected() without the oracle: softmax(q k^T scale) v in float64 numpy.  The CPU tier holds the oracle's O against it."""
    Hq, d, Ncap = Hkv * G, q.shape[2], k.shape[1]
    out = np.zeros(q.shape, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b in range(B):
        L = clamp(lens[b], Ncap)
        lim = limits(L, Nq, causal)
        for h in range(Hq):
            kk, vv = (x[b * Hkv + h // G, :L].astype(np.float64) for x in (k, v))
            s = (q[b * Hq + h].astype(np.float64) @ kk.T) * sc
            for i, c in enumerate(lim):
                if c:
                    p = np.exp(s[i, :c] - s[i, :c].max())
                    out[b * Hq + h, i] = (p / p.sum()) @ vv[:c]
    return out


def uniform_expected(v, lens, B, Hkv, G, Nq, causal):
    """what scale 0 must give: every visible key weighs the same -- O is the mean of the visible V rows, lse = ln(their number)"""
    Hq, Ncap = Hkv * G, v.shape[1]
    out = np.zeros((B * Hq, Nq, v.shape[2]), np.float64)
    lse = np.full((B * Hq, Nq), -np.inf, np.float64)
    for b in range(B):
        for i, c in enumerate(limits(clamp(lens[b], Ncap), Nq, causal)):
            if c:
                for h in range(Hq):
                    out[b * Hq + h, i] = v[b * Hkv + h // G, :c].astype(np.float64).mean(0)
                lse[b * Hq:(b + 1) * Hq, i] = np.log(c)
    return out, lse


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
           + (511, 512, 513, 767, 768, 769, 1023, 1024) + (-1, INT_MIN, 1025, INT_MAX))


def c_lens():
    rest = np.random.default_rng(4242).integers(3, 1023, C_SHAPE["B"] - len(C_FIXED))
    return C_FIXED + tuple(int(x) for x in rest)


def length_categories(lens, ncap, S, pages):
    """the set of edge categories a list of raw lengths covers"""
    cats = set()
    edge = {0: "at", 1: "above"}
    for raw in lens:
        if raw < 0:
            cats.add("clamped up" + (" from INT_MIN" if raw == INT_MIN else ""))
            continue
        if raw > ncap:
            cats.add("clamped down" + (" from INT_MAX" if raw == INT_MAX else ""))
            continue
        L = raw
        if L == 0:
            cats.add("empty")
            continue
        if live_splits(L, S) < S:
            cats.add("empty split")
        for name, unit in [("tile", TILE), ("chunk", chunk_of(L, S))] + [(f"page{ps}", ps) for ps in pages]:
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
