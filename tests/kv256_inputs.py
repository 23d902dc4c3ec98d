"""Shapes, builders, limits and a numpy model for the edge tiers of fa_kvcache_decode_d256 (tests/test_gpu_kv256_edges.py;
tests/test_kv256_inputs.py asserts everything here without a GPU).  Pure numpy plus the `oracle` fixture; nothing here touches a GPU.

The kernel (csrc/fa_fwd_kv256_kernel.hpp) shares no tile code with the d = 64 / 128 stream: 64-key tiles from start_t = start_b
rounded down to a tile, dealt to S splits of chunk = ceil(ceil((L - start_t) / 64) / S) * 64 keys; the G * n_b rows of a
(sequence, K/V head) folded as p = hd * n_b + i into 32-row blocks that vote together; a lazy reference maximum (kThr = 8); a
private merge that weighs the partials by 2^(m_s - M).  Four families of inputs:

  A. census   K = 0, coded V (census_inputs): every visible key counted once, decided between neighbouring integers
  B. range    hostile logits in the mould of softmax_range_inputs.MLA, with model() -- the scheme restated on sr.lazy_pass /
              finish / merge -- so that the CPU tier can show that the check accepts the scheme and rejects the seven sr.DEFECTS
  C. random   lengths, rows, scales and the library's own split count, against cm.expected_f64
  D. far      K/V heads and pages whose byte offsets lie past 2^32 and 2^33

A Problem is the host side of one packed call: padded encodings, raw lengths, the token layout.
"""
import functools

import numpy as np

import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import decode_varlen_inputs as dv
import fallback_inputs as fi
import softmax_range_inputs as sr

D, TILE, ROWS, WS_ROW = 256, 64, 32, 260     # kv256::kD, kTile, kRows, kWsRow
SCALE = 1.0 / 16.0                           # 1 / sqrt(D)
LOG2E, LN2 = fi.LOG2E, fi.LN2


def _ceil(a, b):
    return -(-a // b)


# ---- the host's arithmetic, restated ---------------------------------------------------------------------------------------------------
def window_span_cap(nq, cap, W):
    """fa_fwd_kvwindow.hip: the longest key range a sequence can stream under a window of W >= 1 keys"""
    need = W + nq - 1
    return cap if need >= cap else min(_ceil(need, TILE) * TILE + TILE, cap)


def split_count(B, Hkv, G, max_q, cap, W=0):
    """kv256_split_count for num_splits = 0: 1024 workgroups wanted, at least four tiles per split, no empty split of a full
    sequence"""
    base = B * Hkv * _ceil(G * max_q, ROWS)
    tiles = _ceil(cap if W == 0 else window_span_cap(max_q, cap, W), TILE)
    s = max(1, min(_ceil(1024, base), tiles // 4))
    return _ceil(tiles, _ceil(tiles, s))


def workspace_bytes(B, Hkv, G, max_q, S):
    """S > 1: nqb * 32 rows of 260 floats per (sequence, K/V head, split)"""
    return 0 if S <= 1 else B * Hkv * S * _ceil(G * max_q, ROWS) * ROWS * WS_ROW * 4


def start_of(L, n, W):
    """(start_b, start_t): row 0's lower limit and the first key of the tile it lies in"""
    sb = max(L - n + 1 - W, 0) if W else 0
    return sb, sb & ~(TILE - 1)


def chunk_of(L, n, W, S):
    return _ceil(_ceil(L - start_of(L, n, W)[1], TILE), S) * TILE


# ---- one packed problem ----------------------------------------------------------------------------------------------------------------
class Problem:
    """qb [B*Hkv*G, max_q, D], kb, vb [B*Hkv, Ncap, D] uint16 encodings (vals: their fp32 values), raw lengths, the tokens each sequence
    owns -> the layout of decode_varlen_inputs (dv.LEAD tokens of no sequence in front, dv.TRAIL behind)"""

    def __init__(self, vals, bits, lens, spans, Hkv, G, max_q, Ncap, fmt):
        self.q, self.k, self.v = vals
        self.qb, self.kb, self.vb = bits
        self.lens, self.spans = tuple(int(x) for x in lens), tuple(spans)
        self.B, self.Hkv, self.G, self.max_q, self.Ncap, self.fmt = len(self.lens), Hkv, G, max_q, Ncap, fmt
        self.Hq = Hkv * G
        cu = np.cumsum((dv.LEAD,) + self.spans)
        self.lay = dv.Layout(cu, int(cu[-1]) + dv.TRAIL, max_q)
        assert self.lay.n == [min(s, max_q) for s in self.spans]
        assert self.qb.shape == (self.B * self.Hq, max_q, D) and self.kb.shape == self.vb.shape == (self.B * Hkv, Ncap, D)

    def seen(self):
        """the lengths the poison takes: a sequence without a row reads nothing"""
        return [L if n else 0 for L, n in zip(self.lens, self.lay.n)]

    def packed_q(self):
        return dv.pack_rows(self.lay, self.qb, np.uint16(cm.NAN16))

    def caches(self, W=0):
        """K and V [B, Hkv, Ncap, D] with NaN past each length and below each sequence's own window start"""
        seen = self.seen()
        return [np.concatenate([cm.poisoned(x.reshape(self.B, self.Hkv, self.Ncap, D)[b:b + 1], seen[b:b + 1], max(self.lay.n[b], 1), W)
                                for b in range(self.B)]) for x in (self.kb, self.vb)]

    def pools(self, ps, W=0, seed=7):
        """cm.scatter of caches(): NaN pages no table names, garbage in the dead entries"""
        kc, vc = self.caches(W)
        return cm.scatter(kc, vc, self.seen(), ps, seed + ps, self.max_q, W)

    def limits(self, causal, W=0):
        """lo, c [B*Hq, max_q] from cm.row_limits with each sequence's OWN n_b (dead rows: 0, 0)"""
        lo, c = (np.zeros((self.B * self.Hq, self.max_q), np.int64) for _ in range(2))
        for b in range(self.B):
            hs = slice(b * self.Hq, (b + 1) * self.Hq)
            lo[hs], c[hs], _ = cm.row_limits(cm.clamp(self.lens[b], self.Ncap), self.lay.n[b], self.max_q, causal, W)
        return lo, c

    def reference(self, causal, W=0, scale=None, softcap=0.0):
        """the padded float64 pair of cm.expected_f64, read-only"""
        out, lse = cm.expected_f64(self.q, self.k, self.v, self.lens, self.B, self.Hkv, self.G, self.max_q, causal, W, scale=scale,
                                   softcap=softcap, nq=self.lay.n)
        out.setflags(write=False), lse.setflags(write=False)
        return out, lse

    def split_count(self, W=0):
        return split_count(self.B, self.Hkv, self.G, self.max_q, self.Ncap, W)


@functools.lru_cache(maxsize=None)
def random_problem(oracle, lens, spans, Hkv, G, max_q, Ncap, fmt, seed):
    vals, bits = di.inputs(oracle, len(lens), Hkv, G, max_q, Ncap, D, fmt, seed)
    return Problem(vals, bits, lens, spans, Hkv, G, max_q, Ncap, fmt)


# ---- A. the key census -----------------------------------------------------------------------------------------------------------------
# 40 rows per (sequence, K/V head) where n_b = 8: two blocks, the second with 8 live rows.  Spans 0, 1, 3, 5, 8 and one above max_q.
CENSUS = dict(Hkv=2, G=5, max_q=8, Ncap=1024, lens=(0, 1, 3, 64, 65, 300, 513, 777, 1024, 1500), spans=(3, 8, 8, 1, 8, 0, 11, 8, 5, 8))
CENSUS_S = (1, 3, 5, 7, 16, 0)
CENSUS_W = (0, 3, 70, 300)
CENSUS_PAGES = (0, 16, 128, 256, 1024)
CENSUS_SOFTCAP = 30.0


def census_launches():
    """[(S, W, page size, causal)]: the contiguous launch of every (S, W) and one paged launch beside it, the page size walking with
    S + W so that every pair of (S, page size) and (W, page size) occurs too"""
    out = []
    for iS, S in enumerate(CENSUS_S):
        for iW, W in enumerate(CENSUS_W):
            causal = (iS + (iW >> 1)) & 1
            out += [(S, W, 0, causal), (S, W, CENSUS_PAGES[1 + (iS + iW) % 4], causal)]
    return out


@functools.lru_cache(maxsize=None)
def census_problem(oracle, fmt, coding):
    """ci.z_decode at d = 256 -> (Problem, m per K/V head)"""
    f = CENSUS
    z = ci.z_decode(oracle, len(f["lens"]), f["Hkv"], f["G"], f["max_q"], f["Ncap"], D, fmt, coding)
    return Problem((z["q"], z["k"], z["v"]), z["bits"], f["lens"], f["spans"], f["Hkv"], f["G"], f["max_q"], f["Ncap"], fmt), z["m"]


def census_expected(p, m, coding, causal, W):
    """-> (S [B*Hq, max_q, D] closed-form sums, cnt [B*Hq, max_q], m per query head)"""
    lo, c = p.limits(causal, W)
    S, m_q = ci.decode_sums(m, lo, c, p.G, p.Ncap, D, coding)
    return S, c - lo, m_q


def census_lse(cnt):
    with np.errstate(divide="ignore"):
        return np.log(cnt.astype(np.float64))


# ---- B. the softmax range --------------------------------------------------------------------------------------------------------------
RANGE = dict(B=3, Hkv=1, G=10, max_q=4, Ncap=1024, lens=(933, 66, 130), spans=(4, 2, 4), seed=9700)
RANGE_SPLITS = (1, 2, 3, 5, 16, 0)
RANGE_PAGES = (16, 256)
RANGE_VARIANTS = ("plain", "softcap", "window")
RANGE_STAIR_TILES = 7
# sequence 0 (933 keys = 14 tiles of 64 and 37 keys; 40 rows p = head * 4 + token: heads 0..7 are block 0, heads 8 and 9 block 1):
# (kind, token, head, [(key, lift)]).  Heads 4..7 (block 0) and the rest of heads 8 and 9 (block 1) are benign.
RANGE_KINDS = (
    ("staircase", 0, 1, [(64 * t + 5 + t, fi.STAIR_STEP * t) for t in range(RANGE_STAIR_TILES)]),
    ("jump 40 in the last split", 1, 2, [(900, 40.0)]),
    ("jump 150 in the last split", 2, 8, [(910, 150.0)]),
    ("all but tile 0 below -200", 3, 9, [(20, 210.0)]),
    ("jump 40 on the last key", 3, 0, [(932, 40.0)]),
    ("masked 150 on the last key", 0, 3, [(932, 150.0)]),
)
# sequence 1 (66 keys, two tokens): key 65 is seen by the last token alone under the mask
RANGE_SEQ1 = (("jump 40 on key 65", 1, 0, [(65, 40.0)]), ("jump 150 on key 64", 1, 1, [(64, 150.0)]))
RANGE_SHIFTED = ((0, -fi.KV_SHIFT), (1, fi.KV_SHIFT))   # sequence 2: (head, level of every logit)
# W = 100 on sequence 0: token i sees [830 + i, 930 + i) under the mask and [830 + i, 933) without; start_b = 830, start_t = 768:
# three tiles (768, 832, 896)
RANGE_WINDOW_KINDS = (
    ("masked 150 just below the window", 1, 0, [(830, 150.0)]),
    ("jump 40 on the window's first key", 2, 1, [(832, 40.0)]),
    ("jump 40 on the diagonal", 1, 8, [(930, 40.0)]),
    ("staircase", 0, 9, [(831, 0.0), (870, fi.STAIR_STEP), (905, 2 * fi.STAIR_STEP)]),
)


def range_kinds(variant, b=0):
    if b == 1:
        return RANGE_SEQ1
    return () if b else (RANGE_WINDOW_KINDS if variant == "window" else RANGE_KINDS)


def range_options(variant):
    """(W, softcap) of a variant"""
    return (sr.WINDOW if variant == "window" else 0), (sr.SOFTCAP if variant == "softcap" else 0.0)


def range_scores(q, k, b, i, h, L):
    """[L] float64 log2 scores of (token i, head h) of sequence b (Hkv = 1: the K head of sequence b is b)"""
    return (k[b, :L].astype(np.float64) @ q[b * RANGE["G"] + h, i].astype(np.float64)) * (SCALE * LOG2E)


@functools.lru_cache(maxsize=None)
def range_case(oracle, fmt, variant="plain"):
    """-> (Problem, spikes [(b, kind, token, head, key, lift built, lift measured on the rounded values)]).  The query rows of
    sequences 0 and 1 are made orthogonal (40 <= 256); a hostile key is the sum of the multiples of its rows that brings each to its
    target.  Sequence 2 carries the offsets of fi.kvcache_case.  plain and softcap share their values."""
    f = RANGE
    B, Hq, Nq, Ncap = f["B"], f["G"], f["max_q"], f["Ncap"]
    (q, _, _), _ = oracle.make_qkv(B * Hq, Nq, D, fmt=fmt, seed=f["seed"] + fmt)
    (_, k, v), _ = oracle.make_qkv(B, Ncap, D, fmt=fmt, seed=f["seed"] + 100 + fmt)
    q, k = q.copy(), k.copy()
    for b in (0, 1):
        n = f["spans"][b]
        q[b * Hq:(b + 1) * Hq, :n] = fi._orthogonal_rows(q[b * Hq:(b + 1) * Hq, :n].reshape(Hq * n, D)).reshape(Hq, n, D)
    u = np.ones(D, np.float32) / np.sqrt(D)
    off = np.sqrt(fi.KV_SHIFT / (SCALE * LOG2E * D))       # per component: D * off^2 * SCALE * log2 e = KV_SHIFT
    k[2] -= np.outer(k[2] @ u, u)
    k[2] += off
    for h, level in RANGE_SHIFTED:
        q[2 * Hq + h] -= np.outer(q[2 * Hq + h] @ u, u)
        q[2 * Hq + h] += np.sign(level) * off
    q = sr._round16(q, fmt)
    k = sr._round16(k, fmt).copy()
    plan = [(b, kind) for b in (0, 1) for kind in range_kinds(variant, b)]
    for b in (0, 1):
        L, rebuilt = f["lens"][b], {}
        for bb, (kind, i, h, keys) in plan:
            if bb != b:
                continue
            s = range_scores(q, k, b, i, h, L)
            base = np.delete(s, [key for key, _ in keys]).max()
            qr = q[b * Hq + h, i].astype(np.float64)
            for key, lift in keys:
                rebuilt[key] = rebuilt.get(key, 0.0) + qr * ((base + lift) / (SCALE * LOG2E) / float(qr @ qr))
        for key, row in rebuilt.items():
            k[b, key] = row
    k = sr._round16(k, fmt)
    spikes = []
    for b, (kind, i, h, keys) in plan:
        s = range_scores(q, k, b, i, h, f["lens"][b])
        base = np.delete(s, [key for key, _ in keys]).max()
        spikes += [(b, kind, i, h, key, lift, float(s[key] - base)) for key, lift in keys]
    vals = (q, k, v)
    bits = tuple(oracle.encode16(x, fmt) for x in vals)
    sr._frozen(q, k, *bits)
    return Problem(vals, bits, f["lens"], f["spans"], 1, Hq, Nq, Ncap, fmt), spikes


def range_hostile(variant, b):
    """{(token, head): [keys]} of sequence b"""
    return {(i, h): [key for key, _ in keys] for _, i, h, keys in range_kinds(variant, b)}


@functools.lru_cache(maxsize=None)
def range_reference(oracle, fmt, variant, causal):
    p, _ = range_case(oracle, fmt, variant)
    W, softcap = range_options(variant)
    return p.reference(causal, W, SCALE, softcap)


def range_vmax(p):
    return float(np.abs(p.v).max())


# ---- the model of this kernel ----------------------------------------------------------------------------------------------------------
def model(p, causal, W=0, softcap=0.0, S=1, defect=None, events=None, out16=False, scale=SCALE):
    """The scheme on a Problem -> what the kernel would leave in sentinel-filled packed fp32 O [total_q, Hq, D] and lse
    [Hq, total_q] (out16: O rounded to the format once more).  64-key tiles from start_t, S splits of chunk keys, blocks of 32 rows
    p = hd * n_b + i that vote together, the cap before the masks, sr.finish for one split and sr.merge behind more.  S = 0: the
    host's choice.  events receives {(b, hkv, token, head of the group): [rise array of every split]}"""
    S = S or p.split_count(W)
    o = np.zeros((p.B * p.Hq, p.max_q, D), np.float32)
    lse = np.full((p.B * p.Hq, p.max_q), -np.inf, np.float32)
    for b in range(p.B):
        n, L = p.lay.n[b], cm.clamp(p.lens[b], p.Ncap)
        if n == 0:
            continue
        R = n * p.G
        rows = [divmod(x, n) for x in range(R)]                 # (head of the group, token)
        lo, c, _ = cm.row_limits(L, n, p.max_q, causal, W)
        key = np.arange(L)[None, :]
        vis = (key >= np.array([lo[i] for _, i in rows])[:, None]) & (key < np.array([c[i] for _, i in rows])[:, None])
        waves = [list(range(a, min(a + ROWS, R))) for a in range(0, R, ROWS)]
        start_t, chunk = start_of(L, n, W)[1], chunk_of(L, n, W, S)
        for hkv in range(p.Hkv):
            kk, vv = p.k[b * p.Hkv + hkv, :L].astype(np.float64), p.v[b * p.Hkv + hkv, :L]
            qq = np.stack([p.q[b * p.Hq + hkv * p.G + hd, i] for hd, i in rows]).astype(np.float64)
            s = (qq @ kk.T) * (scale * LOG2E)
            if softcap:
                cap2 = softcap * LOG2E
                s = cap2 * np.tanh(s / cap2)
            parts = [sr.lazy_pass(s, vis, vv, min(start_t + sp * chunk, L), min(L, start_t + sp * chunk + chunk), TILE, p.fmt, waves,
                                  defect) for sp in range(S)]
            ob, lb = sr.finish(parts[0], defect) if S == 1 else sr.merge(parts, defect)
            for x, (hd, i) in enumerate(rows):
                o[b * p.Hq + hkv * p.G + hd, i], lse[b * p.Hq + hkv * p.G + hd, i] = ob[x], lb[x]
                if events is not None:
                    events[b, hkv, i, hd] = [part["rise"][x] for part in parts]
    if out16:
        o = sr._round16(o, p.fmt)
    po = dv.pack_rows(p.lay, o, 0.0)
    po[~p.lay.owned] = np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0]
    return po, dv.pack_lse(p.lay, lse, np.float32(dv.SENTINEL_LSE))


def range_launches():
    """[(variant, causal, S, 16-bit output)]: every launch of the GPU tier's range tests (both formats run all of them)"""
    return [(variant, causal, S, out16) for variant in RANGE_VARIANTS for causal in (True, False) for S in RANGE_SPLITS
            for out16 in (False, True)]


def range_check(oracle, p, got_o, got_lse, want, want_lse, case, out16=False):
    """sr.check_packed on a packed fp32 pair (a 16-bit result widened, the sentinel put back in the tokens of no sequence)"""
    return sr.check_packed(oracle, p.lay, got_o, got_lse, want, want_lse, p.fmt, range_vmax(p), "fa_kvcache_decode_d256", case, out16)


# ---- C. lengths, rows, scale, the library's split count --------------------------------------------------------------------------------
SWEEP = dict(Hkv=di.C_SHAPE["Hkv"], G=di.C_SHAPE["G"], max_q=di.C_SHAPE["Nq"], Ncap=di.C_SHAPE["Ncap"], seed=9800)
SWEEP_W = (0, 100)
SWEEP_S = (di.C_SPLITS, 0)


def sweep_spans():
    """the tokens each of the 48 sequences owns: 0 .. max_q + 2 in turn"""
    return tuple(b % (SWEEP["max_q"] + 3) for b in range(di.C_SHAPE["B"]))


def sweep_problem(oracle, fmt):
    f = SWEEP
    return random_problem(oracle, di.c_lens(), sweep_spans(), f["Hkv"], f["G"], f["max_q"], f["Ncap"], fmt, f["seed"])


# (G, max_q): 128 rows in four full blocks; 35 rows, three of them live in the last block; three rows
ROW_CASES = ((16, 8), (7, 5), (3, 1))
ROW_NCAP = 1000                                  # no multiple of 64: contiguous only
ROW_LENS = (1, 2, 3, 65, 999, 1000, 1001)        # 1, 2, 3 < n_b = 5: rows below their first key beside rows with keys


def rows_problem(oracle, fmt, G, max_q):
    spans = tuple(max_q + (b % 3 == 2) for b in range(len(ROW_LENS)))   # every sequence at max_q rows, some own a token more
    return random_problem(oracle, ROW_LENS, spans, 1, G, max_q, ROW_NCAP, fmt, 9810 + G)


SCALE_SPANS = (3, 3, 5, 3, 3, 4, 3, 3)           # n_b = max_q everywhere, so cm.uniform_expected applies as it is
SCALE_SOFTCAP, SCALE_W = 30.0, 70


def scale_problem(oracle, fmt):
    f = di.D_SHAPE
    return random_problem(oracle, di.D_LENS, SCALE_SPANS, f["Hkv"], f["G"], f["Nq"], f["Ncap"], fmt, 9820)


# num_splits = 0: (B, lengths, W, the split count the rule gives); Hkv = 1 and G * max_q = 32 rows, one block
AUTO = dict(Hkv=1, G=4, max_q=8, Ncap=1024)
AUTO_CASES = ((1, (1000,), 0, 4), (8, (1000, 1024, 513, 64, 5, 0, 300, 777), 0, 4), (8, (1000, 1024, 513, 64, 5, 0, 300, 777), 70, 1))


def auto_problem(oracle, fmt, lens):
    f = AUTO
    spans = tuple((8, 3, 9, 1, 8, 2, 8, 5)[b] for b in range(len(lens)))
    return random_problem(oracle, tuple(lens), spans, f["Hkv"], f["G"], f["max_q"], f["Ncap"], fmt, 9830 + len(lens))


# ---- D. base offsets past 2^32 bytes ---------------------------------------------------------------------------------------------------
# contiguous: a head is Ncap * 512 bytes = 2 MiB, so heads 2048 and 4096 start at 2^32 and 2^33 bytes
FAR_CONTIG = dict(B=4104, Hkv=1, G=1, max_q=1, Ncap=4096)
FAR_CONTIG_LIVE = ((0, 4096), (2049, 100), (4097, 77), (4103, 4096))       # (sequence, length); every other length is 0
# paged: a (page, K/V head) unit is 256 * 512 bytes = 128 KiB and a page holds two, so pages 16384 and 32768 start at 2^32 and 2^33
FAR_PAGED = dict(B=2, Hkv=2, G=1, max_q=1, ps=256, max_pages=8, num_pages=32800, S=4)
FAR_PAGED_LENS = (2048, 3 * 256 + 77)
FAR_PAGED_TABLE = ((5, 16390, 32776, 32799, 6, 16391, 32777, 32798), (32797, 16392, 4, 32778))   # live entries


def far_units(pages, Hkv):
    """the (page, K/V head) units page * Hkv + hkv of a list of pages"""
    return [page * Hkv + h for page in pages for h in range(Hkv)]
