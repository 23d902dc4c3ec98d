"""Inputs, trees, the float64 reference and the numpy kernels of the tree step (tests/test_tree_inputs.py,
tests/test_gpu_kvcache_tree.py): fa_kvcache_decode_varlen_ex with a tree_mask and fa_kvcache_append_varlen_ex with positions.  Pure
numpy plus the `oracle` fixture; nothing here touches a GPU.

The rule, from include/fa_mi355.h: s_b, n_b, L_b as in fa_kvcache_decode_varlen, base_b = L_b - n_b (may be negative), token s_b + j
is the key at base_b + j.  m_i = (tree_mask[s_b + i] & low n_b bits) | 1 << i; row i sees key k iff 0 <= k < L_b, k >= lo_i and
(k < base_b or bit k - base_b of m_i); lo_i = max(0, base_b + popcount(m_i) - W) under a window W, else 0.

Families: ragged_inputs' "spec" and "split" under the names the tree tier uses, and "wide" (64 rows per head: two row blocks, all
four waves, bit 63), registered beside ragged_inputs' EXTRA family so that decode_varlen_inputs' layout, packing and check serve it.
The inputs are ragged_inputs' boosted-tail construction: the tail keys carry e^12 times the weight of the others, so a row's O and
lse are decided by which tail keys it sees.
"""
import functools

import numpy as np

import append_inputs as ai
import append_varlen_inputs as av
import common_inputs as cm
import decode_varlen_inputs as dv
import logit_inputs as li
import ragged_inputs as ri
import rope_inputs as rp

ri.EXTRA.setdefault("tree_wide", dict(B=2, Hkv=1, G=4, Nq=64, Ncap=256, lens=(200, 150), nq=(64, 33), seed=9300))
FAMILY = {"chain_and_fan": "spec", "wide": "tree_wide", "split": "split"}   # the tree tier's name -> decode_varlen_inputs' name
NAMES = tuple(FAMILY)
WINDOWS = (0, 100, 3)     # 3 is below the depth of the chains: the window cuts ancestors
TREES = ("chain", "star", "random")
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def family(name):
    return dv.family(FAMILY[name])


def layout(name):
    return dv.layout(FAMILY[name])


def inputs(oracle, name, d, fmt):
    return dv.inputs(oracle, FAMILY[name], d, fmt)


# ---- trees ------------------------------------------------------------------------------------------------------------------------------
def parents_of(kind, n, rng):
    """parent index of each of n tokens (-1: a root)"""
    if kind == "chain":
        return [i - 1 for i in range(n)]
    if kind == "star":
        return [-1] + [0] * (n - 1)
    return [-1] + [int(rng.integers(-1 if i % 7 == 0 else 0, i)) for i in range(1, n)]


def closed_masks(parents):
    """the ancestor-closed words (self bit included) and the depths, by walking every chain: python ints"""
    words, depth = [], []
    for i, p in enumerate(parents):
        w, dp = 1 << i, 0
        while p >= 0:
            w |= 1 << p
            dp += 1
            p = parents[p]
        words.append(w)
        depth.append(dp)
    return words, depth


@functools.lru_cache(maxsize=None)
def tree(name, kind):
    """-> (words uint64 [total_q] as the kernel gets them, parents int32 [total_q], depth int32 [total_q]).  Tokens of no sequence hold
    all-ones.  `random` is closed only in part: a few rows carry bits ABOVE their own index, a few lack their self bit, and every row
    of a sequence with n_b < 64 carries junk at and above bit n_b, which the entry must ignore."""
    lay = layout(name)
    rng = np.random.default_rng(9400 + len(name) + 17 * TREES.index(kind))
    words = np.full(lay.total_q, ALL, np.uint64)
    parents = np.full(lay.total_q, -1, np.int32)
    depth = np.zeros(lay.total_q, np.int32)
    for b, n in enumerate(lay.n):
        if n == 0:
            continue
        par = parents_of(kind, n, rng)
        w, dp = closed_masks(par)
        if kind == "random":
            for i in range(n):
                if i % 5 == 2 and i + 1 < n:
                    w[i] |= 1 << int(rng.integers(i + 1, n))       # a bit above the row's own: legal
                if i % 6 == 4:
                    w[i] &= ~(1 << i)                             # no self bit: the entry forces it
                if n < 64:
                    w[i] |= int(rng.integers(1, 1 << 20)) << n    # junk at and above n_b: ignored
        s = lay.s[b]
        words[s:s + n] = np.array([x & 0xFFFFFFFFFFFFFFFF for x in w], np.uint64)
        parents[s:s + n], depth[s:s + n] = par, dp
    for a in (words, parents, depth):
        a.setflags(write=False)
    return words, parents, depth


def triangle(lay):
    """the words that make the call the causal one: (1 << (i + 1)) - 1 on every live row, all-ones elsewhere"""
    words = np.full(lay.total_q, ALL, np.uint64)
    for b, n in enumerate(lay.n):
        for i in range(n):
            words[lay.s[b] + i] = np.uint64((1 << (i + 1)) - 1)
    return words


# ---- visibility -------------------------------------------------------------------------------------------------------------------------
WRONG = ("plain_causal", "everything_visible", "bit_off_by_one", "base_from_max_q", "word_at_i", "hd_i_swapped", "high32_dropped",
         "self_bit_not_forced", "bits_ge_n_honoured", "lo_from_i", "mask_on_prefix")


def visibility(lay, lens, Ncap, G, words, W, wrong=None):
    """-> one bool array [G, n_b, L_b] per sequence: which keys each row sees, from the rule in the module docstring (wrong: one of the
    WRONG kernels' rules in its place).  The head axis is there for hd_i_swapped alone."""
    out = []
    for b, n in enumerate(lay.n):
        L = cm.clamp(lens[b], Ncap)
        vis = np.zeros((G, n, L), bool)
        base = L - (lay.max_q if wrong == "base_from_max_q" else n)
        k = np.arange(L)
        for hd in range(G):
            for i in range(n):
                src = i
                if wrong == "hd_i_swapped":          # packed row r = hd * n + i read as (r % G, r // G)
                    src = (hd * n + i) // G
                tok = src if wrong == "word_at_i" else lay.s[b] + src
                w = int(words[tok])
                if wrong == "high32_dropped":
                    w &= 0xFFFFFFFF
                low = w if wrong == "bits_ge_n_honoured" else w & ((1 << n) - 1)
                m = low if wrong == "self_bit_not_forced" else low | (1 << i)
                if wrong == "plain_causal":
                    m = (1 << (i + 1)) - 1
                if wrong == "everything_visible":
                    m = (1 << n) - 1
                pop = i + 1 if wrong == "lo_from_i" else bin(m).count("1")
                lo = max(0, base + pop - W) if W else 0
                rel = k - base + (1 if wrong == "bit_off_by_one" else 0)
                if wrong == "mask_on_prefix":
                    bit = np.array([(m >> int(r % 64)) & 1 for r in rel], bool)
                    vis[hd, i] = (k >= lo) & bit
                else:
                    bit = np.array([r >= 0 and r < 64 and (m >> int(r)) & 1 for r in rel], bool)
                    vis[hd, i] = (k >= lo) & ((rel < 0) | bit)
        out.append(vis)
    return out


def brute_visibility(lay, lens, Ncap, words, W):
    """the same by one loop over (row, key), written from the header's sentence and nothing else -> [n_b, L_b] per sequence"""
    out = []
    for b, n in enumerate(lay.n):
        L = min(max(int(lens[b]), 0), Ncap)
        base = L - n
        vis = np.zeros((n, L), bool)
        for i in range(n):
            m = (int(words[lay.s[b] + i]) & ((1 << n) - 1)) | (1 << i)
            lo = max(0, base + bin(m).count("1") - W) if W else 0
            for key in range(L):
                if key < lo:
                    continue
                vis[i, key] = key < base or bool((m >> (key - base)) & 1)
        out.append(vis)
    return out


def expected_f64(q, k, v, vis, B, Hkv, G, Nq, softcap=0.0, sinks=None, scale=None):
    """cm.expected_f64 with an explicit visibility (one [G, n_b, L_b] per sequence) in the place of its limits: q [B*Hq, Nq, d],
    k/v [B*Hkv, Ncap, d] -> (O [B*Hq, Nq, d], lse [B*Hq, Nq]) float64; dead rows and rows with neither key nor sink: zeros and -inf"""
    Hq, d = Hkv * G, q.shape[2]
    out = np.zeros(q.shape, np.float64)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b in range(B):
        for h in range(Hq):
            r = b * Hq + h
            a = -np.inf if sinks is None else float(sinks[h])
            kk, vv = (x[b * Hkv + h // G].astype(np.float64) for x in (k, v))
            for i in range(vis[b].shape[1]):
                sel = vis[b][h % G, i]
                t = (kk[:sel.size][sel] @ q[r, i].astype(np.float64)) * sc
                if softcap:
                    t = softcap * np.tanh(t / softcap)
                m = max(t.max() if t.size else -np.inf, a)
                if m == -np.inf:
                    continue
                p = np.exp(t - m)
                den = p.sum() + np.exp(a - m)
                if t.size:
                    out[r, i] = (p / den) @ vv[:sel.size][sel]
                lse[r, i] = m + np.log(den)
    return out, lse


@functools.lru_cache(maxsize=None)
def reference(oracle, name, d, fmt, kind, W, variant="none", wrong=None):
    """the float64 result of a family under one of its trees (kind "triangle": the causal words), padded [B*Hq, max_q, ...], read-only"""
    f, lay = family(name), layout(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = inputs(oracle, name, d, fmt)
    words = triangle(lay) if kind == "triangle" else tree(name, kind)[0]
    sinks, softcap = li.options(variant, Hkv * G)
    out, lse = expected_f64(q, k, v, visibility(lay, f["lens"], Ncap, G, words, W, wrong), B, Hkv, G, Nq, softcap, sinks)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def numpy_kernel(oracle, name, d, fmt, kind, W, wrong=None):
    """what a kernel with the rule `wrong` (None: the entry) leaves in pre-filled fp32 O [total_q, Hq, d] and lse [Hq, total_q]"""
    lay = layout(name)
    Hq = family(name)["Hkv"] * family(name)["G"]
    o, lse = reference(oracle, name, d, fmt, kind, W, wrong=wrong)
    po = dv.pack_rows(lay, o.astype(np.float32), 0.0)
    po[~lay.owned] = np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0]
    live = dv.live_mask(lay, Hq)
    pl = dv.pack_lse(lay, np.where(live, lse, -np.inf).astype(np.float32), np.float32(dv.SENTINEL_LSE))
    return po, pl


# ---- the append with positions ----------------------------------------------------------------------------------------------------------
APPEND_WRONG = ("position_as_slot", "slot_as_position", "unclamped", "position_at_i")


def append_positions(x, kind="tree"):
    """int32 [total_new] for av.inputs(...): "tree": depths of a random tree behind each sequence's length, a few just past max_pos and a
    few negative (both clamp); "slot": L_b + i, the plain call's positions.  Rows of no sequence hold a huge value that must not be read."""
    cu, total, lens = x["cu"], x["total"], x["lens"]
    pos = np.full(total, 0x7FFFFFF0, np.int32)
    rng = np.random.default_rng(9500)
    for b, (s, e) in enumerate(av.bounds(cu, total)):
        n = e - s
        if n == 0:
            continue
        L = cm.clamp(lens[b], av.CASE["Ncap"])
        if kind == "slot":
            pos[s:e] = L + np.arange(n)
            continue
        _, dp = closed_masks(parents_of("random", n, rng))
        pos[s:e] = L + np.array(dp)
        pos[s + n // 2] = av.CASE["max_pos"] + 1 + b      # just past the table: row max_pos - 1
        if n > 2:
            pos[s + 1] = -3 - b                           # negative: row 0
    pos.setflags(write=False)
    return pos


def append_model(fmt, d, paged, fp8, rope, pos, wrong=None, qout0=None):
    """av.model with the table row of token t taken from pos[t] (clamped into [0, max_pos)) and the slot left alone -> the same dict.
    wrong: one of APPEND_WRONG in the place of that rule."""
    assert rope
    x = av.inputs(fmt, d, paged, fp8, rope)
    ncap, il, max_pos = av.CASE["Ncap"], rope == 2, av.CASE["max_pos"]
    cu, lens, total, cos, sin = x["cu"], x["lens"], x["total"], x["cos"], x["sin"]
    rows = av.token_rows(cu, total)
    m = [len(r) for r in rows]
    B, nnew = len(rows), max(1, max(m))
    start = [cm.clamp(L, ncap) for L in lens]
    trow = np.zeros((B, nnew), np.int64)
    for b, r in enumerate(rows):
        for i, t in enumerate(r):
            p = int(pos[i if wrong == "position_at_i" else t])
            if wrong == "slot_as_position":
                p = start[b] + i
            trow[b, i] = p % max_pos if wrong == "unclamped" else min(max(p, 0), max_pos - 1)
    kpad, vpad = av.gather(x["knb"], rows), av.gather(x["vnb"], rows)
    krot = rp.rotate_fp32(ai.widen16(kpad, fmt), cos[trow][:, None], sin[trow][:, None], il)
    rot_dim = 2 * cos.shape[1]

    def to16(bits, y):
        out = np.array(bits, np.uint16)
        out[..., :rot_dim] = ai.round16_bits(y[..., :rot_dim], fmt)
        return out
    krows = rp.fp8_codes(krot, x["ks"]) if fp8 else to16(kpad, krot)
    vrows = rp.fp8_codes(ai.widen16(vpad, fmt), x["vs"]) if fp8 else vpad
    place_lens = lens
    if wrong == "position_as_slot":   # the token lands where its position says (first token's position as the sequence's start)
        place_lens = tuple(int(min(max(int(pos[r[0]]), 0), ncap)) if r else lens[b] for b, r in enumerate(rows))
    out = dict(k=ri.place(x["kc0"], krows, place_lens, m, x["table"]), v=ri.place(x["vc0"], vrows, place_lens, m, x["table"]),
               lens=ri.lens_after(lens, m, B, kpad.shape[2], ncap))
    qsrc = x["qsrc"]
    qout = np.full(qsrc.shape, av.QOUT_NAN, np.uint16) if qout0 is None else np.array(qout0)
    qpad = av.gather(qsrc, rows)
    qrot = to16(qpad, rp.rotate_fp32(ai.widen16(qpad, fmt), cos[trow][:, None], sin[trow][:, None], il))
    for b, r in enumerate(rows):
        if r:
            qout[r] = qrot[b, :, :len(r)].transpose(1, 0, 2)
    out["qout"] = qout
    return out
