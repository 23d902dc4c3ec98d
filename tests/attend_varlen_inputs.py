"""Families, classes and the expected result of the mixed prefill + decode step (tests/test_gpu_kvcache_attend_varlen.py,
tests/test_attend_varlen_inputs.py): fa_kvcache_attend_varlen.  Pure numpy; nothing here touches a GPU.

The contract, from include/fa_mi355.h.  [s_b, e_b) are the clamps of cu_seqlens_q into [0, total_q] and span_b = e_b - s_b.  With the
threshold T: span_b = 0 is an idle slot, 1 <= span_b <= T is SHORT (the split-KV half, parts & 1), span_b > T is LONG (the tiled half,
parts & 2).  Every token of every sequence is a live row -- nothing is cut at T -- and row i sees the keys [lo_i, c_i) with
c_i = max(0, L_b - span_b + 1 + i) and lo_i = max(0, L_b - span_b + 1 + i - W) under a window.  A part that is not asked for leaves
the rows of its class alone, and tokens of no sequence are never written.

The expected result is composed from the reference the packed-decode and the varlen-cache tiers share: cm.expected_f64, one call per
sequence with Nq = n = span_b, scattered to the packed layout.  `model` is the routing rule over that reference, with the WRONG rules
the CPU tier holds it against.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_varlen_inputs as dv
import fp8_inputs as f8
import logit_inputs as li
import varlen_inputs as vi
import window_inputs as wi

T = 4                      # the threshold of every family but "default"
HKV, G, PAGE = 2, 2, 16
SHORT, LONG = 1, 2         # FA_ATTEND_SHORT, FA_ATTEND_LONG
WINDOW, SOFTCAP = 48, 30.0   # the options "on together": this window, this soft-cap, sinks with one -inf head
KS, VS = (0.5, 1.25), (2.0, 0.37)   # per-head fp8 scales

# spans: what cu_seqlens_q gives each sequence (three lead and two trail tokens that no sequence owns); lens: the keys in the cache,
# the step's own tokens included.  cu / total_q in the place of spans: the raw vector as it is.
FAMILIES = {
    # span 4 = T is the last SHORT span, 5 = T + 1 the first LONG one, 140 crosses the tiled kernel's 128-row block, 0 is an idle slot
    "mixed": dict(spans=(1, 4, 5, 0, 140), lens=(200, 77, 150, 33, 190), Ncap=256, seed=9100),
    "all_short": dict(spans=(1, 3, 4, 2), lens=(200, 3, 77, 256), Ncap=256, seed=9200),
    "all_long": dict(spans=(5, 9, 130), lens=(100, 9, 256), Ncap=256, seed=9300),
    # raw differences (82, -96, 5, 2, 4) against clamped spans (3, 0, 5, 2, 4): sequence 0 is LONG by its raw difference and SHORT by
    # its span; cu[1] lies beyond total_q; cu[2] decreases
    "clamped": dict(cu=(17, 99, 3, 8, 10, 14), total_q=20, lens=(120, 50, 64, 2, 201), Ncap=256, seed=9400),
    # a LONG sequence with L < span: its first 9 - 5 = 4 rows see no key; a SHORT one with L < span beside it
    "nokey": dict(spans=(3, 9, 1), lens=(2, 5, 100), Ncap=256, seed=9500),
    # total_q = 4 <= T: the LONG half is not launched (one lead and one trail token: five would put total_q above T)
    "tiny": dict(spans=(1, 1), lens=(37, 200), Ncap=256, lead=1, trail=1, seed=9600),
    # "mixed" on a capacity whose split count is above 1 (the bit tests run once with the merge in the SHORT half)
    "split": dict(spans=(1, 4, 5, 0, 140), lens=(900, 77, 150, 33, 700), Ncap=1024, seed=9700),
    # the front end's default threshold of 128 rows on the real grid shapes: 128 is the last SHORT span, 129 the first LONG one
    "default": dict(spans=(1, 128, 129), lens=(300, 300, 300), Ncap=320, T=128, seed=9800),
}
NAMES = tuple(FAMILIES)


class Layout:
    """cu (raw), total_q, s [B], span [B] under the entry's clamps, cls [B] (0, SHORT or LONG)"""

    def __init__(self, cu, total_q, t=T, raw_class=False):
        self.cu, self.total_q = np.asarray(cu, np.int32), int(total_q)
        self.s = [min(max(int(x), 0), self.total_q) for x in self.cu[:-1]]
        e = [max(min(max(int(x), 0), self.total_q), s) for x, s in zip(self.cu[1:], self.s)]
        self.span = [y - x for x, y in zip(self.s, e)]
        by = [int(b) - int(a) for a, b in zip(self.cu[:-1], self.cu[1:])] if raw_class else self.span
        self.cls = [0 if n == 0 else (SHORT if c <= t else LONG) for n, c in zip(self.span, by)]

    def rows(self, parts):
        """[total_q] bool: the tokens a call with `parts` writes"""
        own = np.zeros(self.total_q, bool)
        for s, n, c in zip(self.s, self.span, self.cls):
            if c & parts:
                own[s:s + n] = True
        return own


def threshold(name):
    return FAMILIES[name].get("T", T)


@functools.lru_cache(maxsize=None)
def layout(name):
    f = FAMILIES[name]
    if "cu" in f:
        return Layout(f["cu"], f["total_q"])
    cu = np.cumsum([f.get("lead", 3)] + list(f["spans"]))
    lay = Layout(cu, int(cu[-1]) + f.get("trail", 2), threshold(name))
    assert lay.span == list(f["spans"])
    return lay


def shape(name):
    """(B, Hkv, G, Ncap)"""
    f = FAMILIES[name]
    return len(f["lens"]), HKV, G, f["Ncap"]


def want_S(name, W=0):
    """the split count of the SHORT half: the packed decode entry's with max_q = T"""
    B, Hkv, g, Ncap = shape(name)
    t = threshold(name)
    return wi.split_count(B * Hkv, g * t, Ncap) if W == 0 else wi.splits(B * Hkv, g * t, t, Ncap, W)


@functools.lru_cache(maxsize=None)
def inputs(name, d, fmt):
    """-> (q (total_q, Hq, d), k, v [B*Hkv, Ncap, d]) fp32 values rounded to the 16-bit format, and their encodings; read-only"""
    B, Hkv, g, Ncap = shape(name)
    rng = np.random.default_rng(FAMILIES[name]["seed"] + d + fmt)
    bits = tuple(vi.encode16(rng.standard_normal(s).astype(np.float32), fmt)
                 for s in ((layout(name).total_q, Hkv * g, d), (B * Hkv, Ncap, d), (B * Hkv, Ncap, d)))
    vals = tuple(vi.decode16(b, fmt) for b in bits)
    for a in vals + bits:
        a.setflags(write=False)
    return vals, bits


def options(on, Hq):
    """-> (window, softcap, sinks [Hq] or None): all off, or the three on together with one head without a sink"""
    if not on:
        return 0, 0.0, None
    sinks = li.sinks_for(Hq).astype(np.float32)
    sinks[1] = -np.inf
    return WINDOW, SOFTCAP, sinks


def kv_values(name, d, fmt, fp8=False):
    """the K and V values the kernels see: the 16-bit ones, or their e4m3fn codes dequantised by the per-head scales"""
    (_, k, v), _ = inputs(name, d, fmt)
    if not fp8:
        return k, v
    B = shape(name)[0]
    return (f8.decode(f8.encode(k)) * np.tile(np.array(KS, np.float32), B)[:, None, None],
            f8.decode(f8.encode(v)) * np.tile(np.array(VS, np.float32), B)[:, None, None])


def sequence_f64(name, d, fmt, b, n, on, fp8=False, align=None):
    """the float64 reference of ONE sequence taken as the n rows from token s_b on -> (O [Hq, n, d], lse [Hq, n]).  align (a wrong
    rule's): row i ends at L - align + 1 + i, as in a sequence of `align` rows"""
    lay = layout(name)
    B, Hkv, g, Ncap = shape(name)
    (q, _, _), _ = inputs(name, d, fmt)
    k, v = kv_values(name, d, fmt, fp8)
    W, softcap, sinks = options(on, Hkv * g)
    s = lay.s[b]
    qs = np.ascontiguousarray(q[s:s + n].transpose(1, 0, 2))
    L = FAMILIES[name]["lens"][b]
    if align is not None and align != n:   # the limits of n rows on L - align + n keys are L - align + 1 + i
        L = cm.clamp(L, Ncap) - align + n
    return cm.expected_f64(qs, k[b * Hkv:(b + 1) * Hkv], v[b * Hkv:(b + 1) * Hkv], [L], 1, Hkv, g, n, True, W, softcap=softcap, sinks=sinks)


WRONG = ("short_takes_below_T_only", "long_takes_T", "short_cuts_long", "long_takes_all", "class_from_raw_cu", "long_aligned_to_T",
         "T_plus_1_dropped", "idle_slot_writes")


@functools.lru_cache(maxsize=None)
def model(name, d, fmt, parts=3, on=False, fp8=False, wrong=None):
    """What the call leaves in an fp32 O (total_q, Hq, d) and an lse (Hq, total_q) pre-filled with dv's sentinels: the routing rule as
    specified (wrong None) or with one WRONG rule in its place --
      short_takes_below_T_only  the SHORT half's threshold test is span < T            long_takes_T     the LONG half's is span >= T
      short_cuts_long           the SHORT half computes the first T rows of a LONG sequence, as the packed decode entry cuts them
      long_takes_all            the LONG half computes every sequence
      class_from_raw_cu         the class comes from cu[b+1] - cu[b] before the clamps
      long_aligned_to_T         a LONG sequence's causal alignment uses min(span, T) rows: row i ends at L - T + 1 + i
      T_plus_1_dropped          a sequence of T + 1 rows is taken by neither half
      idle_slot_writes          a sequence of no rows writes one row, at its s_b: its neighbour's first token
    -> (O float32 with the NaN sentinel where nothing was written, lse float32), read-only"""
    assert wrong in (None,) + WRONG and (wrong is None or threshold(name) == T)
    lay = Layout(layout(name).cu, layout(name).total_q, threshold(name), raw_class=wrong == "class_from_raw_cu")   # this call's own
    B, Hkv, g, Ncap = shape(name)
    Hq = Hkv * g
    o = np.full((lay.total_q, Hq, d), np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0], np.float32)
    lse = np.full((Hq, lay.total_q), np.float32(dv.SENTINEL_LSE), np.float32)

    def put(b, n, align=None):
        ob, lb = sequence_f64(name, d, fmt, b, n, on, fp8, align=align)
        o[lay.s[b]:lay.s[b] + n] = ob.transpose(1, 0, 2)
        lse[:, lay.s[b]:lay.s[b] + n] = lb

    for b, (n, c) in enumerate(zip(lay.span, lay.cls)):
        if n == 0:
            continue
        short = n < T if wrong == "short_takes_below_T_only" else c == SHORT
        long_ = n >= T if wrong == "long_takes_T" else (True if wrong == "long_takes_all" else c == LONG)
        if wrong == "T_plus_1_dropped" and n == T + 1:
            short = long_ = False
        if parts & SHORT:
            if short:
                put(b, n)
            elif wrong == "short_cuts_long":
                put(b, T)
        if parts & LONG and long_:
            put(b, n, align=min(n, T) if wrong == "long_aligned_to_T" else None)
    if wrong == "idle_slot_writes":
        for b, n in enumerate(lay.span):
            if n == 0 and lay.s[b] < lay.total_q:
                put(b, 1)
    o.setflags(write=False), lse.setflags(write=False)
    return o, lse


def problems(name, got_o, got_lse, want_o, want_lse, parts, fmt):
    """got (fp32 O (total_q, Hq, d) and lse (Hq, total_q) of a call into sentinel-filled buffers) against model()'s pair -> findings.
    Tokens the call must not write: every sentinel byte still there.  Tokens it writes: vi.problems, the varlen-cache tier's check at
    the project's bounds (which are the packed-decode tier's: cm.MAX_ABS, cm.REL_L2, 2 * cm.P_EPS), rows without a key exact."""
    own = layout(name).rows(parts)
    out = []
    got_o, got_lse = np.ascontiguousarray(got_o, np.float32), np.asarray(got_lse, np.float32)
    if (got_o[~own].view(np.uint32) != dv.SENTINEL_O32).any() or (got_lse[:, ~own] != np.float32(dv.SENTINEL_LSE)).any():
        bad = (got_o[~own].view(np.uint32) != dv.SENTINEL_O32).any(axis=(1, 2)) | (got_lse[:, ~own] != np.float32(dv.SENTINEL_LSE)).any(axis=0)
        out.append(f"token {int(np.flatnonzero(~own)[np.flatnonzero(bad)[0]])} must keep its sentinels and was written")
    if own.any():
        if (got_o[own].view(np.uint32) == dv.SENTINEL_O32).all(axis=(1, 2)).any():
            out.append(f"token {int(np.flatnonzero(own)[np.flatnonzero((got_o[own].view(np.uint32) == dv.SENTINEL_O32).all(axis=(1, 2)))[0]])} "
                       "was not written")
        else:
            out += vi.problems(got_o[own], got_lse[:, own], np.asarray(want_o[own], np.float64), np.asarray(want_lse[:, own], np.float64),
                               np.ones(int(own.sum()), bool), fmt)
    return out
