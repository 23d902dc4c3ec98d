"""Inputs, packing and the check of the token-packed decode entry (tests/test_gpu_kvcache_decode_varlen.py,
tests/test_decode_varlen_inputs.py): fa_kvcache_decode_varlen.  Pure numpy plus the `oracle` fixture; nothing here touches a GPU.

The contract, from include/fa_mi355.h: Q and O are packed (total_q, Hq, d), lse is [Hq, total_q]; [s_b, e_b) are the clamps of
cu_seqlens_q into [0, total_q], n_b = min(e_b - s_b, max_q), row i < n_b of sequence b is token s_b + i, and on those rows the call is
fa_kvcache_decode with Nq = max_q and seqlens_q[b] = n_b on the padded copy.  A token that is no live row of any sequence is never
read and never written.

Families: the three of tests/ragged_inputs.py and its EXTRA["tail"], with max_q = the family's padded Nq and n_b = its counts, so that
the float64 reference is cm.expected_f64 with nq= and the padded entry is the one the ragged tier tests; plus "overlong", whose first
and last sequences own more tokens than max_q.  The packing leaves 3 tokens before s_0 and 2 behind e_{B-1}.  One cu vector gives
e_b = s_{b+1} (where it does not decrease), so a hole BETWEEN two sequences exists only behind a sequence that is cut at max_q: the
first sequence with n_b = max_q owns 2 tokens more than it has rows (spec, tail), and overlong's sequences own up to 5 more.  blocks
and split have no sequence at max_q and so no such hole.  The inputs are ragged_inputs' with the boosted tail keys, which is what makes
a wrong n_b in a limit visible.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_inputs as di
import logit_inputs as li
import ragged_inputs as ri

LEAD, TRAIL, HOLE = 3, 2, 2
# spans: the tokens each sequence owns (e_b - s_b); n_b = min(span, Nq) = (4, 2, 0, 4)
OVERLONG = dict(B=4, Hkv=2, G=2, Nq=4, Ncap=256, lens=(200, 77, 150, 3), spans=(9, 2, 0, 6), seed=8800)
NAMES = list(ri.FAMILIES) + ["overlong"]
SENTINEL_O16, SENTINEL_O32, SENTINEL_LSE = 0x7E5A, 0x7FC5A5A5, -12345.5   # NaN bit patterns for O, a finite float for lse


def family(name):
    if name == "overlong":
        f = dict(OVERLONG)
        f["nq"] = tuple(min(s, f["Nq"]) for s in f["spans"])
        return f
    return ri.family(name)


def want_S(name, W):
    return ri.want_S(family(name), W)


class Layout:
    """One cu_seqlens_q vector over total_q tokens, cut at max_q, under the entry's clamps: cu (as given), total_q, max_q, s [B],
    n [B]; tok [B, max_q] (the token of row i, -1 for a dead row); owned [total_q] bool"""

    def __init__(self, cu, total_q, max_q):
        self.cu, self.total_q, self.max_q = np.asarray(cu, np.int32), int(total_q), int(max_q)
        B = len(self.cu) - 1
        self.s = [min(max(int(x), 0), self.total_q) for x in self.cu[:-1]]
        e = [max(min(max(int(x), 0), self.total_q), s) for x, s in zip(self.cu[1:], self.s)]
        self.n = [min(y - x, self.max_q) for x, y in zip(self.s, e)]
        self.tok = np.full((B, self.max_q), -1, np.int64)
        for b in range(B):
            self.tok[b, :self.n[b]] = self.s[b] + np.arange(self.n[b])
        self.owned = np.zeros(self.total_q, bool)
        self.owned[self.tok[self.tok >= 0]] = True
        assert self.owned.sum() == sum(self.n), "two sequences own one token"


@functools.lru_cache(maxsize=None)
def layout(name):
    f = family(name)
    B, Nq = f["B"], f["Nq"]
    n = cm.counts(f["nq"], B, Nq)
    spans = list(f["spans"]) if "spans" in f else list(n)
    if "spans" not in f and Nq in n:
        spans[n.index(Nq)] += HOLE
    cu = np.cumsum([LEAD] + spans)
    lay = Layout(cu, int(cu[-1]) + TRAIL, Nq)
    assert lay.n == n and not lay.owned[:LEAD].any() and not lay.owned[-TRAIL:].any()
    return lay


@functools.lru_cache(maxsize=None)
def inputs(oracle, name, d, fmt):
    """ri.inputs for its families; the same construction (boosted tail keys) for overlong"""
    if name != "overlong":
        return ri.inputs(oracle, name, d, fmt)
    f = family(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, f["seed"])
    q, k = q.copy(), k.copy()
    for b in range(B):
        L = cm.clamp(f["lens"][b], Ncap)
        q[b * Hkv * G:(b + 1) * Hkv * G, :, 0] = ri.BOOST
        k[b * Hkv:(b + 1) * Hkv, max(0, L - Nq):L, 0] = np.sqrt(d)
    bits = tuple(oracle.encode16(x, fmt) for x in (q, k, v))
    vals = tuple(oracle.decode16(x, fmt) for x in bits)
    for a in vals + bits:
        a.setflags(write=False)
    return vals, bits


@functools.lru_cache(maxsize=None)
def reference(oracle, name, d, fmt, W, causal, variant="none", ragged=True):
    """cm.expected_f64 with nq= (padded [B*Hq, max_q, ...]), computed once and read-only"""
    f = family(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = inputs(oracle, name, d, fmt)
    sinks, softcap = li.options(variant, Hkv * G)
    out, lse = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, causal, W, softcap=softcap, sinks=sinks, nq=f["nq"] if ragged else None)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


# ---- padded <-> packed -----------------------------------------------------------------------------------------------------------------
def pack_rows(lay, padded, fill):
    """padded [B*Hq, max_q, ...] -> packed [total_q, Hq, ...]: the live rows at their tokens, `fill` everywhere else"""
    B = len(lay.n)
    Hq = padded.shape[0] // B
    out = np.full((lay.total_q, Hq) + padded.shape[2:], fill, padded.dtype)
    for b in range(B):
        for i in range(lay.n[b]):
            out[lay.tok[b, i]] = padded[b * Hq:(b + 1) * Hq, i]
    return out


def pack_lse(lay, padded, fill):
    """padded [B*Hq, max_q] -> [Hq, total_q]"""
    return np.ascontiguousarray(pack_rows(lay, padded, fill).T)


def unpack_rows(lay, packed, B, fill=0):
    """packed [total_q, Hq, ...] -> padded [B*Hq, max_q, ...] with `fill` in the dead rows"""
    Hq = packed.shape[1]
    out = np.full((B * Hq, lay.max_q) + packed.shape[2:], fill, packed.dtype)
    for b in range(B):
        for i in range(lay.n[b]):
            out[b * Hq:(b + 1) * Hq, i] = packed[lay.tok[b, i]]
    return out


def live_mask(lay, Hq):
    """[B*Hq, max_q] bool"""
    return np.repeat(lay.tok >= 0, Hq, axis=0)


# ---- the check the GPU tier applies ----------------------------------------------------------------------------------------------------
def check(oracle, lay, got_o, got_lse, want, want_lse, fmt, what, sentinel=True):
    """got_o [total_q, Hq, d] float32 and got_lse [Hq, total_q] float32 of a call whose O (fp32) and lse were pre-filled with the
    sentinels, against the PADDED float64 reference: the project's bounds on the live rows (MAX_ABS, REL_L2, 2 * P_EPS on lse), rows
    without a key exactly 0 / -inf, and every token that is no live row still the sentinel, bit for bit.  Every figure is printed
    before it is judged."""
    B = len(lay.n)
    Hq = got_o.shape[1]
    assert got_o.shape == (lay.total_q, Hq, want.shape[2]) and got_lse.shape == (Hq, lay.total_q), what + ": shapes"
    if sentinel:
        free = ~lay.owned
        assert (np.ascontiguousarray(got_o[free]).view(np.uint32) == SENTINEL_O32).all(), what + ": an O row of no sequence was written"
        assert (got_lse[:, free] == np.float32(SENTINEL_LSE)).all(), what + ": an lse entry of no sequence was written"
    live = live_mask(lay, Hq)
    o = unpack_rows(lay, got_o, B)
    lse = unpack_rows(lay, np.ascontiguousarray(got_lse.T), B, fill=-np.inf)
    w = np.asarray(want, np.float32)
    ma, rl = oracle.max_abs(o, w), oracle.rel_l2(o, w)
    fin = np.isfinite(want_lse)
    assert not (fin & ~live).any()
    le = float(np.abs(lse[fin] - want_lse[fin]).max()) if fin.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert np.isfinite(o).all(), what + ": O is not finite"
    assert not np.isnan(lse).any(), what + ": NaN in lse"
    nokey = live & ~fin
    assert (o[nokey] == 0.0).all() and (lse[nokey] == -np.inf).all(), what + ": a row without a key is not exactly 0 / -inf"
    assert ma <= cm.MAX_ABS and rl <= cm.REL_L2[fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert np.isfinite(lse[fin]).all() and le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"


# ---- numpy kernels: the right one and six wrong ones -----------------------------------------------------------------------------------
WRONG = ("ignores_s_b", "max_q_in_the_limit", "ignores_q_stride_h", "lse_token_major", "zeros_in_free_tokens", "sink_per_split")


def packed_q(oracle, name, d, fmt, seed=77):
    """the family's Q, packed, with OTHER random rows (boosted like the live ones) in the tokens of no sequence -> fp32 values"""
    lay = layout(name)
    (q, _, _), _ = inputs(oracle, name, d, fmt)
    Hq = q.shape[0] // len(lay.n)
    out = pack_rows(lay, q, 0.0)
    noise = np.random.default_rng(seed).uniform(-1, 1, out.shape).astype(np.float32)
    noise[..., 0] = ri.BOOST
    out[~lay.owned] = oracle.decode16(oracle.encode16(noise, fmt), fmt)[~lay.owned]
    return out


def numpy_kernel(oracle, name, d, fmt, W, causal, variant="none", wrong=None, S=1):
    """What a kernel would leave in pre-filled fp32 O [total_q, Hq, d] and lse [Hq, total_q]: float64 arithmetic rounded to fp32, with
    one of the WRONG rules in the place of the right one (None: the entry as specified)."""
    f, lay = family(name), layout(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    Hq = Hkv * G
    (_, k, v), _ = inputs(oracle, name, d, fmt)
    qp = packed_q(oracle, name, d, fmt)
    q = np.zeros((B * Hq, Nq, d), np.float32)
    for b in range(B):
        for i in range(lay.n[b]):
            t = (b * Nq + i) % lay.total_q if wrong == "ignores_s_b" else lay.tok[b, i]
            q[b * Hq:(b + 1) * Hq, i] = qp[t, 0][None] if wrong == "ignores_q_stride_h" else qp[t]
    sinks, softcap = li.options(variant, Hq)
    nq = None if wrong == "max_q_in_the_limit" else f["nq"]
    o, lse = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, causal, W, softcap=softcap, sinks=sinks, nq=nq)
    if wrong == "sink_per_split":   # every split joins the sink to its partial: S sinks in the merged sum
        assert sinks is not None and S > 1
        a = np.tile(np.asarray(sinks, np.float64), B)[:, None]
        with np.errstate(divide="ignore"):
            extra = np.log(np.exp(lse) + (S - 1) * np.exp(a))
        o = o * np.exp(lse - extra)[..., None]
        lse = extra
    live = live_mask(lay, Hq)
    o, lse = np.where(live[..., None], o, 0.0), np.where(live, lse, -np.inf)
    po = pack_rows(lay, o.astype(np.float32), 0.0)
    po[~lay.owned] = np.array([SENTINEL_O32], np.uint32).view(np.float32)[0]
    pl = pack_lse(lay, lse.astype(np.float32), np.float32(SENTINEL_LSE))
    if wrong == "zeros_in_free_tokens":
        po[~lay.owned], pl[:, ~lay.owned] = 0.0, -np.inf
    if wrong == "lse_token_major":
        pl = np.ascontiguousarray(pl.T).reshape(Hq, lay.total_q)
    return po, pl
