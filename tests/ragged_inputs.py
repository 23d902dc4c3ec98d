"""Inputs and references for the per-sequence counts of the KV-cache step (tests/test_gpu_kvcache_ragged.py, tests/test_ragged_inputs.py):
`seqlens_q` of fa_kvcache_decode and `seqlens_new` of fa_kvcache_append_ex.  Pure numpy plus the `oracle` fixture
(tests/conftest.py); nothing here touches a GPU.  The clamp of a count, a sequence's row limits and the decode reference with its
`nq` argument are tests/common_inputs.py's; here are the families, their boosted inputs, and the append restated in integer numpy.

The contract, from include/fa_mi355.h.  Decode: Nq is the padded row count, n_b = min(max(seqlens_q[b], 0), Nq); row i < n_b of every
head of sequence b is live and sees the keys [lo_i, c_i) with c_i = max(0, L_b - n_b + 1 + i) under the causal mask (L_b without) and
lo_i = max(0, L_b - n_b + 1 + i - W) under a window (0 without); a live row without a key has O = 0 and lse = -inf (the sink logit
with sinks); a dead row, i >= n_b, has O = 0 and lse = -inf exactly, sinks or not.  Append: Nnew is the padded token count,
m_b = min(max(seqlens_new[b], 0), Nnew); token t < m_b goes to p = L_b + t by the flat entries' placement, token t >= m_b nowhere,
and the length becomes min(L_b + m_b, Ncap).

Inputs.  A kernel that ignored seqlens_q would move every causal limit of a sequence with n_b < Nq down by Nq - n_b keys.  On random
inputs that is a handful of keys among hundreds or thousands and moves nothing measurable, so the LAST Nq keys of every sequence are
boosted: their K rows get k[0] = sqrt(d) and every Q row gets q[0] = BOOST, which lifts their logits by BOOST nats -- above the
log-sum-exp of all the other keys of the longest sequence here (about 9.6 at 8000 keys).  A row's output and lse are then decided by
HOW MANY of those tail keys it sees, which is exactly what n_b changes.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_inputs as di
import logit_inputs as li
import window_inputs as wi

BOOST = 12.0
WINDOWS = (0, 100)

# family: B, Hkv, G, Nq (padded), Ncap, lengths AFTER the append, n_b
FAMILIES = {
    # an idle slot (n = 0); a sequence with L < n, whose first rows see nothing under the mask (L = 5, n = 8: rows 0..2)
    "spec": dict(B=5, Hkv=2, G=4, Nq=8, Ncap=320, lens=(300, 129, 64, 7, 5), nq=(8, 3, 1, 0, 8), seed=8100),
    # G * Nq = 160 padded rows, two row blocks: 128 live rows (the second block dead); 132 live rows (four of them in block 2)
    "blocks": dict(B=2, Hkv=1, G=4, Nq=40, Ncap=200, lens=(200, 150), nq=(32, 33), seed=8200),
    # S > 1 by the split rule; an idle slot behind the merge
    "split": dict(B=2, Hkv=1, G=2, Nq=4, Ncap=8192, lens=(8000, 4100), nq=(3, 0), seed=8300),
}

# Not one of the parity families: full counts on a shape whose last wave is partly filled by rows that have no peer in it.  G = 1 and
# Nq = 40: wave 1 holds rows 32 .. 39 and 24 lanes past Nq, which the un-ragged kernel gives the limits of rows 0 .. 23 (q_row % Nq).
# Under the causal mask at L = 200 those limits (161 .. 184) end two tiles below the live rows' (193 .. 200), and the K/V heads
# with an odd index visit tile 3 first: lanes and live rows meet their first key in different tiles.  The ragged kernel must give
# such lanes the same limits when every n_b = Nq, or a reference maximum moves in another tile and live rows round differently.
# Its keys are NOT boosted: behind a boosted tile 3 no later tile could raise a live row's maximum, and a vote would change no bit.
EXTRA = {
    "tail": dict(B=2, Hkv=2, G=1, Nq=40, Ncap=256, lens=(200, 71), nq=(40, 40), seed=8700, boost=False),
}


def family(name):
    return FAMILIES[name] if name in FAMILIES else EXTRA[name]


def shape(f):
    return tuple(f[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))


def want_S(f, W):
    """the split count of a launch: from the PADDED shape (window 0: the capacity, else the window's span)"""
    B, Hkv, G, Nq, Ncap = shape(f)
    return wi.split_count(B * Hkv, G * Nq, Ncap) if W == 0 else wi.splits(B * Hkv, G * Nq, Nq, Ncap, W)


# ---- the limits -----------------------------------------------------------------------------------------------------------------------
def limits(lens, nq, B, Hkv, G, Nq, Ncap, causal, W):
    """-> lo, c int64 and live bool, each [B * Hkv * G, Nq] (ci.decode_limits with the sequence's own count)"""
    Hq = Hkv * G
    out = [np.zeros((B * Hq, Nq), t) for t in (np.int64, np.int64, bool)]
    for b, n in enumerate(cm.counts(nq, B, Nq)):
        for a, x in zip(out, cm.row_limits(cm.clamp(lens[b], Ncap), n, Nq, causal, W)):
            a[b * Hq:(b + 1) * Hq] = x
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(oracle, name, d, fmt):
    """di.inputs of the family with the tail keys boosted (module docstring) -> (q, k, v) fp32 16-bit-rounded and their encodings"""
    f = family(name)
    B, Hkv, G, Nq, Ncap = shape(f)
    (q, k, v), _ = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, f["seed"])
    q, k = q.copy(), k.copy()
    for b in range(B if f.get("boost", True) else 0):
        L = cm.clamp(f["lens"][b], Ncap)
        q[b * Hkv * G:(b + 1) * Hkv * G, :, 0] = BOOST
        k[b * Hkv:(b + 1) * Hkv, max(0, L - Nq):L, 0] = np.sqrt(d)
    bits = tuple(oracle.encode16(x, fmt) for x in (q, k, v))
    vals = tuple(oracle.decode16(x, fmt) for x in bits)
    for a in vals + bits:
        a.setflags(write=False)
    return vals, bits


@functools.lru_cache(maxsize=None)
def reference(oracle, name, d, fmt, W, causal, ragged=True, variant="none"):
    """cm.expected_f64 of a family, computed once and read-only; ragged=False: what a kernel that ignores seqlens_q would return"""
    f = FAMILIES[name]
    B, Hkv, G, Nq, Ncap = shape(f)
    (q, k, v), _ = inputs(oracle, name, d, fmt)
    sinks, softcap = li.options(variant, Hkv * G)
    out, lse = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, causal, W, softcap=softcap, sinks=sinks, nq=f["nq"] if ragged else None)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def live_rows(name):
    """[B * Hq, Nq] bool"""
    f = FAMILIES[name]
    B, Hkv, G, Nq, Ncap = shape(f)
    return limits(f["lens"], f["nq"], B, Hkv, G, Nq, Ncap, True, 0)[2]


def poison_dead_q(qb, name):
    """q encodings [B*Hq, Nq, d] -> a copy with a NaN bit pattern in every element of every dead row"""
    out = np.array(qb)
    out[~live_rows(name)] = cm.NAN16
    return out


# ---- the census -----------------------------------------------------------------------------------------------------------------------
def census_check(ci, O, lse, S, cnt, m, sink, live, what):
    """ci.census_check on rows that divide by cnt + 1 where the row is live and its head has a sink of 0, else by cnt; the row totals
    and exp(lse) decided between neighbouring integers as in li.sink_census_check; dead rows exact zeros and -inf.
    O, S [bh, Nq, d]; lse, cnt, live [bh, Nq]; m, sink [bh]"""
    O, lse = np.asarray(O, np.float64).reshape(S.shape), np.asarray(lse, np.float64).reshape(cnt.shape)
    den = cnt + (np.asarray(sink)[:, None] * live)
    assert not np.isnan(lse).any() and np.isfinite(O).all(), what
    assert (O[~live] == 0).all() and (lse[~live] == -np.inf).all(), what + ": a dead row is not exactly 0 / -inf"
    ci.census_check(O, S, den, m, what=what)
    total = O.sum(-1) * den / np.asarray(m, np.float64)[:, None]
    assert (np.abs(total - cnt) <= ci.MARGIN).all(), f"{what}: row totals off by {np.abs(total - cnt).max():.3f}"
    with np.errstate(over="ignore"):
        assert (np.abs(np.exp(lse) - den) <= ci.MARGIN).all(), f"{what}: exp(lse) off by {np.abs(np.exp(lse) - den).max():.3f}"


# ---- the append -----------------------------------------------------------------------------------------------------------------------
def lens_after(lens, new, B, nnew, ncap):
    """what seqlens_out receives: min(L_b + m_b, Ncap) (lens None: every sequence empty)"""
    start = [0] * B if lens is None else [cm.clamp(L, ncap) for L in lens]
    return np.array([min(L + m, ncap) for L, m in zip(start, cm.counts(new, B, nnew))], np.int32)


def place(cache, rows, lens, new, table=None):
    """The cache [B, Hkv, Ncap, d] (table None) or pool [num_pages, Hkv, ps, d] after the append of the first m_b tokens of `rows`
    [B, Hkv, Nnew, d] (in the cache's element type, already rotated or quantised): append_inputs' placement, token by token."""
    out = np.array(cache)
    B, nnew = rows.shape[0], rows.shape[2]
    ncap = cache.shape[2] if table is None else table.shape[1] * cache.shape[2]
    start = [0] * B if lens is None else [cm.clamp(L, ncap) for L in lens]
    for b, m in enumerate(cm.counts(new, B, nnew)):
        for t in range(m):
            p = start[b] + t
            if p >= ncap:
                continue
            if table is None:
                out[b, :, p] = rows[b, :, t]
            else:
                ps = cache.shape[2]
                page = int(table[b, p // ps])
                if 0 <= page < cache.shape[0]:
                    out[page, :, p % ps] = rows[b, :, t]
    return out


def keep_dead_q(q_rot, q_src, new):
    """Qout [B, Hq, Nnew, d]: the rotated rows of the first m_b tokens, the source bits of the rest"""
    out = np.array(q_rot)
    for b, m in enumerate(cm.counts(new, q_src.shape[0], q_src.shape[2])):
        out[b, :, m:] = q_src[b, :, m:]
    return out
