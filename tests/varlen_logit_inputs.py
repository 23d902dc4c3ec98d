"""Seeded inputs for tests/test_gpu_varlen_logits.py -- fa_forward_varlen_ex: the variable-length packed prefill with a sliding window,
soft-capped logits and attention sinks -- with the entry restated in float64 numpy on tests/varlen_inputs.py's conventions (packing,
clamped bounds, NaN tail rows, poison, the one check `problems`), and nine WRONG restatements, each a plausible kernel bug.  Pure
numpy; nothing here touches a GPU (tests/test_varlen_logit_inputs.py asserts, without one, that no parity launch could pass on a
kernel that ignores or mis-implements an option).

Semantics, from include/fa_mi355.h, for row i of a sequence with Lq rows and Lk keys, query head hq:
  window W >= 1   the row sees [lo_i, c_i), lo_i = max(0, Lk - Lq + 1 + i - W), the same with and without the causal flag; c_i = Lk
                  without it, max(0, Lk - Lq + 1 + i) with it.  W = 0: lo_i = 0
  softcap > 0     t_j = softcap * tanh(s_j / softcap) on every logit s_j = scale q.k_j, before the masks
  sinks           one extra key with the logit a = sinks[hq] (natural log, not scaled, not capped) and a zero V row, under any mask:
                  O_i = sum_j exp(t_j) v_j / (exp(a) + sum_j exp(t_j)), lse_i = ln(exp(a) + sum_j exp(t_j)); a row without a key:
                  O = 0, lse = a; a = -inf: no sink for the head.  Rows of no sequence are not written.
"""
import functools

import numpy as np

import common_inputs as cm
import varlen_inputs as vi

TILE = cm.TILE            # 64 keys per K/V tile
SOFTCAP = 1.0             # at the default scale the logits are about N(0, 1): tanh bends them visibly (tests/logit_inputs.py's value)
WINDOWS = (1, 17, 64, 100)   # every causal row sees its own key only; inside a tile; a tile edge; straddling two

# vi.LQ against itself and against vi.LK2, plus one batch whose 449-row sequence makes a workgroup skip several leading tiles and, in
# its second block (rows 128..255), puts the first and the last wave 96 rows -- more than one 64-key tile -- apart
BATCHES = {"self": (vi.LQ, vi.LQ), "cross": (vi.LQ, vi.LK2), "long": ((449, 130), (449, 513))}

# (batch, Hkv, G, d, fmt, causal, out_f32, scale, W, softcap on, sinks on); scale None = 1/sqrt(d)
CASES = (
    ("self", 2, 2, 64, 0, 1, 1, None, 17, 0, 0),
    ("self", 1, 4, 128, 1, 1, 0, None, 64, 1, 0),
    ("self", 3, 1, 128, 0, 0, 1, None, 100, 0, 1),
    ("self", 2, 2, 64, 1, 0, 0, None, 1, 1, 1),
    ("cross", 2, 2, 128, 0, 1, 1, None, 1, 0, 1),
    ("cross", 1, 4, 64, 1, 0, 1, None, 17, 1, 0),
    ("cross", 3, 1, 64, 0, 1, 0, None, 100, 1, 1),
    ("cross", 2, 2, 128, 1, 0, 0, None, 64, 0, 0),
    ("long", 2, 2, 64, 0, 1, 1, None, 64, 0, 1),
    ("long", 1, 4, 128, 0, 1, 0, None, 100, 1, 0),
    ("long", 2, 2, 128, 1, 0, 1, None, 17, 0, 1),
    ("long", 3, 1, 64, 1, 1, 0, None, 1, 1, 1),
    ("self", 2, 2, 64, 0, 1, 1, None, 0, 1, 0),        # the cap alone
    ("cross", 2, 2, 128, 0, 1, 1, None, 0, 0, 1),      # the sinks alone
    ("long", 1, 4, 64, 0, 1, 1, -0.125, 100, 1, 1),    # a negative scale: tanh is odd
    ("cross", 1, 4, 128, 1, 1, 1, None, 17, 1, 1),
)


def case_id(c):
    batch, Hkv, G, d, fmt, causal, f32, scale, W, cap, snk = c
    return (f"{batch}-Hkv{Hkv}G{G}-d{d}-{cm.FMT_NAME[fmt]}-{'causal' if causal else 'full'}-{'f32' if f32 else 'o16'}-W{W}"
            + ("-cap" if cap else "") + ("-sinks" if snk else "") + ("" if scale is None else f"-scale{scale}"))


def sinks_for(Hq):
    """a mixed vector: every second head has no sink (-inf), the others distinct finite logits in [1.5, 3.5) -- next to rows that see
    one key (lse about 0) and rows that see hundreds (lse about 6)"""
    return np.array([1.5 + 0.5 * (h % 4) if h % 2 == 0 else -np.inf for h in range(Hq)], np.float32)


@functools.lru_cache(maxsize=None)
def make(case):
    """one parity case -> dict as vi.make's, plus W, softcap and sinks ([Hq] float32 or None)"""
    batch, Hkv, G, d, fmt, causal, f32, scale, W, cap, snk = case
    lq, lk = BATCHES[batch]
    seed = 3000 + CASES.index(case) if case in CASES else 2999
    q, qb = vi.packed(lq, Hkv * G, d, fmt, seed)
    k, kb = vi.packed(lk, Hkv, d, fmt, seed + 100)
    v, vb = vi.packed(lk, Hkv, d, fmt, seed + 200)
    return dict(q=q, k=k, v=v, qb=qb, kb=kb, vb=vb, cu_q=vi.cu_of(lq), cu_k=vi.cu_of(lk), Hkv=Hkv, G=G, d=d, fmt=fmt, causal=bool(causal),
                f32=bool(f32), scale=(1.0 / np.sqrt(d)) if scale is None else float(scale), lq=lq, lk=lk, W=W,
                softcap=SOFTCAP if cap else 0.0, sinks=sinks_for(Hkv * G) if snk else None)


# ---- the limits of a sequence's rows -------------------------------------------------------------------------------------------------
WRONG = ("no_window", "lo_low", "lo_high", "lo_start", "t0_last", "cap_after", "sink_scaled", "sink_per_tile", "sink_dead")


def limits(Lq, Lk, causal, W, wrong=None):
    """-> (lo [Lq], c [Lq]) int64: row i sees the keys [lo_i, c_i) (none when lo_i >= c_i).  wrong --
      no_window  the window ignored
      lo_low     lo_i one too low (W + 1 keys under the mask)
      lo_high    lo_i one too high (W - 1 keys)
      lo_start   lo aligned to the START of the keys, i + 1 - W
      t0_last    the workgroup's first tile taken from its LAST row, so its earlier rows lose the keys below that tile"""
    i = np.arange(Lq, dtype=np.int64)
    pos = Lk - Lq + 1 + i
    c = np.maximum(0, pos) if causal else np.full(Lq, Lk, np.int64)
    if W == 0 or wrong == "no_window":
        return np.zeros(Lq, np.int64), c
    lo = np.maximum(0, pos - W - (wrong == "lo_low") + (wrong == "lo_high"))
    if wrong == "lo_start":
        lo = np.maximum(0, i + 1 - W)
    if wrong == "t0_last":
        last = np.minimum(Lq - 1, i // vi.BM * vi.BM + vi.BM - 1)
        lo = np.maximum(lo, np.maximum(0, Lk - Lq + 1 + last - W) // TILE * TILE)
    return lo, c


# ---- the entry in float64, and the wrong ones ------------------------------------------------------------------------------------------
def varlen_logits_f64(q, k, v, cu_q, cu_k, Hkv, G, causal, scale, W=0, softcap=0.0, sinks=None, wrong=None, base=None):
    """-> (O (total_q, Hq, d), lse (Hq, total_q)) float64.  Rows of no sequence hold `base` = (O value, lse value), default (0, -inf).
    wrong: None, one of limits()'s, or --
      cap_after      the cap applied after the masks: a masked key of the sequence becomes the finite logit -softcap
      sink_scaled    the sink logit multiplied by scale
      sink_per_tile  the sink counted once per 64-key tile that holds a visible key of the row
      sink_dead      rows of no sequence get the sink too: O = 0, lse = sinks[hq]"""
    total_q, Hq, d = q.shape
    total_k = k.shape[0]
    assert Hq == Hkv * G and wrong in (None,) + WRONG
    o0, l0 = (0.0, -np.inf) if base is None else base
    out = np.full(q.shape, o0, np.float64)
    lse = np.full((Hq, total_q), l0, np.float64)
    if wrong == "sink_dead" and sinks is not None:
        dead = ~vi.owned(cu_q, total_q)
        for hq in range(Hq):
            if np.isfinite(sinks[hq]):
                out[dead, hq] = 0.0
                lse[hq, dead] = float(sinks[hq])
    for (sq, eq), (sk, ek) in zip(vi.bounds(cu_q, total_q), vi.bounds(cu_k, total_k)):
        Lq, Lk = eq - sq, ek - sk
        if Lq == 0:
            continue
        lo, c = limits(Lq, Lk, causal, W, wrong)
        j = np.arange(Lk, dtype=np.int64)
        vis = (j[None, :] >= lo[:, None]) & (j[None, :] < c[:, None])                      # (Lq, Lk)
        tiles = np.where(c > lo, (np.maximum(c, 1) - 1) // TILE - lo // TILE + 1, 1)         # tiles with a visible key (1: none)
        for hq in range(Hq):
            hk = hq // G
            s = (q[sq:eq, hq].astype(np.float64) @ k[sk:ek, hk].astype(np.float64).T) * scale
            if softcap > 0.0:
                s = softcap * np.tanh(s / softcap)
            t = np.where(vis, s, -softcap if (wrong == "cap_after" and softcap > 0.0) else -np.inf)
            a = -np.inf if sinks is None else float(sinks[hq]) * (scale if wrong == "sink_scaled" else 1.0)
            m = np.maximum(t.max(axis=1, initial=-np.inf), a)                               # (Lq,)
            none = ~np.isfinite(m)                                                          # neither key nor sink
            ms = np.where(none, 0.0, m)
            p = np.exp(t - ms[:, None])
            with np.errstate(over="ignore"):
                ws = np.exp(a - ms) * (tiles if wrong == "sink_per_tile" else 1.0) if np.isfinite(a) else np.zeros(Lq)
            den = p.sum(axis=1) + ws
            out[sq:eq, hq] = np.where(none[:, None], 0.0, (p @ v[sk:ek, hk].astype(np.float64)) / np.where(none, 1.0, den)[:, None])
            with np.errstate(divide="ignore"):
                lse[hq, sq:eq] = np.where(none, -np.inf, ms + np.log(np.where(none, 1.0, den)))
    return out, lse


def run_f64(c, wrong=None, base=None, **over):
    """varlen_logits_f64 on a made case; `over` replaces options (W=0: the window dropped, ...)"""
    o = dict(W=c["W"], softcap=c["softcap"], sinks=c["sinks"])
    o.update(over)
    return varlen_logits_f64(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["Hkv"], c["G"], c["causal"], c["scale"], wrong=wrong, base=base,
                             **o)


@functools.lru_cache(maxsize=None)
def expected(case):
    """the reference of the parity tests: computed once, shared and read-only"""
    out, lse = run_f64(make(case))
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def dropped(c):
    """[(name, options)] of a case with one of its options taken away: what a kernel that ignores that option computes"""
    out = []
    if c["W"]:
        out.append(("window", dict(W=0)))
    if c["softcap"]:
        out.append(("softcap", dict(softcap=0.0)))
    if c["sinks"] is not None:
        out.append(("sinks", dict(sinks=None)))
    return out
