"""Seeded inputs for tests/test_gpu_kvcache_logits.py -- attention sinks and soft-capped logits on KV-cache decode (fa_kvcache_decode
behind the `sinks` and `softcap` keywords of the four decode front ends) -- with the options of every launch, and the
helpers that show each launch could not pass on a kernel that ignores the feature (tests/test_logit_inputs.py asserts them without a
GPU).  Pure numpy plus the `oracle` fixture (tests/conftest.py); nothing here touches a GPU.  The reference is
tests/common_inputs.py::expected_f64 with its `softcap` and `sinks` arguments.

Shapes, inputs and poison are tests/window_inputs.py's (its three families are already the smallest that reach one pass, a split with
empty splits and a start inside a tile, and five rows on folded heads under both masks).  What is new here:
  soft-cap  t_j = softcap * tanh(s_j / softcap) on every logit, before the masks
  sinks     one extra key per row with the head's logit a (natural-log units, not scaled, not capped) and a zero V row:
            O_i = sum_j exp(t_j) v_j / (exp(a) + sum_j exp(t_j)),  lse_i = ln(exp(a) + sum_j exp(t_j));
            a row without a key: O = 0 and lse = a;  a = -inf: no sink for the head
"""
import functools

import numpy as np

import census_inputs as ci
import common_inputs as cm
import window_inputs as wi

SOFTCAP = 1.0                       # the parity value: at the default scale it moves lse by 0.26 .. 0.56 and O by 0.05 .. 0.34
VARIANTS = ("sinks", "softcap", "both")
LSE_MOVES = 0.05                    # what the feature must move a live row's lse by, so that a kernel that ignores it fails
WINDOWED = {"one_pass": 65, "split": 1024, "rows": 64}   # the one windowed value per case; 0 (no window) is the other


def sinks_for(Hq):
    """per-head sinks in [6.5, 9.5), distinct across neighbouring heads: a >= lse_0 - 2.97 moves lse by >= 0.05, and the no-sink
    log-sum-exps of these shapes lie between about 1 and 9"""
    return np.array([6.5 + 3.0 * ((3 * h) % 8) / 8.0 for h in range(Hq)], np.float32)


def options(variant, Hq):
    """-> (sinks [Hq] fp32 or None, softcap)"""
    assert variant in VARIANTS + ("none",)
    return (sinks_for(Hq) if variant in ("sinks", "both") else None), (SOFTCAP if variant in ("softcap", "both") else 0.0)


def case_windows(name):
    return (0, WINDOWED[name])


def want_S(name, W):
    """the split count of a launch of a case: the window's span in place of the capacity (window 0: the capacity)"""
    c = wi.CASES[name]
    bh, rows = c["B"] * c["Hkv"], c["G"] * c["Nq"]
    return wi.split_count(bh, rows, c["Ncap"]) if W == 0 else wi.splits(bh, rows, c["Nq"], c["Ncap"], W)


@functools.lru_cache(maxsize=None)
def reference(oracle, name, d, fmt, W, causal, variant, scale=None):
    """cm.expected_f64 of a case of wi.CASES under a variant ("none": the feature off), computed once and read-only"""
    c = wi.CASES[name]
    (q, k, v), _ = wi.inputs(oracle, c["B"], c["Hkv"], c["G"], c["Nq"], c["Ncap"], d, fmt, c["seed"])
    sinks, softcap = options(variant, c["Hkv"] * c["G"])
    out, lse = cm.expected_f64(q, k, v, c["lens"], c["B"], c["Hkv"], c["G"], c["Nq"], causal, W, scale=scale, softcap=softcap, sinks=sinks)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


LAUNCHES = [(name, W, causal, variant) for name, c in wi.CASES.items() for W in case_windows(name) for causal in c["causal"]
            for variant in VARIANTS]


def feature_shows(oracle, name, d, fmt, W, causal, variant, without="none"):
    """the reference of `variant` against the reference of `without` (the same launch with an option taken away): what a kernel
    that ignores that option would be off by.  -> (fraction of live rows whose lse moves by >= LSE_MOVES, largest move of O)"""
    o1, l1 = reference(oracle, name, d, fmt, W, causal, variant)
    o0, l0 = reference(oracle, name, d, fmt, W, causal, without)
    live = np.isfinite(reference(oracle, name, d, fmt, W, causal, "none")[1])
    assert live.any()
    return float((np.abs(l1[live] - l0[live]) >= LSE_MOVES).mean()), float(np.abs(o1 - o0).max())


# ---- the sink census ------------------------------------------------------------------------------------------------------------------
# (case, window, causal): one pass and S = 1 on folded heads under both masks; S = 4 with empty splits, windowed and not; S = 16
CENSUS = (("one_pass", 65, False), ("rows", 64, False), ("rows", 64, True), ("rows", 0, True), ("split", 1024, False), ("split", 0, False))


def census_sinks(Hq):
    """per-head sinks alternating 0.0 and -inf: a sink of 0 next to scores of 0 has weight exactly 1"""
    return np.array([0.0 if h % 2 == 0 else -np.inf for h in range(Hq)], np.float32)


def census_case(oracle, name, d, fmt, W, causal):
    """family Z of tests/census_inputs.py on a case: K = 0, V in the residue coding with m_h -> dict bits (q, k, v encodings),
    S [B*Hq, Nq, d] the integer column sums, cnt [B*Hq, Nq] the keys a row sees, m per query head, sink [B*Hq] 1 where the head has
    a sink of 0"""
    c = wi.CASES[name]
    B, Hkv, G, Nq, Ncap = (c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
    z = ci.z_decode(oracle, B, Hkv, G, Nq, Ncap, d, fmt, "residue")
    lo, lim = ci.decode_limits(c["lens"], B, Hkv, G, Nq, Ncap, causal, W)
    S, m_q = ci.decode_sums(z["m"], lo, lim, G, Ncap, d, "residue")
    sink = np.tile(np.isfinite(census_sinks(Hkv * G)), B).astype(np.int64)
    return dict(bits=z["bits"], S=S, cnt=lim - lo, m=m_q, sink=sink, s_max=float(S.max()))


def sink_census_check(O, lse, z, what="sink census"):
    """O [B*Hq, Nq, d] and lse [B*Hq, Nq] (numpy, fp32 results or a float64 model) against census_case's z, each a decision between
    neighbouring integers with the census's MARGIN.  With den_i = cnt_i + 1 on a head with a sink of 0 and cnt_i on a head with
    -inf: O * den equals the integer column sums (ci.census_check: a key dropped, doubled or taken from another head), the row
    total sum_col O * den / m equals cnt_i (a single column holds about cnt / d of it, too little to tell den from den + 1; the
    total does), and exp(lse) rounds to den_i (0 for a row with neither key nor sink: lse = -inf)."""
    den = z["cnt"] + z["sink"][:, None]
    O = np.asarray(O, np.float64).reshape(z["S"].shape)
    lse = np.asarray(lse, np.float64).reshape(den.shape)
    assert not np.isnan(lse).any() and np.isfinite(O).all(), what
    ci.census_check(O, z["S"], den, z["m"], what=what)
    total = O.sum(-1) * den / z["m"][:, None]
    assert (np.abs(total - z["cnt"]) <= ci.MARGIN).all(), f"{what}: row totals off by {np.abs(total - z['cnt']).max():.3f}"
    assert (np.abs(np.exp(lse) - den) <= ci.MARGIN).all(), f"{what}: exp(lse) off by {np.abs(np.exp(lse) - den).max():.3f}"
