"""Inputs, closed-form expected values and the criterion of the key census (tests/test_gpu_census.py; tests/test_census_inputs.py
asserts everything here without a GPU).  Pure numpy plus the `oracle` fixture (tests/conftest.py); the two *_torch helpers take the
torch module from their caller and work on whatever device their arguments live on.

The census makes ACCOUNTING errors discrete.  With weights that are uniform over the keys a row sees and V entries that are 0 or
one small integer m_h per head, O[h, i, col] * cnt_i is the integer S[h, i, col] = sum of V[h, j, col] over the keys j in
[lo_i, c_i) (c_i: the row's upper limit; cnt_i = c_i - lo_i: the number of keys it sees).  A key that is dropped, counted twice,
taken from another tile or from another head moves S by at least min(m_h), so the criterion is a decision between neighbouring
integers, not a tolerance.

V codings (every entry 0 or m_h, exact in fp16, bf16 and e4m3fn):
  residue  V[h, j, col] = m_h where col == j % d          -- a dropped or doubled key or tile changes one column count by one
  tile     V[h, j, col] = m_h where col == (j // 64) % d  -- a tile read in place of another moves 64 from one column to another
m_h differs between neighbouring heads (family Z), so rows of another head show as S off by a multiple of another m.

Family Z: K = 0, Q random.  Every score is exactly 0 whatever the scale; the weights are identical across keys in every pass.
Family R: K[h, j] = k0_h for all j; row i has ONE score s_i, and Q is scaled row by row so that s_i takes the value its regime
needs.  Weights are uniform within a row, while references, gates and the fallback chain of the pipeline see real logits.

The exactness rule (asserted for every listed shape by the CPU tier):
  fp32 output, family Z and the rp16 kernels: a packed weight has P_BITS[fmt] significant bits, so products and sums are exact
  while P_BITS + log2(S) <= 24; one division remains -- the deviation is about count * 2^-22 (count = S / m_h).
  family R: a kernel may add up unrounded fp32 weights while P.V uses the packed ones: a relative P_EPS[fmt].  Shapes keep
  4 * P_EPS[fmt] * max(count) <= 0.125: fp16 count <= 64, bf16 count <= 8 (so bf16 uses the residue coding only).
  16-bit output: only shapes with 2 * P_EPS[fmt] * max(count) <= 0.125.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_inputs as di
import fallback_inputs as fi

F16, BF16 = 0, 1
P_BITS = {F16: 11, BF16: 8}       # significant bits of a weight packed to the input format
MARGIN = 0.25                     # decision margin between neighbouring integers (not a measured tolerance)
CODINGS = ("residue", "tile")
LOG2E = fi.LOG2E


# ---- V codings and their closed-form sums -------------------------------------------------------------------------------------------
def head_values(bh, family):
    """m_h: family Z (h % 8) + 1 -- neighbouring heads differ; family R 1"""
    return np.array([(h % 8) + 1 if family == "Z" else 1 for h in range(bh)], np.float64)


def columns(n, d, coding):
    """the column key j marks: [n] int"""
    j = np.arange(n)
    assert coding in CODINGS
    return j % d if coding == "residue" else (j // cm.TILE) % d


def v_coded(m, n, d, coding):
    """-> V [bh, n, d] fp32: m_h in column columns(n, d, coding)[j] of key j, 0 elsewhere"""
    v = np.zeros((len(m), n, d), np.float32)
    v[:, np.arange(n), columns(n, d, coding)] = np.asarray(m, np.float32)[:, None]
    return v


def prefix_counts(n, d, coding):
    """P [n + 1, d] float64: P[t, col] = number of keys j < t that mark col (a float64 cumulative sum of the unit coding)"""
    unit = np.zeros((n + 1, d), np.float64)
    unit[np.arange(1, n + 1), columns(n, d, coding)] = 1.0
    return np.cumsum(unit, 0)


def expected_sums(m, lo, c, n, d, coding):
    """m [bh], lo and c [bh, rows] (or [rows]): row i of head h sees the keys [lo, c) of its head's n keys -> S [bh, rows, d]
    float64, S[h, i, col] = sum of V[h, j, col] over those keys."""
    P = prefix_counts(n, d, coding)
    lo, c = (np.broadcast_to(np.asarray(x, np.int64), (len(m), np.shape(x)[-1])) for x in (lo, c))
    assert (lo >= 0).all() and (c <= n).all()
    cnt = P[np.maximum(c, lo)] - P[lo]
    return np.asarray(m, np.float64)[:, None, None] * cnt


def expected_sums_torch(torch, m, lo, c, n, d, coding, device):
    """expected_sums in torch float64 on `device` (the full-size shapes): m [bh], lo and c [rows] int64 tensors or lists"""
    j = torch.arange(n, device=device)
    col = j % d if coding == "residue" else (j // cm.TILE) % d
    unit = torch.zeros((n + 1, d), dtype=torch.float64, device=device)
    unit[j + 1, col] = 1.0
    P = torch.cumsum(unit, 0)
    lo, c = (torch.as_tensor(x, dtype=torch.int64, device=device) for x in (lo, c))
    cnt = P[torch.maximum(c, lo)] - P[lo]                                     # [rows, d]
    return torch.as_tensor(m, dtype=torch.float64, device=device)[:, None, None] * cnt[None]


def v_coded_torch(torch, m, n, d, coding, dtype, device):
    j = torch.arange(n, device=device)
    col = j % d if coding == "residue" else (j // cm.TILE) % d
    v = torch.zeros((len(m), n, d), dtype=dtype, device=device)
    v[:, j, col] = torch.as_tensor(m, dtype=torch.float32, device=device).to(dtype)[:, None]
    return v


def max_count(lo, c, n, d, coding):
    """the largest S / m_h any row has"""
    return float(expected_sums(np.ones(1), np.asarray(lo).reshape(1, -1), np.asarray(c).reshape(1, -1), n, d, coding).max())


# ---- limits ---------------------------------------------------------------------------------------------------------------------------
def prefill_limits(n, causal):
    """fa_forward: row i sees [0, i + 1) under the mask, [0, n) without -> (lo [n], c [n])"""
    return np.zeros(n, np.int64), (np.arange(1, n + 1) if causal else np.full(n, n, np.int64))


def decode_limits(lens, B, Hkv, G, Nq, Ncap, causal, W=0):
    """the cache entries: per query head [B * Hkv * G, Nq] lower and upper limits (cm.row_limits; a bad length is clamped)"""
    lo = np.zeros((B * Hkv * G, Nq), np.int64)
    c = np.zeros((B * Hkv * G, Nq), np.int64)
    for b in range(B):
        hs = slice(b * Hkv * G, (b + 1) * Hkv * G)
        lo[hs], c[hs], _ = cm.row_limits(cm.clamp(lens[b], Ncap), Nq, Nq, causal, W)
    return lo, c


def decode_sums(m_kv, lo, c, G, n, d, coding):
    """m_kv [B * Hkv] (K/V heads), lo and c [B * Hkv * G, Nq] -> S [B * Hkv * G, Nq, d] and m per query head"""
    m_q = np.repeat(np.asarray(m_kv, np.float64), G)
    return expected_sums(m_q, lo, c, n, d, coding), m_q


# ---- the criterion ----------------------------------------------------------------------------------------------------------------------
def census_check(O, S, cnt, m, v_scale=1.0, what="census"):
    """O, S [bh, rows, d]; cnt [bh, rows] or [rows]: the NUMBER of keys a row sees (upper limit minus lower limit); m [bh].  numpy
    arrays, or torch tensors on one device.  Asserts |O * cnt / (m * v_scale) - S / m| <= MARGIN elementwise and that a row with
    cnt = 0 is all zeros; returns the largest deviation.  (The float64 reference has deviation 0.)"""
    c = cnt
    is_np = isinstance(O, np.ndarray)
    if is_np:
        O, S = np.asarray(O, np.float64), np.asarray(S, np.float64)
        c = np.broadcast_to(np.asarray(c, np.float64), O.shape[:2])
        m = np.asarray(m, np.float64).reshape(-1, 1, 1)
    else:
        import torch
        O, S = O.double(), S.double()
        c = torch.as_tensor(c, dtype=torch.float64, device=O.device).expand(O.shape[:2])
        m = torch.as_tensor(m, dtype=torch.float64, device=O.device).reshape(-1, 1, 1)
    assert O.shape == S.shape and O.ndim == 3, (O.shape, S.shape)
    dead = c == 0
    assert bool((O[dead] == 0).all()), what + ": a row without a key is not exactly zero"
    assert bool((S[dead] == 0).all())
    dev = abs(O * c[:, :, None] / (m * float(v_scale)) - S / m)
    worst = float(dev.max()) if (dev.size if is_np else dev.numel()) else 0.0
    if not worst <= MARGIN:   # (a NaN fails too)
        bad = (~(dev <= MARGIN)).nonzero()
        h, i, col = (int(x[0]) for x in (bad if is_np else bad.T))
        raise AssertionError(f"{what}: {int((~(dev <= MARGIN)).sum())} entries off, first at head {h} row {i} column {col}: "
                             f"O * c / m = {float(O[h, i, col] * c[h, i] / (m[h, 0, 0] * float(v_scale))):.4f}, "
                             f"S / m = {float(S[h, i, col] / m[h, 0, 0]):.1f} (c = {int(c[h, i])}, m = {float(m[h, 0, 0]):.0f})")
    return worst


# ---- the exactness rule ---------------------------------------------------------------------------------------------------------------
def z_exact(fmt, s_max):
    """family Z, fp32 output: products and sums exact"""
    return s_max <= 0 or P_BITS[fmt] + np.log2(s_max) <= 24


def r_exact(fmt, count_max):
    """family R: a sum of unrounded weights against packed ones in P.V"""
    return 4 * cm.P_EPS[fmt] * count_max <= 0.125


def out16_exact(fmt, count_max):
    """16-bit output: O itself is rounded to the format"""
    return 2 * cm.P_EPS[fmt] * count_max <= 0.125


# ---- family Z ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def z_prefill(oracle, bh, n, d, fmt, coding, seed=7000):
    """fa_forward inputs: Q random (oracle.make_qkv), K = 0, V coded with m_h = (h % 8) + 1 -> dict q, k, v fp32, bits, m"""
    (q, _, _), (qb, _, _) = oracle.make_qkv(bh, n, d, fmt=fmt, seed=seed + n + d)
    m = head_values(bh, "Z")
    k = np.zeros((bh, n, d), np.float32)
    v = v_coded(m, n, d, coding)
    bits = (qb, oracle.encode16(k, fmt), oracle.encode16(v, fmt))
    assert np.array_equal(oracle.decode16(bits[2], fmt), v)   # every entry is exact in the format
    for a in (q, k, v) + bits:
        a.setflags(write=False)
    return dict(q=q, k=k, v=v, bits=bits, m=m)


@functools.lru_cache(maxsize=None)
def z_decode(oracle, B, Hkv, G, Nq, Ncap, d, fmt, coding, seed=7100):
    """the cache entries: q [B * Hkv * G, Nq, d] random, k = 0 and v coded [B * Hkv, Ncap, d], m per K/V head"""
    (q, _, _), (qb, _, _) = oracle.make_qkv(B * Hkv * G, Nq, d, fmt=fmt, seed=seed + Ncap + d)
    m = head_values(B * Hkv, "Z")
    k = np.zeros((B * Hkv, Ncap, d), np.float32)
    v = v_coded(m, Ncap, d, coding)
    bits = (qb, oracle.encode16(k, fmt), oracle.encode16(v, fmt))
    for a in (q, k, v) + bits:
        a.setflags(write=False)
    return dict(q=q, k=k, v=v, bits=bits, m=m)


# ---- family R ---------------------------------------------------------------------------------------------------------------------------
# the three regimes, one head each (log2 units; d = 64: 64-row waves of a 512-row workgroup, d = 128: 32-row waves of a 256-row one;
# the half-width kernels halve both).  The patterns below repeat every 8 rows, so every 16-row block of every wave holds all of them.
REGIMES = ("folded", "row-sum gate", "beyond kFoldMax")
K_FOLD_MAX = 24.0                 # the largest kFoldMax of the fold kernels (fa_fwd_rp.hip 24, fa_fwd_rp16_kernel.hpp 16)
HIGH, LOW = 8.0, {F16: -14.0, BF16: -110.0}   # regime (b): rows at HIGH and at LOW in every 16-row block
GATE_LO_LOG2 = {F16: -16.0, BF16: -100.0}     # the lower row-sum gate: fp16 l >= c * 2^-16, bf16 l >= 2^-100
GATE_HI = 60000.0                              # the upper one
BEYOND = 30.0                                  # regime (c): every row's score


def r_targets(regime, n, fmt):
    """the score (log2 units) row i is built for"""
    i = np.arange(n)
    if regime == "folded":                  # within [1, 4): the whole wave within a few units, no Q row near zero
        return 1.0 + 3.0 * ((i * 37) % 64) / 64.0
    if regime == "row-sum gate":            # i % 8 == 0: HIGH, i % 8 == 1: LOW, the rest in [1, 2)
        return np.where(i % 8 == 0, HIGH, np.where(i % 8 == 1, LOW[fmt], 1.0 + ((i * 5) % 16) / 16.0))
    assert regime == "beyond kFoldMax"
    return BEYOND + ((i * 3) % 8) / 8.0


@functools.lru_cache(maxsize=None)
def r_case(oracle, n, d, fmt, coding, seed=7300):
    """Three heads of n rows, head r in regime REGIMES[r]: K[h, j] = k0_h (the first key oracle.make_qkv draws for the head), V coded
    with m = 1, Q drawn by oracle.make_qkv and scaled row by row to its target score (a row whose random score is below 0.25 log2
    units in magnitude is replaced by the multiple of k0_h with that score, so that no scale exceeds 4 |target|).  All values are
    rounded to the format; scores() measures what the rounded values give.  -> dict q, k, v, bits, m, targets [3, n]"""
    (q, k, _), _ = oracle.make_qkv(3, n, d, fmt=fmt, seed=seed + n + d + fmt)
    q = q.astype(np.float64)
    k0 = k[:, 0].astype(np.float64)
    targets = np.stack([r_targets(r, n, fmt) for r in REGIMES])
    unit = LOG2E / np.sqrt(d)
    for h in range(3):
        raw = (q[h] @ k0[h]) * unit
        weak = np.abs(raw) < 0.25
        q[h, weak] = k0[h] / ((k0[h] @ k0[h]) * unit)      # score 1
        raw[weak] = 1.0
        q[h] *= (targets[h] / raw)[:, None]
    m = head_values(3, "R")
    kk = np.repeat(k0[:, None, :], n, axis=1).astype(np.float32)
    bits = tuple(oracle.encode16(x, fmt) for x in (q.astype(np.float32), kk, v_coded(m, n, d, coding)))
    q, kk, v = (oracle.decode16(b, fmt) for b in bits)
    for a in (q, kk, v) + bits:
        a.setflags(write=False)
    targets.setflags(write=False)
    return dict(q=q, k=kk, v=v, bits=bits, m=m, targets=targets)


def scores(case):
    """[bh, n] float64: the one score (log2 units, scale 1 / sqrt(d)) of every row, from the rounded values; asserts K is row-constant"""
    q, k = case["q"], case["k"]
    assert (k == k[:, :1]).all()
    return np.einsum("hid,hd->hi", q.astype(np.float64), k[:, 0].astype(np.float64)) * (LOG2E / np.sqrt(q.shape[2]))


def fold_reference(s_wave, n_keys, causal):
    """the folded pass' reference for one wave (fa_fwd_rp16_body.inc, restated in float64): the maximum over the wave's rows and
    first 32 keys + 1 under the mask; without one, placed so that N * (mean weight of those scores) lands at 2^6, the shift
    clamped to [-6, kFoldMax]."""
    mx = s_wave.max()
    if causal:
        return mx + 1.0
    e = np.exp2(s_wave - mx).mean()
    return mx + min(max(np.log2(n_keys * e) - 6.0, -6.0), 16.0)


def assert_regimes(case, d, fmt, causal, wave_rows):
    """(a) every wave of head 0: reference within kFoldMax = 16, every row sum inside the gates' window -- stays folded;
    (b) every wave of head 1: reference within 16, yet a row 20 or more units below its wave's maximum whose row sum lies below
        the lower gate (above and below in one wave: HIGH and LOW are 22 or more apart) -- refused by the row-sum gate; the exact
        pass' own reference is the row's score + 4, so its weights are 2^-4 and it keeps the block;
    (c) every wave of head 2: a reference beyond the largest kFoldMax (24) -- fp16 goes straight to the running-max pass (the redo
        list of the full-width kernels), bf16 to the exact pass."""
    s = scores(case)
    n = s.shape[1]
    # the scores lie where they were built, up to the rounding of Q and K to the format: 2 P_EPS on every product of the row
    slack = 2 * cm.P_EPS[fmt] * np.einsum("hid,hd->hi", np.abs(case["q"]).astype(np.float64), np.abs(case["k"][:, 0]).astype(np.float64)) \
        * (LOG2E / np.sqrt(d))
    assert (np.abs(s - case["targets"]) <= slack + 1e-6).all(), np.abs(s - case["targets"]).max()
    folded_q = np.abs(case["q"]).max() * LOG2E / np.sqrt(d)
    assert folded_q < 65504.0 / 4
    for r0 in range(0, n, wave_rows):
        rows = np.arange(r0, min(n, r0 + wave_rows))
        seen = np.minimum(rows + 1, n) if causal else np.full(len(rows), n)
        for h in range(3):
            ref = fold_reference(s[h, rows], n, causal)
            lsum = np.log2(seen) + s[h, rows] - ref          # log2 of the row sum of the folded pass
            lo_gate = GATE_LO_LOG2[fmt] + (np.log2(seen) if fmt == F16 else 0.0)
            if h == 0:
                assert abs(ref) <= 15.0 and (lsum < np.log2(GATE_HI) - 1).all() and (lsum >= lo_gate + 1).all(), (r0, ref)
                assert s[h, rows].max() - s[h, rows].min() <= 3.0
            elif h == 1:
                assert abs(ref) <= 15.0, (r0, ref)
                if len(rows) >= 2 and (rows % 8 == 1).any():
                    assert (lsum < lo_gate - 1).any(), (r0, lsum.min(), lo_gate)
                    assert s[h, rows].max() - s[h, rows].min() >= 20.0
            else:
                assert abs(ref) > K_FOLD_MAX + 1 and s[h, rows].min() > K_FOLD_MAX + 1, (r0, ref)


# ---- the GPU shapes (tests/test_gpu_census.py takes them from here; the CPU tier asserts the exactness rule for each) -------------
Z_PREFILL_N = {64: (1, 63, 64, 65, 257, 600, 1000, 2049), 128: (1, 65, 300, 513, 1000), 16: (17, 100, 257), 32: (17, 100, 257),
               256: (17, 100, 257)}
Z_BH = 3
CAUSAL_ALGOS = {64: (0, 1, 2, 6, 24), 128: (0, 1, 2, 6, 24, 28)}
Z_OUT16 = dict(bh=3, n=257, d=64)                       # the short 16-bit-output shape; codings by out16_exact
GRID_CAUSAL = ((300, 1000, 64), (300, 1000, 128), (700, 600, 64))   # (BH, N, d), algos 0 and 24: more items than CUs
GRID_ALGOS = (0, 24)
GRID_BENCH = dict(B=8, H=16, n=4096, d=64)
GRID_1W = dict(n=8192, d=128, algo=28)                  # BH = CUs // 8
R_SHAPES = {(64, F16): (600, 1000), (64, BF16): (333, 512), (128, F16): (300, 600), (128, BF16): (300, 600)}
R_ALGOS = {64: (24, 26, 27, 29, 23), 128: (24, 28)}
R_CAUSAL_ALGOS = {64: (24,), 128: (24, 28)}
R_HALF_WIDTH = (26, 27, 29)
WAVE_ROWS = {64: 64, 128: 32}
SPLITKV = di.D_SPLITKV + ((130, 777),)                  # (nq, nk), two heads each; 130 rows: two row blocks


def r_codings(fmt):
    return CODINGS if fmt == F16 else ("residue",)


def out16_codings(fmt):
    lo, c = prefill_limits(Z_OUT16["n"], False)
    return tuple(cd for cd in CODINGS if out16_exact(fmt, max_count(lo, c, Z_OUT16["n"], Z_OUT16["d"], cd)))
