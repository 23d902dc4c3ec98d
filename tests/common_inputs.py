"""What every KV-cache test module shares: the project's bounds, the one statement of which keys a row sees, the decode references,
the page scatter with its poison, and the two host-to-device conversions.  Pure numpy plus the `oracle` fixture (tests/conftest.py);
the device helpers take the torch module from their caller.  Imports none of the per-feature modules (tests/*_inputs.py), which keep
their cases, seeds, families and the host's arithmetic restated.

Semantics, from include/fa_mi355.h.  L = min(max(length, 0), Ncap).  Nq is the padded row count and n = min(max(count, 0), Nq) the
live one (no counts: n = Nq).  Row i < n of every head sees the keys [lo_i, c_i): c_i = max(0, L - n + 1 + i) under the causal mask
(aligned to the end of the sequence) and L without, lo_i = max(0, L - n + 1 + i - W) under a window of W keys and 0 without (W = 0).
A live row without a key has O = 0 and lse = -inf (the sink logit where its head has one); a dead row, i >= n, has O = 0 and
lse = -inf exactly, sinks or not.
"""
import numpy as np

# ---- the project's bounds (tests/test_gpu_parity.py documents their origin and imports them from here) ------------------------------
MAX_ABS = 1e-2                          # the project's north-star tolerance
REL_L2 = {0: 2e-3, 1: 1.2e-2}           # fp16 / bf16 inputs (P is rounded to the input type)
P_EPS = {0: 2.0 ** -11, 1: 2.0 ** -8}   # largest relative rounding error of one weight in the format P is packed to
NAN16 = 0x7FFF                          # a NaN in fp16 and in bf16
GARBAGE = (-1, 1 << 30)                 # what a block table holds for a page no visible key lies in
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
TILE = 64                               # kBlockN
ROWS = 128                              # split::kRows, query rows per workgroup
FMT_NAME = {0: "fp16", 1: "bf16"}


def peaked_tol(fmt, vmax, kernels=1):
    """The tolerance model of tools/fuzz_gpu.py, for inputs that make sharply PEAKED rows (large logits, the first rows under the
    causal mask): the north-star bar plus what the 16-bit format of P itself imposes.  A row whose weight sits on two or three
    comparable keys moves by at most (relative rounding of one weight, P_EPS) x (the spread of the dominant V rows, <= 2 vmax, of
    which a convex combination keeps at most vmax).  `kernels` = how many independently rounding kernels the difference is taken
    between (2 when comparing two of ours with each other, or when the result passes through two in a row)."""
    return MAX_ABS + kernels * float(vmax) * P_EPS[fmt]


# ---- lengths and limits -------------------------------------------------------------------------------------------------------------
def clamp(L, ncap):
    """the kernel's min(max(L, 0), Ncap)"""
    return min(max(int(L), 0), ncap)


def count(raw, padded):
    """n_b resp. m_b: the clamp of one count"""
    return min(max(int(raw), 0), padded)


def counts(raw, B, padded):
    """None (no vector: every sequence has the padded count) or a vector -> the clamped counts"""
    return [padded] * B if raw is None else [count(x, padded) for x in raw]


def row_limits(L, n, Nq, causal, W=0):
    """one sequence of L keys with n live rows of Nq -> (lo [Nq], c [Nq] int64, live [Nq] bool); dead rows have lo = c = 0"""
    lo, c = np.zeros(Nq, np.int64), np.zeros(Nq, np.int64)
    for i in range(n):
        c[i] = max(0, L - n + 1 + i) if causal else L
        lo[i] = min(max(0, L - n + 1 + i - W) if W else 0, c[i])
    return lo, c, np.arange(Nq) < n


# ---- references ---------------------------------------------------------------------------------------------------------------------
def expected_f64(q, k, v, lens, B, Hkv, G, Nq, causal, W=0, scale=None, softcap=0.0, sinks=None, nq=None):
    """q [B*Hkv*G, Nq, d], k/v [B*Hkv, Ncap, d] fp32 (16-bit-rounded), sinks [Hkv*G] or None, nq [B] or None
    -> (O [B*Hq, Nq, d], lse [B*Hq, Nq]) float64, row by row:
      soft-cap  t_j = softcap * tanh(s_j / softcap) on every logit s_j = q.k_j * scale, before the masks
      sinks     one extra key per row with the head's logit a (natural-log units, not scaled, not capped) and a zero V row; it
                takes part in the reference maximum; a = -inf: no sink for the head
    Dead rows and rows with neither key nor sink: zeros and -inf."""
    Hq, d, Ncap = Hkv * G, q.shape[2], k.shape[1]
    out = np.zeros(q.shape, np.float64)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b, n in enumerate(counts(nq, B, Nq)):
        lo, c, live = row_limits(clamp(lens[b], Ncap), n, Nq, causal, W)
        for h in range(Hq):
            r = b * Hq + h
            a = -np.inf if sinks is None else float(sinks[h])
            kk, vv = (x[b * Hkv + h // G].astype(np.float64) for x in (k, v))
            for i in np.flatnonzero(live):
                t = (kk[lo[i]:c[i]] @ q[r, i].astype(np.float64)) * sc
                if softcap:
                    t = softcap * np.tanh(t / softcap)
                m = max(t.max() if t.size else -np.inf, a)
                if m == -np.inf:
                    continue
                p = np.exp(t - m)
                den = p.sum() + np.exp(a - m)
                if t.size:
                    out[r, i] = (p / den) @ vv[lo[i]:c[i]]
                lse[r, i] = m + np.log(den)
    return out, lse


def expected(oracle, q, k, v, lens, B, Hkv, G, Nq, causal, W=0, scale=None):
    """The same shapes -> (O [B*Hq, Nq, d] fp32, lse [B*Hq, Nq] float64).  O from oracle.forward_cross (float64 accumulators) on
    k[:, lo:c], grouped by the distinct (lo, c) of a sequence's rows, lse from float64 numpy; a row without a key is zeros and
    -inf.  An implementation independent of expected_f64: tests/test_decode_inputs.py and tests/test_window_inputs.py hold one
    against the other."""
    Hq, d, Ncap = Hkv * G, q.shape[2], k.shape[1]
    out = np.zeros(q.shape, np.float32)
    lse = np.full(q.shape[:2], -np.inf, np.float64)
    sc = 1.0 / np.sqrt(d) if scale is None else float(scale)
    for b in range(B):
        qs = slice(b * Hq, (b + 1) * Hq)
        kb, vb = (np.repeat(x[b * Hkv:(b + 1) * Hkv], G, axis=0) for x in (k, v))   # K/V head of every query head
        los, cs, _ = row_limits(clamp(lens[b], Ncap), Nq, Nq, causal, W)
        rng = [(int(lo), int(c)) for lo, c in zip(los, cs)]
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


def uniform_expected(v, lens, B, Hkv, G, Nq, causal, W=0):
    """what scale 0 must give: every visible key weighs the same -- O is the mean of the V rows in [lo_i, c_i), lse = ln(their
    number)"""
    Hq, Ncap = Hkv * G, v.shape[1]
    out = np.zeros((B * Hq, Nq, v.shape[2]), np.float64)
    lse = np.full((B * Hq, Nq), -np.inf, np.float64)
    for b in range(B):
        los, cs, _ = row_limits(clamp(lens[b], Ncap), Nq, Nq, causal, W)
        for i, (lo, c) in enumerate(zip(los, cs)):
            if c:
                for h in range(Hq):
                    out[b * Hq + h, i] = v[b * Hkv + h // G, lo:c].astype(np.float64).mean(0)
                lse[b * Hq:(b + 1) * Hq, i] = np.log(c - lo)
    return out, lse


# ---- poison and scatter -------------------------------------------------------------------------------------------------------------
def poisoned(cache, lens, nq=1, W=0, nan=NAN16):
    """cache [B, Hkv, Ncap, d] (16-bit encodings, or fp8 codes with their NaN code) -> a copy with `nan` in every row at and past
    the sequence's (clamped) length and in every row below row 0's lower limit, which no row of the sequence sees"""
    out = np.array(cache)
    for b in range(out.shape[0]):
        L = clamp(lens[b], out.shape[2])
        out[b, :, L:] = nan
        out[b, :, :row_limits(L, nq, nq, False, W)[0][0]] = nan
    return out


def scatter(kc, vc, lens, ps, seed, nq=1, W=0, nan=NAN16, spare=3):
    """K and V caches [B, Hkv, Ncap, d] (16-bit encodings or fp8 codes) -> (K pool, V pool [num_pages, Hkv, ps, d], table
    [B, max_pages] int32).  Pages are dealt out by a seeded permutation of a pool with `spare` pages more than B * max_pages.  A page
    past the last live one, or wholly below row 0's lower limit, gets no pool page: its table entry holds garbage.  Every page no
    table names and every row outside [row 0's lower limit, length) holds `nan`.  A sequence whose raw length exceeds the capacity
    is full: all its entries are live and all its rows valid."""
    B, Hkv, Ncap, d = kc.shape
    max_pages = Ncap // ps
    assert max_pages * ps == Ncap
    num_pages = B * max_pages + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    pools = [np.full((num_pages, Hkv, ps, d), nan, kc.dtype) for _ in range(2)]
    table = np.empty((B, max_pages), np.int32)
    nxt = 0
    for b in range(B):
        L = clamp(lens[b], Ncap)
        sb = int(row_limits(L, nq, nq, False, W)[0][0])
        for pi in range(max_pages):
            if pi * ps >= L or (pi + 1) * ps <= sb:
                table[b, pi] = GARBAGE[pi % 2]
                continue
            page = int(perm[nxt])
            nxt += 1
            table[b, pi] = page
            r0, r1 = max(sb - pi * ps, 0), min(ps, L - pi * ps)   # the page's rows inside [start, L); the rest stay NaN
            for pool, src in zip(pools, (kc, vc)):
                pool[page, :, r0:r1] = src[b, :, pi * ps + r0:pi * ps + r1]
    return pools[0], pools[1], table


# ---- the check of a decode result -----------------------------------------------------------------------------------------------------
def check_decode(oracle, got, got_lse, want, want_lse, fmt, what):
    """got [B*Hq, Nq, d] and got_lse [B*Hq, Nq] (numpy) against expected()'s pair at the project's bounds: MAX_ABS and REL_L2 for O,
    2 * P_EPS absolute for lse; every figure is printed before it is judged.  Shared by the GPU tiers whose checks are exactly
    these (tests/test_gpu_kvcache.py, _paged.py and _window.py); the others add conditions of their own and keep their own."""
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    live = np.isfinite(want_lse)
    le = float(np.abs(got_lse[live] - want_lse[live]).max()) if live.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {MAX_ABS:.1e} {REL_L2[fmt]:.1e} {2 * P_EPS[fmt]:.2e})")
    assert np.isfinite(got).all(), what + ": O is not finite"
    assert not np.isnan(got_lse).any(), what + ": NaN in lse"
    assert ma <= MAX_ABS and rl <= REL_L2[fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    # rows without a key: exact zeros and -inf; every other row: a finite lse within the bound
    assert (got[~live] == 0.0).all(), what + ": a row without a key is not exactly zero"
    assert (got_lse[~live] == -np.inf).all(), what + ": a row without a key has lse != -inf"
    assert np.isfinite(got_lse[live]).all(), what
    assert le <= 2 * P_EPS[fmt], f"{what}: lse off by {le:.3e}"


# ---- host to device -----------------------------------------------------------------------------------------------------------------
def dev16(torch, bits, fmt):
    """uint16 encodings -> a device tensor of fp16 (fmt 0) or bf16 (fmt 1) with those bits"""
    return torch.from_numpy(np.array(bits, order="C").view(np.int16)).cuda().view(torch.bfloat16 if fmt else torch.float16)


def dev8(torch, codes):
    """e4m3fn codes -> a device tensor of torch.float8_e4m3fn with those bytes"""
    return torch.from_numpy(np.array(codes, dtype=np.uint8)).cuda().view(torch.float8_e4m3fn)
