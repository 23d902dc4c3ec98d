"""Seeded inputs for tests/test_gpu_varlen.py -- fa_forward_varlen (variable-length packed prefill: cu_seqlens, grouped-query heads, a
causal mask aligned to the end of each sequence's keys, lse) -- with the entry restated in float64 numpy, five WRONG restatements of
it, the one check both tiers apply, and the block-slot arithmetic of the kernel.  Pure numpy; nothing here touches a GPU
(tests/test_varlen_inputs.py asserts, without one, that no parity launch could pass on a wrong kernel).

Semantics, from include/fa_mi355.h.  q (total_q, Hq, d), k and v (total_k, Hkv, d), Hq = Hkv * G, query head hq uses K/V head hq // G.
For sequence b: s = clamp(cu[b], 0, total), e = clamp(cu[b+1], s, total), for q and k separately; Lq = e_q - s_q, Lk = e_k - s_k.  Row i
of the sequence sees the keys [0, c_i) of it: c_i = Lk without the mask, max(0, Lk - Lq + 1 + i) with it.  A row without a key is O = 0
and lse = -inf; lse = ln sum_j exp(scale q.k_j) (natural log), laid out (Hq, total_q).  Rows of no sequence are not written.
"""
import functools

import numpy as np

import common_inputs as cm

BM = 128                 # query rows per workgroup = rows per block slot (csrc/fa_fwd_varlen.hip)
TAIL = 8                 # rows of no sequence behind cu[B], holding cm.NAN16 in Q, K and V
POISON = -768.0          # what O and lse hold before a launch (exact in fp16, bf16 and fp32)

# Lengths: any workgroup height in {64,128,256} and the 64-key tile have a boundary inside some sequence
LQ = (1, 63, 65, 0, 129, 257)
LK2 = (1, 200, 65, 5, 70, 300)   # Lk > Lq, Lk < Lq (rows i < Lq - Lk see no key), Lq = 0 with Lk > 0
BATCHES = {"self": (LQ, LQ), "cross": (LQ, LK2), "one": ((64,), (64,))}

# (batch, Hkv, G, d, fmt, causal, out_f32, scale); scale None = 1/sqrt(d)
CASES = (
    ("self", 2, 2, 64, 0, 0, 1, None),
    ("self", 1, 4, 128, 1, 1, 0, None),
    ("self", 3, 1, 128, 0, 1, 1, None),
    ("self", 2, 2, 64, 1, 0, 0, None),
    ("cross", 2, 2, 128, 0, 1, 1, None),
    ("cross", 1, 4, 64, 1, 0, 1, None),
    ("cross", 3, 1, 64, 0, 1, 0, None),
    ("cross", 1, 4, 128, 1, 1, 1, None),
    ("cross", 2, 2, 128, 0, 0, 0, None),
    ("cross", 2, 2, 64, 0, 1, 1, None),
    ("one", 1, 4, 64, 0, 1, 1, None),
    ("one", 3, 1, 128, 1, 0, 0, None),
    ("self", 2, 2, 64, 0, 1, 1, -0.125),
)


def case_id(c):
    batch, Hkv, G, d, fmt, causal, f32, scale = c
    return f"{batch}-Hkv{Hkv}G{G}-d{d}-{cm.FMT_NAME[fmt]}-{'causal' if causal else 'full'}-{'f32' if f32 else 'o16'}" + \
        ("" if scale is None else f"-scale{scale}")


# ---- 16-bit formats in numpy -----------------------------------------------------------------------------------------------------------
def encode16(x, fmt):
    """float32 -> uint16 encodings, round to nearest even (finite inputs)"""
    x = np.ascontiguousarray(x, np.float32)
    if fmt == 0:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def decode16(u, fmt):
    u = np.ascontiguousarray(u, np.uint16)
    if fmt == 0:
        return u.view(np.float16).astype(np.float32)
    return (u.astype(np.uint32) << 16).view(np.float32)


# ---- packing ---------------------------------------------------------------------------------------------------------------------------
def cu_of(lens):
    """lengths -> the B+1 prefix sums, int32"""
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def bounds(cu, total):
    """the entry's clamp: [(s, e)] per sequence"""
    out = []
    for b in range(len(cu) - 1):
        s = min(max(int(cu[b]), 0), total)
        out.append((s, min(max(int(cu[b + 1]), s), total)))
    return out


def owned(cu, total):
    """[total] bool: the rows that belong to a sequence"""
    m = np.zeros(total, bool)
    for s, e in bounds(cu, total):
        m[s:e] = True
    return m


def packed(lens, H, d, fmt, seed, tail=TAIL):
    """(values (total, H, d) float32, encodings uint16): 16-bit-rounded N(0,1) rows for sum(lens) tokens, then `tail` rows of NaN"""
    n = int(sum(lens))
    bits = np.full((n + tail, H, d), cm.NAN16, np.uint16)
    bits[:n] = encode16(np.random.default_rng(seed).standard_normal((n, H, d)).astype(np.float32), fmt)
    return decode16(bits, fmt), bits


@functools.lru_cache(maxsize=None)
def make(case):
    """one parity case -> dict(q, k, v values; qb, kb, vb encodings; cu_q, cu_k; the case's fields)"""
    batch, Hkv, G, d, fmt, causal, f32, scale = case
    lq, lk = BATCHES[batch]
    seed = 1000 + CASES.index(case) if case in CASES else 999
    q, qb = packed(lq, Hkv * G, d, fmt, seed)
    k, kb = packed(lk, Hkv, d, fmt, seed + 100)
    v, vb = packed(lk, Hkv, d, fmt, seed + 200)
    return dict(q=q, k=k, v=v, qb=qb, kb=kb, vb=vb, cu_q=cu_of(lq), cu_k=cu_of(lk), Hkv=Hkv, G=G, d=d, fmt=fmt, causal=bool(causal),
                f32=bool(f32), scale=(1.0 / np.sqrt(d)) if scale is None else float(scale), lq=lq, lk=lk)


# ---- the entry in float64, and five wrong ones -----------------------------------------------------------------------------------------
WRONG = ("start", "next_row", "head_mod", "drop_tail", "log2")


def varlen_f64(q, k, v, cu_q, cu_k, Hkv, G, causal, scale, wrong=None, base=None):
    """-> (O (total_q, Hq, d), lse (Hq, total_q)) float64.  Rows of no sequence hold `base` = (O value, lse value), default (0, -inf).
    wrong: None, or one of WRONG --
      start      the causal mask aligned to the START of the keys, c_i = min(i + 1, Lk)
      next_row   every sequence reads one key row too many (the next sequence's first row, or the tail)
      head_mod   query head hq reads K/V head hq % Hkv
      drop_tail  the last partial block of BM query rows of a sequence is not computed: it keeps `base`
      log2       lse in log2 units"""
    total_q, Hq, d = q.shape
    total_k = k.shape[0]
    assert Hq == Hkv * G and wrong in (None,) + WRONG
    o0, l0 = (0.0, -np.inf) if base is None else base
    out = np.full(q.shape, o0, np.float64)
    lse = np.full((Hq, total_q), l0, np.float64)
    for (sq, eq), (sk, ek) in zip(bounds(cu_q, total_q), bounds(cu_k, total_k)):
        Lq, Lk = eq - sq, ek - sk
        if wrong == "next_row":
            Lk = min(Lk + 1, total_k - sk)
        done = Lq - Lq % BM if wrong == "drop_tail" else Lq
        for i in range(done):
            c = Lk if not causal else (min(i + 1, Lk) if wrong == "start" else max(0, Lk - Lq + 1 + i))
            for hq in range(Hq):
                hk = hq % Hkv if wrong == "head_mod" else hq // G
                out[sq + i, hq] = 0.0
                lse[hq, sq + i] = -np.inf
                if c == 0:
                    continue
                t = (k[sk:sk + c, hk].astype(np.float64) @ q[sq + i, hq].astype(np.float64)) * scale
                m = t.max()
                p = np.exp(t - m)
                out[sq + i, hq] = (p / p.sum()) @ v[sk:sk + c, hk].astype(np.float64)
                lse[hq, sq + i] = (m + np.log(p.sum())) * (np.log2(np.e) if wrong == "log2" else 1.0)
    return out, lse


def expected_varlen_f64(q, k, v, cu_q, cu_k, Hkv, G, causal, scale):
    """the reference of the parity tests"""
    return varlen_f64(q, k, v, cu_q, cu_k, Hkv, G, causal, scale)


@functools.lru_cache(maxsize=None)
def expected(case):
    c = make(case)
    return expected_varlen_f64(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["Hkv"], c["G"], c["causal"], c["scale"])


# ---- the one check of a result ---------------------------------------------------------------------------------------------------------
def problems(got, got_lse, want, want_lse, own, fmt, base=(POISON, POISON)):
    """got (total_q, Hq, d), got_lse (Hq, total_q) against the reference at the project's bounds (cm.MAX_ABS and cm.REL_L2[fmt] for O over
    the rows of a sequence, 2 * cm.P_EPS[fmt] absolute for lse), rows without a key exactly 0 and -inf, rows of no sequence still `base`,
    nothing NaN -> a list of findings, each naming a row; empty: the result passes."""
    got, got_lse = np.asarray(got, np.float64), np.asarray(got_lse, np.float64)
    out = []

    def first(mask_rows):
        return int(np.flatnonzero(mask_rows)[0])

    bad = np.isnan(got).any(axis=(1, 2)) | np.isnan(got_lse).any(axis=0)
    if bad.any():
        out.append(f"NaN in row {first(bad)}")
    if (~own).any():
        bad = ~own & ((got != base[0]).any(axis=(1, 2)) | (got_lse != base[1]).any(axis=0))
        if bad.any():
            out.append(f"row {first(bad)} of no sequence was written")
    nokey = own[None, :] & ~np.isfinite(want_lse)                # (Hq, total_q)
    bad = (nokey & (got_lse != -np.inf)).any(axis=0) | (nokey.T[:, :, None] & (got != 0.0)).any(axis=(1, 2))
    if bad.any():
        out.append(f"row {first(bad)} without a key is not exactly 0 / -inf")
    live = own[None, :] & np.isfinite(want_lse)
    with np.errstate(invalid="ignore"):
        err = np.where(live, np.abs(got_lse - np.where(live, want_lse, 0.0)), 0.0)
    err = np.where(np.isnan(err), np.inf, err)
    if err.max(initial=0.0) > 2 * cm.P_EPS[fmt]:
        out.append(f"lse of row {first((err > 2 * cm.P_EPS[fmt]).any(axis=0))} off by {err.max():.3e} (bound {2 * cm.P_EPS[fmt]:.2e})")
    diff = np.where(np.isnan(got[own]), np.inf, np.abs(got[own] - want[own]))
    if diff.size:
        ma = float(diff.max())
        with np.errstate(over="ignore", invalid="ignore"):
            rl = float(np.sqrt((diff ** 2).sum() / max((want[own] ** 2).sum(), 1e-300)))
        if ma > cm.MAX_ABS:
            out.append(f"O of row {int(np.flatnonzero(own)[int(np.argmax(diff.max(axis=(1, 2))))])}: max_abs {ma:.3e} > {cm.MAX_ABS:.1e}")
        if not rl <= cm.REL_L2[fmt]:
            out.append(f"O: rel_l2 {rl:.3e} > {cm.REL_L2[fmt]:.1e} (worst row "
                       f"{int(np.flatnonzero(own)[int(np.argmax(diff.max(axis=(1, 2))))])})")
    return out


def figures(got, got_lse, want, want_lse, own):
    """(max_abs, rel_l2 of O over the rows of a sequence, largest lse error over the rows with a key), for printing"""
    got, got_lse = np.asarray(got, np.float64), np.asarray(got_lse, np.float64)
    diff = np.abs(got[own] - want[own])
    live = own[None, :] & np.isfinite(want_lse)
    le = float(np.abs(got_lse[live] - want_lse[live]).max()) if live.any() else 0.0
    return (float(diff.max(initial=0.0)), float(np.sqrt((diff ** 2).sum() / max((want[own] ** 2).sum(), 1e-300))), le)


# ---- the block slots of the kernel -----------------------------------------------------------------------------------------------------
def first_slot(cu_q, total_q, b, bm=BM):
    """first_b = floor(s_q(b) / bm) + b: sequence b owns the slots [first_b, first_{b+1}); b = B gives the end of the last"""
    return min(max(int(cu_q[b]), 0), total_q) // bm + b


def num_slots(total_q, B, bm=BM):
    """slots per query head: host integers only"""
    return total_q // bm + B
