"""Seeded inputs for tests/test_gpu_varlen_cache_fp8.py -- fa_forward_varlen_kvcache_fp8: the varlen prefill against an fp8 (OCP
e4m3fn) KV cache, contiguous [B,Hkv,Ncap,d] or paged [num_pages,Hkv,page_size,d] behind a block table, one byte per element, with one
fp32 scale per K/V head for K and for V -- on the conventions of tests/varlen_cache_inputs.py (geometry, page scatter, garbage in the
table entries nothing may read), tests/fp8_inputs.py (the format restated; the NaN code 0x7F as poison) and tests/varlen_inputs.py
(packed Q, NaN tail rows, the one check `problems`).  Seven WRONG kernels are restated by what they would read or compute.  Pure numpy;
nothing here touches a GPU (tests/test_varlen_cache_fp8_inputs.py asserts, without one, that no parity launch could pass on a wrong
kernel).

Semantics, from include/fa_mi355.h: fa_forward_varlen_kvcache's, with k8, v8 the decoded codes: the logits are
scale * k_scale[hkv] * q.k8 (soft-cap, masks and sinks after that; the sinks take neither scale), O = v_scale[hkv] * softmax.v8, and lse
is that of the scaled logits.
"""
import functools

import numpy as np

import common_inputs as cm
import fp8_inputs as f8
import varlen_cache_inputs as ci
import varlen_inputs as vi
import varlen_logit_inputs as li

NAN8 = f8.NAN_CODES[0]
NCAP = ci.NCAP
PAGE_SIZES = ci.PAGE_SIZES
BATCHES = ci.BATCHES
# one scale per K/V head, all distinct, none 1, K's and V's different; powers of two are avoided on purpose except one: the decode
# tests' habit, so that a scale is not hidden by an exponent shift alone
K_SCALES = (0.75, 1.5, 0.625)
V_SCALES = (1.25, 0.5, 1.75)

# (batch, Hkv, G, d, fmt, causal, out_f32, scale, W, softcap on, sinks on); scale None = 1/sqrt(d)
CASES = (
    ("chunk", 2, 2, 64, 0, 1, 1, None, 0, 0, 0),
    ("chunk", 1, 4, 128, 1, 1, 0, None, 0, 0, 0),
    ("short", 3, 1, 128, 0, 0, 1, None, 0, 0, 0),
    ("short", 2, 2, 64, 1, 1, 0, None, 0, 0, 0),
    ("chunk", 2, 2, 128, 0, 1, 1, -0.125, 0, 0, 0),      # a negative scale
    ("chunk", 2, 2, 128, 0, 1, 1, None, 100, 0, 0),      # the window crosses the prefix boundary; pages below lo_0 are freed
    ("chunk", 1, 4, 64, 1, 1, 0, None, 17, 1, 0),
    ("chunk", 3, 1, 64, 0, 0, 1, None, 1, 0, 1),
    ("short", 2, 2, 128, 1, 1, 1, None, 400, 1, 1),
    ("chunk", 2, 2, 64, 0, 1, 0, None, 0, 1, 0),         # the cap alone
    ("chunk", 2, 2, 128, 1, 0, 1, None, 0, 0, 1),        # the sinks alone
    ("short", 3, 1, 64, 0, 1, 1, -0.125, 100, 1, 1),     # a negative scale with everything on: tanh is odd
)

case_id = ci.case_id
lo0_of = ci.lo0_of


def scales_for(Hkv):
    return np.array(K_SCALES[:Hkv], np.float32), np.array(V_SCALES[:Hkv], np.float32)


def packed8(lens, H, d, scales, seed, tail=vi.TAIL):
    """codes (total + tail, H, d) uint8: f8.encode(x / scale[h]) of N(0,1) rows x for sum(lens) tokens, then `tail` rows of the NaN code"""
    n = int(sum(lens))
    codes = np.full((n + tail, H, d), NAN8, np.uint8)
    x = np.random.default_rng(seed).standard_normal((n, H, d)).astype(np.float32)
    codes[:n] = f8.encode(x / np.asarray(scales, np.float32)[None, :, None])
    return codes


def cache_of(k8, cu_k, lq, lk, W, ncap=NCAP):
    """packed codes (total, Hkv, d) -> the contiguous cache [B,Hkv,ncap,d] with the NaN code in every row outside [lo_0, Lk)"""
    out = np.full((len(lk), k8.shape[1], ncap, k8.shape[2]), NAN8, np.uint8)
    for b, lo in enumerate(lo0_of(lq, lk, W)):
        out[b, :, lo:lk[b]] = k8[cu_k[b] + lo:cu_k[b + 1]].transpose(1, 0, 2)
    return out


@functools.lru_cache(maxsize=None)
def make(case):
    """one parity case -> dict as ci.make's: k, v are the DECODED codes of the gathered keys (packed, NaN tail), k8, v8 their codes,
    kc, vc the contiguous cache of codes, k_scale, v_scale [Hkv] float32"""
    batch, Hkv, G, d, fmt, causal, f32, scale, W, cap, snk = case
    lq, lk = BATCHES[batch]
    seed = 8000 + CASES.index(case) if case in CASES else 7999
    q, qb = vi.packed(lq, Hkv * G, d, fmt, seed)
    ks, vs = scales_for(Hkv)
    k8, v8 = packed8(lk, Hkv, d, ks, seed + 100), packed8(lk, Hkv, d, vs, seed + 200)
    cu_k = vi.cu_of(lk)
    return dict(q=q, qb=qb, k=f8.decode(k8), v=f8.decode(v8), k8=k8, v8=v8, cu_q=vi.cu_of(lq), cu_k=cu_k, Hkv=Hkv, G=G, d=d, fmt=fmt,
                causal=bool(causal), f32=bool(f32), scale=(1.0 / np.sqrt(d)) if scale is None else float(scale), lq=lq, lk=lk, W=W,
                softcap=li.SOFTCAP if cap else 0.0, sinks=li.sinks_for(Hkv * G) if snk else None, k_scale=ks, v_scale=vs,
                kc=cache_of(k8, cu_k, lq, lk, W), vc=cache_of(v8, cu_k, lq, lk, W), lens=np.array(lk, np.int32))


def scatter(kc, vc, lk, lo0, ps, seed, spare=ci.SPARE):
    """ci.scatter on caches of codes: the NaN code where it puts cm.NAN16 (every unnamed page, every row outside [lo_0, Lk)), cm.GARBAGE
    in the table entries nothing may read"""
    wide = [np.where(x == NAN8, cm.NAN16, x.astype(np.uint16)).astype(np.uint16) for x in (kc, vc)]
    kp, vp, table = ci.scatter(wide[0], wide[1], lk, lo0, ps, seed, spare)
    return tuple(np.where(p == cm.NAN16, NAN8, p).astype(np.uint8) for p in (kp, vp)) + (table,)


@functools.lru_cache(maxsize=None)
def paged(case, ps):
    """the case's cache scattered into pages of ps keys -> (K pool, V pool, table), read-only"""
    c = make(case)
    out = scatter(c["kc"], c["vc"], c["lk"], lo0_of(c["lq"], c["lk"], c["W"]), ps, seed=9000 + 13 * ps)
    for a in out:
        a.setflags(write=False)
    return out


def reference_f64(c, k_scale=None, v_scale=None, base=None):
    """li.run_f64 per K/V head on the decoded codes with scale * k_scale[h], O multiplied by v_scale[h]"""
    ks = c["k_scale"] if k_scale is None else k_scale
    vs = c["v_scale"] if v_scale is None else v_scale
    G = c["G"]
    outs, lses = [], []
    for h in range(c["Hkv"]):
        hq = slice(h * G, (h + 1) * G)
        sub = dict(c, q=c["q"][:, hq], k=c["k"][:, h:h + 1], v=c["v"][:, h:h + 1], Hkv=1, scale=c["scale"] * float(ks[h]),
                   sinks=None if c["sinks"] is None else c["sinks"][hq])
        o, l = li.run_f64(sub, base=base)
        own = vi.owned(c["cu_q"], o.shape[0])
        o[own] *= float(vs[h])
        outs.append(o), lses.append(l)
    return np.concatenate(outs, axis=1), np.concatenate(lses, axis=0)


@functools.lru_cache(maxsize=None)
def expected(case):
    """the reference of the parity tests; read-only"""
    out, lse = reference_f64(make(case))
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


# ---- the kernel's reads and arithmetic restated, and seven wrong ones ------------------------------------------------------------------
WRONG = ("no_k_scale", "no_v_scale", "scales_swapped", "scale_by_hq", "pitch16", "halves_swapped", "v_scale_on_lse")


def gather(kp, vp, table, lens, Hkv, ps, wrong=None):
    """what a kernel reads: per sequence (K, V) float32 [Lk, Hkv, d] through the table, byte addresses taken in the flat pool as the
    hardware would.  A live entry outside [0, num_pages) is a page of zeros; an address outside the pool reads NaN.  wrong --
      pitch16         the 16-bit row pitch on the byte cache: row j of a page-head block read at byte 2 * j * d of it
      halves_swapped  the two widened halves of a 16-byte load swapped: elements 16 c + (0..7) and 16 c + (8..15) of a row exchanged"""
    num_pages, _, _, d = kp.shape
    flat = [f8.decode(p).reshape(-1) for p in (kp, vp)]
    tbl = np.asarray(table)
    col = np.arange(d)
    if wrong == "halves_swapped":
        col = col ^ 8
    out = []
    for b in range(len(lens)):
        Lk = cm.clamp(lens[b], tbl.shape[1] * ps)
        j = np.arange(Lk)
        page = tbl[b, j // ps].astype(np.int64)
        row = j % ps
        ok = (page >= 0) & (page < num_pages)
        seq = []
        for f in flat:
            rows = np.empty((Lk, Hkv, d), np.float32)
            for h in range(Hkv):
                at = ((page * Hkv + h) * ps * d + row * d * (2 if wrong == "pitch16" else 1))[:, None] + col[None, :]
                inside = ok[:, None] & (at < f.size)
                rows[:, h] = np.where(inside, f[np.where(inside, at, 0)], np.where(ok[:, None], np.nan, 0.0))
            seq.append(rows)
        out.append(tuple(seq))
    return out


def attend(c, seqs, wrong=None, base=None):
    """the entry in float64 on per-sequence keys `seqs` = gather()'s result, NaN-aware as ci.attend_f64 (which it calls, query head by
    query head, with that head's factor).  wrong --
      no_k_scale      k_scale dropped from the logits
      no_v_scale      v_scale dropped from O
      scales_swapped  v_scale in the logits and k_scale on O
      scale_by_hq     both scales indexed by the QUERY head: index hq of a vector of Hkv entries (past its end: not a number)
      v_scale_on_lse  the epilogue's factor applied to both results: lse multiplied by v_scale too"""
    Hkv, G = c["Hkv"], c["G"]
    ks, vs = c["k_scale"].astype(np.float64), c["v_scale"].astype(np.float64)
    if wrong == "scales_swapped":
        ks, vs = vs, ks
    own = vi.owned(c["cu_q"], c["q"].shape[0])
    outs, lses = [], []
    for hq in range(Hkv * G):
        h = hq // G
        at = hq if wrong == "scale_by_hq" else h
        fk = 1.0 if wrong == "no_k_scale" else (ks[at] if at < Hkv else np.nan)
        fv = 1.0 if wrong == "no_v_scale" else (vs[at] if at < Hkv else np.nan)
        sub = dict(c, q=c["q"][:, hq:hq + 1], Hkv=1, G=1, scale=c["scale"] * (1.0 if np.isnan(fk) else fk),
                   sinks=None if c["sinks"] is None else c["sinks"][hq:hq + 1])
        o, l = ci.attend_f64(sub, [(kk[:, h:h + 1], vv[:, h:h + 1]) for kk, vv in seqs], base=base)
        o[own] *= fv
        if np.isnan(fk):
            o[own], l[:, own] = np.nan, np.nan
        if wrong == "v_scale_on_lse":
            l[:, own] *= fv
        outs.append(o), lses.append(l)
    return np.concatenate(outs, axis=1), np.concatenate(lses, axis=0)


def run_paged(case, ps, wrong=None, base=None):
    """a (wrong) kernel on the case's pools of page size ps"""
    c = make(case)
    kp, vp, table = paged(case, ps)
    return attend(c, gather(kp, vp, table, c["lens"], c["Hkv"], ps, wrong if wrong in ("pitch16", "halves_swapped") else None),
                  wrong, base)
