"""Seeded inputs for tests/test_gpu_varlen_cache.py -- fa_forward_varlen_kvcache: the variable-length prefill with its K/V rows taken
from the KV cache, contiguous [B,Hkv,Ncap,d] or paged [num_pages,Hkv,page_size,d] behind a block table -- on the conventions of
tests/varlen_inputs.py (packed Q, NaN tail rows, poison, the one check `problems`) and tests/common_inputs.py (the page scatter: a
seeded permutation, spare pages, NaN where no visible key lies, garbage in table entries nothing may read).  The reference gathers
each sequence's keys and calls tests/varlen_logit_inputs.py's float64 entry; six WRONG kernels are restated by the address they would
read the laid-out pools at.  Pure numpy; nothing here touches a GPU (tests/test_varlen_cache_inputs.py asserts, without one, that no
parity launch could pass on a wrong kernel).

Semantics, from include/fa_mi355.h.  Lq_b from cu_seqlens_q; Lk_b = clamp(seqlens_k[b], 0, Ncap) counts the chunk's own tokens; key j
of sequence b is cache row j, paged: row j % page_size of page table[b][j // page_size].  Row i sees [lo_i, c_i): c_i = Lk, or
max(0, Lk - Lq + 1 + i) under causal; lo_i = max(0, Lk - Lq + 1 + i - W) under a window, else 0.  Pages wholly below
lo_0 = max(0, Lk - Lq + 1 - W) may be freed; table entries at or past ceil(Lk / page_size) are never read; a live entry outside
[0, num_pages) reads as a page of zeros.
"""
import functools

import numpy as np

import common_inputs as cm
import varlen_inputs as vi
import varlen_logit_inputs as li

NCAP = 640
PAGE_SIZES = (16, 32, 64, 128)       # below, at and above the 64-key tile
SPARE = 3
LQ = vi.LQ                           # chunk lengths (1, 63, 65, 0, 129, 257)
PREFIX = (0, 200, 15, 5, 70, 300)    # keys already cached; Lk = prefix + Lq
# "chunk": every sequence is a prefix plus its chunk.  "short": Lk = 0 under a live row, Lk < Lq twice (rows i < Lq - Lk see no key
# under causal), keys under no row (Lq = 0), and one long sequence
BATCHES = {"chunk": (LQ, tuple(p + n for p, n in zip(PREFIX, LQ))), "short": (LQ, (0, 40, 80, 3, 100, 557))}
WINDOWS = (0, 1, 17, 64, 100, 400)

# (batch, Hkv, G, d, fmt, causal, out_f32, scale, W, softcap on, sinks on); scale None = 1/sqrt(d)
CASES = (
    ("chunk", 2, 2, 64, 0, 1, 1, None, 0, 0, 0),
    ("chunk", 1, 4, 128, 1, 1, 0, None, 0, 0, 0),
    ("chunk", 3, 1, 128, 0, 0, 1, None, 0, 0, 0),
    ("short", 2, 2, 128, 0, 1, 0, None, 0, 0, 0),
    ("short", 1, 4, 64, 1, 0, 1, None, 0, 0, 0),
    ("chunk", 2, 2, 64, 0, 1, 1, -0.125, 0, 0, 0),       # a negative scale
    ("chunk", 2, 2, 128, 0, 1, 1, None, 100, 0, 0),      # the window crosses the prefix boundary; pages below lo_0 are freed
    ("chunk", 1, 4, 64, 1, 1, 0, None, 17, 1, 0),
    ("chunk", 3, 1, 64, 0, 0, 1, None, 64, 0, 1),
    ("chunk", 2, 2, 128, 1, 1, 1, None, 1, 1, 1),
    ("chunk", 3, 1, 128, 0, 1, 0, None, 400, 1, 1),
    ("short", 2, 2, 64, 0, 1, 1, None, 100, 0, 1),
    ("short", 1, 4, 128, 1, 0, 0, None, 17, 1, 0),
    ("short", 3, 1, 64, 1, 1, 1, None, 64, 1, 1),
    ("chunk", 2, 2, 64, 0, 1, 1, None, 0, 1, 0),         # the cap alone
    ("chunk", 2, 2, 128, 1, 0, 0, None, 0, 0, 1),        # the sinks alone
    ("chunk", 1, 4, 64, 0, 1, 1, -0.125, 100, 1, 1),     # a negative scale: tanh is odd
)

case_id = li.case_id


def lo0_of(lq, lk, W):
    """per sequence the first key any of its rows sees: lo of row 0, or Lk for a sequence without a row (nothing of it is visible)"""
    return [Lk if Lq == 0 else (max(0, Lk - Lq + 1 - W) if W else 0) for Lq, Lk in zip(lq, lk)]


@functools.lru_cache(maxsize=None)
def make(case):
    """one parity case -> dict as li.make's, with the packed k, v, kb, vb the GATHERED keys (what fa_forward_varlen is given), plus
    kc, vc: the contiguous cache [B,Hkv,NCAP,d] as encodings with cm.NAN16 in every row outside [lo_0, Lk); lens: seqlens_k"""
    batch, Hkv, G, d, fmt, causal, f32, scale, W, cap, snk = case
    lq, lk = BATCHES[batch]
    seed = 5000 + CASES.index(case) if case in CASES else 4999
    q, qb = vi.packed(lq, Hkv * G, d, fmt, seed)
    k, kb = vi.packed(lk, Hkv, d, fmt, seed + 100)
    v, vb = vi.packed(lk, Hkv, d, fmt, seed + 200)
    cu_k = vi.cu_of(lk)
    kc, vc = (np.full((len(lk), Hkv, NCAP, d), cm.NAN16, np.uint16) for _ in range(2))
    for b, lo in enumerate(lo0_of(lq, lk, W)):
        for cache, bits in ((kc, kb), (vc, vb)):
            cache[b, :, lo:lk[b]] = bits[cu_k[b] + lo:cu_k[b + 1]].transpose(1, 0, 2)
    return dict(q=q, k=k, v=v, qb=qb, kb=kb, vb=vb, cu_q=vi.cu_of(lq), cu_k=cu_k, Hkv=Hkv, G=G, d=d, fmt=fmt, causal=bool(causal),
                f32=bool(f32), scale=(1.0 / np.sqrt(d)) if scale is None else float(scale), lq=lq, lk=lk, W=W,
                softcap=li.SOFTCAP if cap else 0.0, sinks=li.sinks_for(Hkv * G) if snk else None, kc=kc, vc=vc,
                lens=np.array(lk, np.int32))


def scatter(kc, vc, lk, lo0, ps, seed, spare=SPARE):
    """cm.scatter with a first visible key PER SEQUENCE: caches [B,Hkv,Ncap,d] (encodings) -> (K pool, V pool [num_pages,Hkv,ps,d],
    table [B,max_pages] int32).  Pages are dealt out by a seeded permutation of a pool with `spare` pages more than B * max_pages.  A
    page past the last live one, or wholly below lo_0, gets no pool page: its table entry holds garbage.  Every page no table names
    and every row outside [lo_0, Lk) holds cm.NAN16."""
    B, Hkv, Ncap, d = kc.shape
    max_pages = Ncap // ps
    assert max_pages * ps == Ncap
    num_pages = B * max_pages + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    pools = [np.full((num_pages, Hkv, ps, d), cm.NAN16, kc.dtype) for _ in range(2)]
    table = np.empty((B, max_pages), np.int32)
    nxt = 0
    for b in range(B):
        L, sb = cm.clamp(lk[b], Ncap), int(lo0[b])
        for pi in range(max_pages):
            if pi * ps >= L or (pi + 1) * ps <= sb:
                table[b, pi] = cm.GARBAGE[pi % 2]
                continue
            page = int(perm[nxt])
            nxt += 1
            table[b, pi] = page
            r0, r1 = max(sb - pi * ps, 0), min(ps, L - pi * ps)
            for pool, src in zip(pools, (kc, vc)):
                pool[page, :, r0:r1] = src[b, :, pi * ps + r0:pi * ps + r1]
    return pools[0], pools[1], table


@functools.lru_cache(maxsize=None)
def paged(case, ps):
    """the case's cache scattered into pages of ps keys -> (K pool, V pool, table), read-only"""
    c = make(case)
    out = scatter(c["kc"], c["vc"], c["lk"], lo0_of(c["lq"], c["lk"], c["W"]), ps, seed=7000 + 13 * ps)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(case):
    """the reference of the parity tests: each sequence's keys gathered (make()'s k, v), through li.varlen_logits_f64; read-only"""
    out, lse = li.run_f64(make(case))
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


# ---- the kernel's addressing restated, and six wrong ones ------------------------------------------------------------------------------
WRONG = ("len_excl", "page_pitch", "row_in_page", "tile_one_page", "head_in_page", "lo_prefix")


def gather(kp, vp, table, lens, lq, Hkv, ps, fmt, wrong=None):
    """what a kernel reads: per sequence (K, V) float32 [Lk, Hkv, d] through the table, element addresses taken in the flat pool as
    the hardware would.  A live entry outside [0, num_pages) is a page of zeros; an address outside the pool reads NaN.  wrong --
      len_excl       Lk taken without the chunk's own tokens (seqlens_k - Lq)
      page_pitch     the table row of sequence b found at b * (max_pages + 1)
      row_in_page    row j % 64 of the page instead of j % page_size
      tile_one_page  a whole 64-key tile taken from the page of its first row (rows counted on from that page's start)
      head_in_page   the head index outside the page block: element ((page * ps + row) * Hkv + h) * d"""
    num_pages, _, _, d = kp.shape
    flat = [decode_nan(p, fmt).reshape(-1, d) for p in (kp, vp)]
    tbl = np.asarray(table).reshape(-1)
    max_pages = table.shape[1]
    out = []
    for b in range(len(lens)):
        Lk = cm.clamp(lens[b], max_pages * ps)
        if wrong == "len_excl":
            Lk = max(Lk - lq[b], 0)
        j = np.arange(Lk)
        first = j // cm.TILE * cm.TILE if wrong == "tile_one_page" else j
        pi = first // ps
        row = j - pi * ps if wrong == "tile_one_page" else (j % cm.TILE if wrong == "row_in_page" else j % ps)
        at = b * (max_pages + 1 if wrong == "page_pitch" else max_pages) + pi
        page = np.where(at < tbl.size, tbl[np.minimum(at, tbl.size - 1)], -1).astype(np.int64)
        ok = (page >= 0) & (page < num_pages)
        seq = []
        for f in flat:
            rows = np.empty((Lk, Hkv, d), np.float32)
            for h in range(Hkv):
                idx = (page * ps + row) * Hkv + h if wrong == "head_in_page" else (page * Hkv + h) * ps + row
                inside = ok & (idx >= 0) & (idx < f.shape[0])
                rows[:, h] = np.where(inside[:, None], f[np.where(inside, idx, 0)], np.where(ok[:, None], np.nan, 0.0))
            seq.append(rows)
        out.append(tuple(seq))
    return out


def decode_nan(bits, fmt):
    """vi.decode16 that keeps cm.NAN16 a NaN"""
    return vi.decode16(np.ascontiguousarray(bits), fmt)


def attend_f64(c, seqs, wrong=None, base=None):
    """the entry in float64 on per-sequence keys `seqs` = gather()'s result, NaN-aware: a row that SEES a key with a NaN in K or V is NaN;
    what it does not see is not touched.  wrong = "lo_prefix": the window restarted at the prefix boundary, lo_i raised to Lk - Lq for
    every row whose window would reach below it.  -> (O (total_q, Hq, d), lse (Hq, total_q)); rows of no sequence hold `base`"""
    q, Hkv, G, W, softcap, sinks, scale = c["q"], c["Hkv"], c["G"], c["W"], c["softcap"], c["sinks"], c["scale"]
    total_q, Hq, d = q.shape
    o0, l0 = (0.0, -np.inf) if base is None else base
    out = np.full(q.shape, o0, np.float64)
    lse = np.full((Hq, total_q), l0, np.float64)
    for (sq, eq), (kk, vv) in zip(vi.bounds(c["cu_q"], total_q), seqs):
        Lq, Lk = eq - sq, kk.shape[0]
        if Lq == 0:
            continue
        lo, lim = li.limits(Lq, Lk, c["causal"], W)
        if wrong == "lo_prefix" and W:
            lo = np.maximum(lo, max(Lk - Lq, 0))
        j = np.arange(Lk, dtype=np.int64)
        vis = (j[None, :] >= lo[:, None]) & (j[None, :] < lim[:, None])
        for hq in range(Hq):
            hk = hq // G
            kh, vh = kk[:, hk].astype(np.float64), vv[:, hk].astype(np.float64)
            nan_key = np.isnan(kh).any(axis=1) | np.isnan(vh).any(axis=1)
            s = (q[sq:eq, hq].astype(np.float64) @ np.nan_to_num(kh).T) * scale
            if softcap > 0.0:
                s = softcap * np.tanh(s / softcap)
            t = np.where(vis, s, -np.inf)
            a = -np.inf if sinks is None else float(sinks[hq])
            m = np.maximum(t.max(axis=1, initial=-np.inf), a)
            none = ~np.isfinite(m)
            ms = np.where(none, 0.0, m)
            p = np.exp(t - ms[:, None])
            den = p.sum(axis=1) + (np.exp(a - ms) if np.isfinite(a) else 0.0)
            o = np.where(none[:, None], 0.0, (p @ np.nan_to_num(vh)) / np.where(none, 1.0, den)[:, None])
            with np.errstate(divide="ignore"):
                l = np.where(none, -np.inf, ms + np.log(np.where(none, 1.0, den)))
            sees_nan = (vis & nan_key[None, :]).any(axis=1)
            out[sq:eq, hq] = np.where(sees_nan[:, None], np.nan, o)
            lse[hq, sq:eq] = np.where(sees_nan, np.nan, l)
    return out, lse


def run_paged(case, ps, wrong=None, base=None):
    """a (wrong) kernel on the case's pools of page size ps"""
    c = make(case)
    kp, vp, table = paged(case, ps)
    seqs = gather(kp, vp, table, c["lens"], c["lq"], c["Hkv"], ps, c["fmt"], None if wrong == "lo_prefix" else wrong)
    return attend_f64(c, seqs, wrong if wrong == "lo_prefix" else None, base)
