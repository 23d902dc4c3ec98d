"""Inputs, the float64 reference, packing and the check of the MLA entries (tests/test_gpu_mla.py, tests/test_mla_inputs.py):
fa_mla_decode and fa_mla_append.  Pure numpy plus the `oracle` fixture; nothing here touches a GPU.

The contract, from include/fa_mi355.h: the latent cache holds one row of 576 elements per token for all heads; Q is packed
(total_q, Hq, 576), O (total_q, Hq, 512), lse [Hq, total_q]; [s_b, e_b) are the clamps of cu_seqlens_q, n_b = min(e_b - s_b, max_q),
L_b = clamp(seqlens_k[b], 0, capacity).  Row i < n_b of head h sees the keys [0, c_i), c_i = max(0, L_b - n_b + 1 + i) under the
causal mask and L_b without; logits over all 576 elements, O over the first 512.

The packing is decode_varlen_inputs.Layout (3 tokens before s_0, 2 behind e_{B-1}), the page scatter and the bounds are
common_inputs'.  Inputs are N(0,1) rounded to the 16-bit type, with scale = 576 ** -0.5: logits of O(1).  One element of q and of each
sequence's last max_q keys is boosted mildly (a logit share of BOOST_Q * BOOST_K / 24 = 2), so that a wrong causal limit moves weight
the bounds see; the element is the first ROTARY one (column 512), which moves the logits and never reaches O.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_varlen_inputs as dv

DC, DR, DQK = 512, 64, 576
SCALE = DQK ** -0.5
BOOST_Q, BOOST_K = 4.0, 12.0
LEAD, TRAIL = dv.LEAD, dv.TRAIL

# lens are RAW (the entry clamps them into [0, Ncap]); spans are the tokens each sequence owns, n_b = min(span, max_q)
FAMILIES = {
    # one head; L in {0, 1, 63, 64}: L = 0 and L = 1 < n_b = 2 leave rows without a key; a negative raw length
    "h1": dict(B=4, Hq=1, max_q=2, Ncap=256, lens=(-3, 1, 63, 64), spans=(1, 2, 1, 2), seed=9101),
    # an idle slot (n_b = 0), a sequence that owns more tokens than max_q, L = capacity, L = 3 < n_b = 4
    "h5": dict(B=4, Hq=5, max_q=4, Ncap=256, lens=(65, 200, 256, 3), spans=(0, 1, 4, 6), seed=9102),
    # a raw length above the capacity; L = 65 is one key into the second 64-key tile
    "h16": dict(B=3, Hq=16, max_q=2, Ncap=512, lens=(600, 300, 65), spans=(1, 2, 1), seed=9103),
    # 3 x 48 = 144 rows: more than one row block at 64 and at 128 rows per workgroup
    "h48": dict(B=2, Hq=48, max_q=3, Ncap=256, lens=(200, 130), spans=(3, 2), seed=9104),
    # the workload's head count, one token per sequence
    "h128": dict(B=2, Hq=128, max_q=1, Ncap=256, lens=(256, 77), spans=(1, 1), seed=9105),
}
NAMES = list(FAMILIES)


def family(name):
    return FAMILIES[name]


@functools.lru_cache(maxsize=None)
def layout(name):
    f = family(name)
    cu = np.cumsum([LEAD] + list(f["spans"]))
    lay = dv.Layout(cu, int(cu[-1]) + TRAIL, f["max_q"])
    assert lay.n == [min(s, f["max_q"]) for s in f["spans"]]
    return lay


@functools.lru_cache(maxsize=None)
def inputs(oracle, name, fmt):
    """-> ((q [B*Hq, max_q, 576], c [B, Ncap, 576]) fp32 values of 16-bit numbers, (their uint16 encodings)), read-only"""
    f = family(name)
    B, Hq, Nq, Ncap = f["B"], f["Hq"], f["max_q"], f["Ncap"]
    rng = np.random.default_rng(f["seed"])
    q = rng.standard_normal((B * Hq, Nq, DQK)).astype(np.float32)
    c = rng.standard_normal((B, Ncap, DQK)).astype(np.float32)
    q[:, :, DC] = BOOST_Q
    for b in range(B):
        L = cm.clamp(f["lens"][b], Ncap)
        c[b, max(0, L - Nq):L, DC] = BOOST_K
    bits = tuple(oracle.encode16(x, fmt) for x in (q, c))
    vals = tuple(oracle.decode16(x, fmt) for x in bits)
    for a in vals + bits:
        a.setflags(write=False)
    return vals, bits


def expected_f64(q, c, lens, n, max_q, Hq, causal, scale=SCALE):
    """q [B*Hq, max_q, 576], c [B, Ncap, 576] (16-bit-rounded values), lens raw [B], n [B] live rows
    -> (O [B*Hq, max_q, 512], lse [B*Hq, max_q]) float64, row by row; dead rows and rows without a key: zeros and -inf"""
    B, Ncap = c.shape[0], c.shape[1]
    out = np.zeros((B * Hq, max_q, DC), np.float64)
    lse = np.full((B * Hq, max_q), -np.inf, np.float64)
    for b in range(B):
        _, lim, live = cm.row_limits(cm.clamp(lens[b], Ncap), n[b], max_q, causal)
        cb = c[b].astype(np.float64)
        for h in range(Hq):
            for i in np.flatnonzero(live):
                if lim[i] == 0:
                    continue
                s = (cb[:lim[i]] @ q[b * Hq + h, i].astype(np.float64)) * scale
                m = s.max()
                p = np.exp(s - m)
                out[b * Hq + h, i] = (p / p.sum()) @ cb[:lim[i], :DC]
                lse[b * Hq + h, i] = m + np.log(p.sum())
    return out, lse


@functools.lru_cache(maxsize=None)
def reference(oracle, name, fmt, causal):
    """expected_f64 of the family (padded [B*Hq, max_q, ...]), computed once and read-only"""
    f, lay = family(name), layout(name)
    (q, c), _ = inputs(oracle, name, fmt)
    out, lse = expected_f64(q, c, f["lens"], lay.n, f["max_q"], f["Hq"], causal)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def packed_q_bits(oracle, name, fmt, nan=cm.NAN16):
    """the family's Q encodings, packed (total_q, Hq, 576), with NaN in the rows of no sequence"""
    _, (qb, _) = inputs(oracle, name, fmt)
    return dv.pack_rows(layout(name), qb, np.uint16(nan))


def poisoned_cache(oracle, name, fmt):
    """the family's cache encodings [B, Ncap, 576] with NaN in every row at or past the clamped length"""
    _, (_, cb) = inputs(oracle, name, fmt)
    return cm.poisoned(cb[:, None], family(name)["lens"])[:, 0]


def paged_cache(oracle, name, fmt, ps, seed=5):
    """-> (pool [num_pages, ps, 576] uint16, table [B, max_pages] int32) by common_inputs.scatter: a shuffled table, garbage in the
    entries past the last live page, NaN in every pool row no key lies in"""
    _, (_, cb) = inputs(oracle, name, fmt)
    pool, _, table = cm.scatter(cb[:, None], cb[:, None], family(name)["lens"], ps, seed)
    return np.ascontiguousarray(pool[:, 0]), table


def check(oracle, name, got_o, got_lse, want, want_lse, fmt, what, sentinel=True):
    """got_o [total_q, Hq, 512] float32, got_lse [Hq, total_q] float32 against the padded float64 reference at the project's bounds,
    exactly as common_inputs.check_decode applies them (MAX_ABS, REL_L2[fmt], 2 * P_EPS[fmt] on lse), with the packed tier's rules on
    rows without a key and tokens of no sequence: decode_varlen_inputs.check"""
    dv.check(oracle, layout(name), got_o, got_lse, want, want_lse, fmt, what, sentinel=sentinel)


# ---- numpy kernels: the right one and the wrong ones the check must reject -----------------------------------------------------------
WRONG = ("v_all_576", "v_last_512", "logits_512", "scale_512_only", "causal_at_start", "max_q_in_the_limit", "fold_transposed",
         "no_length_clamp", "lse_log2", "merge_without_l")


def numpy_kernel(oracle, name, fmt, causal=True, wrong=None, S=2):
    """What a kernel would leave in pre-filled fp32 O [total_q, Hq, 512] and lse [Hq, total_q]: float64 arithmetic rounded to fp32,
    with one of the WRONG rules in the place of the right one (None: the entry as specified, merged from S key splits)."""
    f, lay = family(name), layout(name)
    B, Hq, Nq, Ncap = f["B"], f["Hq"], f["max_q"], f["Ncap"]
    (q, c), _ = inputs(oracle, name, fmt)
    flat = np.concatenate([c.reshape(-1, DQK).astype(np.float64), np.zeros((Ncap, DQK))])   # what lies behind a sequence's cache
    o = np.zeros((B * Hq, Nq, DC), np.float64)
    lse = np.full((B * Hq, Nq), -np.inf, np.float64)
    for b in range(B):
        n = lay.n[b]
        L = max(int(f["lens"][b]), 0) if wrong == "no_length_clamp" else cm.clamp(f["lens"][b], Ncap)
        keys = flat[b * Ncap:b * Ncap + L]
        for p in range(n * Hq):
            i, h = divmod(p, Hq)
            qi, qh = (p % n, p // n) if wrong == "fold_transposed" else (i, h)   # the row's Q read as if the fold were head-major
            qq = q[b * Hq + qh, qi].astype(np.float64)
            if not causal:
                lim = L
            elif wrong == "causal_at_start":
                lim = min(i + 1, L)
            else:
                lim = max(0, L - (Nq if wrong == "max_q_in_the_limit" else n) + 1 + i)
            if lim == 0:
                continue
            kk = keys[:lim]
            if wrong == "logits_512":
                s = (kk[:, :DC] @ qq[:DC]) * SCALE
            elif wrong == "scale_512_only":
                s = (kk[:, :DC] @ qq[:DC]) * SCALE + kk[:, DC:] @ qq[DC:]
            else:
                s = (kk @ qq) * SCALE
            vv = kk[:, DR:] if wrong == "v_last_512" else kk[:, :DC]
            # S splits of the 64-key tiles, merged: (o_s unnormalised, m_s, l_s) -> M, sum of w_s l_s, sum of w_s o_s
            tiles = -(-lim // 64)
            per = -(-tiles // S) * 64
            parts = [(s[a:a + per], vv[a:a + per]) for a in range(0, lim, per)]
            ms = [x.max() for x, _ in parts]
            M = max(ms)
            ls = [np.exp(x - m).sum() for (x, _), m in zip(parts, ms)]
            os_ = [np.exp(x - m) @ v for (x, v), m in zip(parts, ms)]
            w = [np.exp(m - M) for m in ms]
            if wrong == "merge_without_l":
                den = sum(w)
                num = sum(wi * oi / li for wi, oi, li in zip(w, os_, ls))
            else:
                den = sum(wi * li for wi, li in zip(w, ls))
                num = sum(wi * oi for wi, oi in zip(w, os_))
            o[b * Hq + h, i] = num / den
            lse[b * Hq + h, i] = M + np.log(den)
            if wrong == "v_all_576":   # a 576-wide PV product whose rows land in the 512-wide O row: the tail of the row before it
                full = (np.exp(s - M) / np.exp(s - M).sum()) @ kk
                o[b * Hq + h, i] = np.concatenate([full[DC:], full[:DC - DR]])
    if wrong == "lse_log2":
        lse = lse / np.log(2.0)
    po = dv.pack_rows(lay, o.astype(np.float32), 0.0)
    po[~lay.owned] = np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0]
    pl = dv.pack_lse(lay, lse.astype(np.float32), np.float32(dv.SENTINEL_LSE))
    return po, pl


# ---- fa_mla_append ---------------------------------------------------------------------------------------------------------------------
def append_model(cache, new, cu, lens, total_new, table=None):
    """The bytes fa_mla_append leaves: cache [B, Ncap, 576] uint16 (or with `table` a pool [num_pages, ps, 576]), new [total_new, 576]
    uint16, cu [B+1] raw, lens [B] raw or None -> (cache after, lengths after)"""
    out = np.array(cache)
    B = len(cu) - 1
    if table is None:
        cap = cache.shape[1]
    else:
        ps = cache.shape[1]
        cap = table.shape[1] * ps
    after = np.zeros(B, np.int32)
    for b in range(B):
        s = min(max(int(cu[b]), 0), total_new)
        e = max(min(max(int(cu[b + 1]), 0), total_new), s)
        L = 0 if lens is None else cm.clamp(lens[b], cap)
        for i in range(e - s):
            p = L + i
            if p >= cap:
                break
            if table is None:
                out[b, p] = new[s + i]
            else:
                page = int(table[b, p // ps])
                if 0 <= page < cache.shape[0]:
                    out[page, p % ps] = new[s + i]
        after[b] = min(L + (e - s), cap)
    return out, after
