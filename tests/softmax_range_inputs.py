"""Wide-logit-range inputs for the two kernel families that keep their own copy of the online softmax with a lazy reference maximum:
fa_mla_decode (with its private merge) and the varlen prefill template (fa_forward_varlen, its window / soft-cap / sinks form,
fa_forward_varlen_kvcache contiguous, paged and fp8, and the prefill arm of fa_kvcache_attend_varlen) -- and a numpy MODEL of that
scheme with seven defect switches.  tests/test_softmax_range_inputs.py shows without a GPU that the inputs force what they are named
for and that the check of tests/test_gpu_softmax_range.py accepts the model and rejects every defect.  Pure numpy plus the `oracle`
fixture; nothing here touches a GPU.

The scheme (fa_tile.hpp): a row keeps a reference m_ref (log2 units) that moves only when the maximum of a key tile
exceeds it by more than kThr = 8 for SOME row of the wave (the vote is wave-wide: every row of a voting wave takes
max(m_ref, its tile maximum)); when it moves, O and l are rescaled by alpha = 2^(m_ref - m_new).  Weights 2^(s - m_ref) are rounded
to the input format, l sums the rounded weights, O and l are fp32.  MLA decode deals 64-key units to S splits, walks a split in
32-key tiles and merges the partials by 2^(m_s - M).

Scores and lifts are in log2 units (logit * log2 e).  `base` of a row is its largest BENIGN score: over every key of its sequence
that was not rebuilt for that row.  A spike is (row, key, lift): the key scores base + lift with the row.  A key is rebuilt as a sum
of multiples of hostile query rows that were made orthogonal to each other first, so one key can serve two rows and is benign for all
the others.  Every builder rounds to the 16-bit format and then MEASURES its lifts.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_varlen_inputs as dv
import fallback_inputs as fi
import mla_inputs as mi
import varlen_inputs as vi
import varlen_logit_inputs as li

KTHR = 8.0                      # fa_tile.hpp
LOG2E, LN2 = fi.LOG2E, fi.LN2
STEP = fi.STAIR_STEP            # 7: one step stays under kThr, the next one moves the reference
SHIFT = fi.KV_SHIFT             # 300 log2 units
FMTS = (0, 1)


def bounds(fmt, vmax, out_same=False):
    """(max-abs, rel-L2) on O: test_gpu_fallback_paths.py's _bounds rule with peaked rows -- fp16 cm.MAX_ABS and cm.REL_L2, bf16
    cm.peaked_tol and 3e-2, rel-L2 x 1.5 for a 16-bit output"""
    import test_gpu_fallback_paths as fp
    return fp._bounds(fmt, vmax, out_same, True)


def _round16(x, fmt):
    return vi.decode16(vi.encode16(x, fmt), fmt)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- MLA ---------------------------------------------------------------------------------------------------------------------------------
MLA = dict(B=3, Hq=5, max_q=4, Ncap=512, lens=(421, 66, 130), spans=(4, 2, 4), seed=9301)
MLA_TILE, MLA_UNIT = 32, 64
MLA_SPLITS = (1, 2, 3, MLA["Ncap"] // 64, 0)
# sequence 0 (421 keys = 13 tiles of 32 and 5 keys): (kind, token, head, [(key, lift)]); every row shares the one wave of its sequence
MLA_STAIR_TILES = 7
MLA_KINDS = (
    ("staircase", 0, 1, [(32 * t + 5 + t, STEP * t) for t in range(MLA_STAIR_TILES)]),
    ("jump 40 in the last split", 1, 2, [(390, 40.0)]),
    ("jump 150 in the last split", 2, 3, [(400, 150.0)]),
    ("all but tile 0 below -200", 3, 4, [(20, 210.0)]),
    ("jump 40 on the last key", 3, 0, [(420, 40.0)]),
    ("masked 150 on the last key", 0, 0, [(420, 150.0)]),
)
# sequence 1 (66 keys, two tokens): key 65 is seen by the last token alone under the mask; both spikes belong to its rows
MLA_SEQ1 = (("jump 40 on key 65", 1, 0, [(65, 40.0)]), ("jump 150 on key 64", 1, 1, [(64, 150.0)]))
MLA_SHIFTED = ((0, -SHIFT), (1, SHIFT))   # sequence 2: (head, level of every logit)


@functools.lru_cache(maxsize=None)
def mla_layout():
    cu = np.cumsum([mi.LEAD] + list(MLA["spans"]))
    lay = dv.Layout(cu, int(cu[-1]) + mi.TRAIL, MLA["max_q"])
    assert lay.n == list(MLA["spans"])
    return lay


def mla_scores(q, c, b, Hq, i, h, L):
    """[L] float64 log2 scores of (token i, head h) of sequence b"""
    return (c[b, :L].astype(np.float64) @ q[b * Hq + h, i].astype(np.float64)) * (mi.SCALE * LOG2E)


@functools.lru_cache(maxsize=None)
def mla_case(fmt):
    """-> dict: q [B*Hq, max_q, 576], c [B, Ncap, 576] (16-bit-rounded fp32), bits, spikes [(b, kind, token, head, key, lift built,
    lift measured)].  The hostile keys live in the ROTARY columns (512..575) only: the rotary parts of a sequence's query rows are made
    orthogonal (20 <= 64 rows), and a key's rotary part becomes the sum of multiples of rows' rotary parts that brings each of those
    rows' TOTAL score to its target.  V -- the first 512 columns -- stays N(0,1)."""
    f = MLA
    B, Hq, Nq, Ncap = f["B"], f["Hq"], f["max_q"], f["Ncap"]
    rng = np.random.default_rng(f["seed"] + fmt)
    q = rng.standard_normal((B * Hq, Nq, mi.DQK)).astype(np.float32)
    c = rng.standard_normal((B, Ncap, mi.DQK)).astype(np.float32)
    for b in (0, 1):
        n = f["spans"][b]
        rot = q[b * Hq:(b + 1) * Hq, :n, mi.DC:].reshape(Hq * n, mi.DR)
        q[b * Hq:(b + 1) * Hq, :n, mi.DC:] = fi._orthogonal_rows(rot).reshape(Hq, n, mi.DR)
    # sequence 2: every key carries the same offset along the all-ones direction of the rotary columns, head 0 against it, head 1 along it
    u = np.ones(mi.DR, np.float32) / np.sqrt(mi.DR)
    off = np.sqrt(SHIFT / (mi.SCALE * LOG2E * mi.DR))
    c[2, :, mi.DC:] -= np.outer(c[2, :, mi.DC:] @ u, u)
    c[2, :, mi.DC:] += off
    q[2 * Hq:3 * Hq, :, mi.DC:] -= (q[2 * Hq:3 * Hq, :, mi.DC:] @ u)[..., None] * u
    for h, level in MLA_SHIFTED:
        q[2 * Hq + h, :, mi.DC:] += np.sign(level) * off
    q = _round16(q, fmt)
    c = _round16(c, fmt).copy()
    plan = [(0, k) for k in MLA_KINDS] + [(1, k) for k in MLA_SEQ1]
    for b in (0, 1):
        L = f["lens"][b]
        rebuilt = {}
        for bb, (kind, i, h, keys) in plan:
            if bb != b:
                continue
            own = [key for key, _ in keys]
            s = mla_scores(q, c, b, Hq, i, h, L)
            base = np.delete(s, own).max()
            qr = q[b * Hq + h, i, mi.DC:].astype(np.float64)
            for key, lift in keys:
                nope = float(c[b, key, :mi.DC].astype(np.float64) @ q[b * Hq + h, i, :mi.DC].astype(np.float64))
                want = (base + lift) / (mi.SCALE * LOG2E) - nope
                rebuilt[key] = rebuilt.get(key, 0.0) + qr * (want / float(qr @ qr))
        for key, rot in rebuilt.items():
            c[b, key, mi.DC:] = rot
    c = _round16(c, fmt)
    spikes = []
    for b, (kind, i, h, keys) in plan:
        s = mla_scores(q, c, b, Hq, i, h, f["lens"][b])
        base = np.delete(s, [key for key, _ in keys]).max()
        spikes += [(b, kind, i, h, key, lift, float(s[key] - base)) for key, lift in keys]
    bits = tuple(vi.encode16(x, fmt) for x in (q, c))
    _frozen(q, c, *bits)
    return dict(q=q, c=c, bits=bits, spikes=spikes, fmt=fmt)


def mla_hostile(b):
    """{(token, head): [keys]} of sequence b"""
    return {(i, h): [key for key, _ in keys] for kind, i, h, keys in (MLA_KINDS if b == 0 else MLA_SEQ1 if b == 1 else ())}


@functools.lru_cache(maxsize=None)
def mla_reference(fmt, causal):
    case = mla_case(fmt)
    out, lse = mi.expected_f64(case["q"], case["c"], MLA["lens"], mla_layout().n, MLA["max_q"], MLA["Hq"], causal)
    _frozen(out, lse)
    return out, lse


def mla_packed_q_bits(fmt, nan=cm.NAN16):
    return dv.pack_rows(mla_layout(), mla_case(fmt)["bits"][0], np.uint16(nan))


def mla_poisoned_cache(fmt):
    return cm.poisoned(mla_case(fmt)["bits"][1][:, None], MLA["lens"])[:, 0]


def mla_paged_cache(fmt, ps, seed=5):
    cb = mla_case(fmt)["bits"][1]
    pool, _, table = cm.scatter(cb[:, None], cb[:, None], MLA["lens"], ps, seed)
    return np.ascontiguousarray(pool[:, 0]), table


def mla_vmax(fmt):
    return float(np.abs(mla_case(fmt)["c"][:, :, :mi.DC]).max())


def figures_packed(lay, got_o, got_lse, want, want_lse):
    """(max_abs, rel_l2 of O over the live rows, largest lse error over the rows with a key) of a packed result against the PADDED
    float64 reference; NaN counts as inf"""
    B = len(lay.n)
    o = dv.unpack_rows(lay, np.asarray(got_o, np.float64), B)
    lse = dv.unpack_rows(lay, np.ascontiguousarray(np.asarray(got_lse, np.float64).T), B, fill=-np.inf)
    diff = np.abs(o - want)
    diff = np.where(np.isnan(diff), np.inf, diff)
    fin = np.isfinite(want_lse)
    le = np.abs(lse[fin] - want_lse[fin])
    le = float(np.where(np.isnan(le), np.inf, le).max(initial=0.0))
    with np.errstate(over="ignore", invalid="ignore"):
        rl = float(np.sqrt((diff ** 2).sum() / max((want ** 2).sum(), 1e-300)))
    return float(diff.max()), (rl if rl == rl else np.inf), le


def check_packed(oracle, lay, got_o, got_lse, want, want_lse, fmt, vmax, entry, case, out_same=False):
    """The GPU tier's check of a packed fp32 result [total_q, Hq, dv], lse [Hq, total_q]: the structure of decode_varlen_inputs.check
    (sentinels in the tokens of no sequence, rows without a key exactly 0 / -inf, nothing NaN) at bounds(): for fp16 these are
    dv.check's own numbers, and dv.check itself is applied as well.  Prints the RANGE line first.  -> (max_abs, rel_l2, lse_abs)"""
    B, Hq = len(lay.n), got_o.shape[1]
    ma, rl, le = figures_packed(lay, got_o, got_lse, want, want_lse)
    ma_b, rl_b = bounds(fmt, vmax, out_same)
    print(f"RANGE|{entry}|{case}|{ma:.3e}|{rl:.3e}|{le:.3e}   (bounds {ma_b:.3e} {rl_b:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    what = f"{entry} {case}"
    free = ~lay.owned
    assert (np.ascontiguousarray(got_o[free]).view(np.uint32) == dv.SENTINEL_O32).all(), what + ": an O row of no sequence was written"
    assert (got_lse[:, free] == np.float32(dv.SENTINEL_LSE)).all(), what + ": an lse entry of no sequence was written"
    live = dv.live_mask(lay, Hq)
    o = dv.unpack_rows(lay, got_o, B)
    lse = dv.unpack_rows(lay, np.ascontiguousarray(got_lse.T), B, fill=-np.inf)
    fin = np.isfinite(want_lse)
    assert np.isfinite(o).all(), what + ": O is not finite"
    assert not np.isnan(lse).any(), what + ": NaN in lse"
    nokey = live & ~fin
    assert (o[nokey] == 0.0).all() and (lse[nokey] == -np.inf).all(), what + ": a row without a key is not exactly 0 / -inf"
    assert ma <= ma_b and rl <= rl_b, f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert np.isfinite(lse[fin]).all() and le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"
    if fmt == 0 and not out_same:
        dv.check(oracle, lay, got_o, got_lse, want, want_lse, fmt, what)
    return ma, rl, le


# ---- the model of the lazy scheme ----------------------------------------------------------------------------------------------------------
DEFECTS = ("no_alpha_o", "no_alpha_l", "vote_prev", "max_before_mask", "merge_first", "merge_plain", "lse_stale_m")


def _round_weights(p, fmt):
    with np.errstate(over="ignore"):
        return p.astype(np.float16).astype(np.float32) if fmt == 0 else _round16(p, fmt)


def lazy_pass(s, vis, v, k0, k1, tile, fmt, waves, defect=None):
    """One pass of the scheme over the keys [k0, k1) in tiles of `tile` keys from k0 on.  s [R, K] float64 final scores (log2 units,
    before the masks), vis [R, K] bool, v [K, dv] values, waves: lists of rows that vote together.
    -> dict(o [R, dv], m, l, m_stale [R] float32 -- unnormalised partial --, rise [R, tiles] float64: tile maximum minus the reference it
    met (nan: no reference yet or no visible key in the tile))
    Defects: no_alpha_o, no_alpha_l, vote_prev, max_before_mask (see DEFECTS); the others act in finish() and merge()."""
    R = s.shape[0]
    m = np.full(R, -np.inf, np.float32)
    m_stale = m.copy()
    prev = m.copy()
    l = np.zeros(R, np.float32)
    o = np.zeros((R, v.shape[1]), np.float32)
    rises = []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t0 in range(k0, k1, tile):
            sl = slice(t0, min(t0 + tile, k1))
            st = np.where(vis[:, sl], s[:, sl], -np.inf).astype(np.float32)
            tmax = s[:, sl].max(axis=1).astype(np.float32) if defect == "max_before_mask" else st.max(axis=1)
            rise = (tmax - m).astype(np.float64)
            rises.append(np.where(np.isfinite(rise), rise, np.nan))
            own = (tmax - (prev if defect == "vote_prev" else m)) > np.float32(KTHR)
            for w in waves:
                if not own[w].any():
                    continue
                m_new = np.maximum(tmax[w], m[w])
                alpha = np.where(m[w] == -np.inf, np.float32(0.0), np.exp2(m[w] - m_new)).astype(np.float32)
                if defect != "no_alpha_o":
                    o[w] *= alpha[:, None]
                if defect != "no_alpha_l":
                    l[w] *= alpha
                m_stale[w] = np.where((m_new != m[w]) & np.isfinite(m[w]), m[w], m_stale[w])
                m[w] = m_new
            prev = tmax
            neg_m = np.where(m == -np.inf, np.float32(0.0), -m)
            p = _round_weights(np.exp2(st + neg_m[:, None]).astype(np.float32), fmt)
            l = (l + p.sum(axis=1, dtype=np.float32)).astype(np.float32)
            o = (o + (p.astype(np.float64) @ v[sl].astype(np.float64)).astype(np.float32)).astype(np.float32)
    m_stale = np.where(np.isfinite(m_stale), m_stale, m)   # the reference before its last move; a row that never moved: its reference
    return dict(o=o, m=m, l=l, m_stale=m_stale, rise=np.stack(rises, axis=1) if rises else np.zeros((R, 0)))


def finish(part, defect=None, sink2=None):
    """the epilogue of a single pass -> (O [R, dv], lse [R] natural log) float32; sink2 [R]: a sink logit per row in log2 units (-inf:
    none), joined to (m, l) once"""
    o, m, l = part["o"].copy(), part["m"].copy(), part["l"].copy()
    m_used = part["m_stale"] if defect == "lse_stale_m" else m
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        none = m == -np.inf
        if sink2 is not None:
            sk = np.asarray(sink2, np.float32)
            m_new = np.maximum(m, sk)
            wk = np.where(none, np.float32(0.0), np.exp2(m - m_new)).astype(np.float32)
            ws = np.where(sk == -np.inf, np.float32(0.0), np.exp2(sk - m_new)).astype(np.float32)
            l = (l * wk + ws).astype(np.float32)
            o = o * wk[:, None]
            m_used = np.minimum(m_used, m_new) if defect == "lse_stale_m" else m_new
            m = m_new
        inv = np.where(none | (l == 0), np.float32(0.0), np.float32(1.0) / l)
        out = (o * inv[:, None]).astype(np.float32)
        lse = np.where((m == -np.inf) | (l == 0), -np.inf, (m_used + np.log2(l)) * np.float32(LN2)).astype(np.float32)
    return out, lse


def merge(parts, defect=None):
    """the merge behind S > 1 splits: weights 2^(m_s - M), M the largest m_s; a partial with m = -inf weighs 0"""
    ms = np.stack([p["m"] for p in parts])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        M = ms[0] if defect == "merge_first" else ms.max(axis=0)
        L = np.zeros_like(M)
        acc = np.zeros_like(parts[0]["o"])
        for p in parts:
            w = np.where(p["m"] == -np.inf, np.float32(0.0), np.float32(1.0) if defect == "merge_plain" else np.exp2(p["m"] - M))
            w = w.astype(np.float32)
            L = (L + p["l"] * w).astype(np.float32)
            acc = (acc + p["o"] * w[:, None]).astype(np.float32)
        inv = np.where(L == 0, np.float32(0.0), np.float32(1.0) / L)
        M_used = np.stack([p["m_stale"] for p in parts]).max(axis=0) if defect == "lse_stale_m" else M
        lse = np.where(L == 0, -np.inf, (M_used + np.log2(L)) * np.float32(LN2)).astype(np.float32)
        return (acc * inv[:, None]).astype(np.float32), lse


def mla_split_count(B, Hq, max_q, cap):
    """the library's choice (fa_mla_decode.hip: two workgroups per CU of 256, at least four 64-key units per split)"""
    tiles = -(-cap // MLA_UNIT)
    base = B * -(-(max_q * Hq) // 64)
    s = max(1, min(-(-512 // base), tiles // 4))
    return -(-tiles // -(-tiles // s))


def mla_model(q, c, lens, lay, Hq, fmt, causal=True, S=1, defect=None, events=None):
    """The scheme on an MLA problem (q [B*Hq, max_q, 576], c [B, Ncap, 576] rounded values) -> what a kernel would leave in
    sentinel-filled packed fp32 O [total_q, Hq, 512] and lse [Hq, total_q].  events: a dict that receives {(b, token, head):
    [rise arrays, one per split]}"""
    B, Ncap, Nq = c.shape[0], c.shape[1], lay.max_q
    S = S or mla_split_count(B, Hq, Nq, Ncap)
    o = np.zeros((B * Hq, Nq, mi.DC), np.float32)
    lse = np.full((B * Hq, Nq), -np.inf, np.float32)
    for b in range(B):
        n, L = lay.n[b], cm.clamp(lens[b], Ncap)
        R = n * Hq
        if R == 0:
            continue
        rows = [divmod(p, Hq) for p in range(R)]
        lim = cm.row_limits(L, n, Nq, causal)[1]
        s = np.stack([mla_scores(q, c, b, Hq, i, h, L) for i, h in rows]) if L else np.zeros((R, 0))
        vis = np.arange(L)[None, :] < np.array([lim[i] for i, _ in rows])[:, None]
        waves = [list(range(a, min(a + 32, R))) for a in range(0, R, 32)]
        chunk = -(-(-(-L // MLA_UNIT)) // S) * MLA_UNIT
        parts = [lazy_pass(s, vis, c[b, :L, :mi.DC], min(sp * chunk, L), min(L, sp * chunk + chunk), MLA_TILE, fmt, waves, defect)
                 for sp in range(S)]
        ob, lb = finish(parts[0], defect) if S == 1 else merge(parts, defect)
        for p, (i, h) in enumerate(rows):
            o[b * Hq + h, i], lse[b * Hq + h, i] = ob[p], lb[p]
            if events is not None:
                events[b, i, h] = [part["rise"][p] for part in parts]
    po = dv.pack_rows(lay, o, 0.0)
    po[~lay.owned] = np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0]
    return po, dv.pack_lse(lay, lse, np.float32(dv.SENTINEL_LSE))


# ---- varlen prefill ------------------------------------------------------------------------------------------------------------------------
VARLEN = dict(Hkv=1, G=2, lq=(130, 5), lk=(421, 66))
VARLEN_D = (64, 128)
FEATURES = ("plain", "window", "softcap", "sinks")
WINDOW = 100
SOFTCAP = 20.0        # natural units: a +150 (log2) spike is bent to about 29 log2 units, still far above kThr; benign logits barely move
SINK_GAP = 60.0       # natural units
VARLEN_SHIFT = VARLEN["lk"][0] - VARLEN["lq"][0]   # 291: row i of sequence 0 sees the keys j <= i + 291 under the mask
VARLEN_STAIR_TILES = 7
# sequence 0, 64-key tiles (421 keys = 6 tiles and 37 keys), rows 0..127 one 128-row block of four 32-row waves, rows 128..129 the next:
# (kind, row, head of the group, [(key, lift)], visible under the mask)
VARLEN_KINDS = (
    ("staircase", 100, 0, [(64 * t + 3 + t if t < 6 else 386, STEP * t) for t in range(VARLEN_STAIR_TILES)], True),   # wave 3
    ("jump 40 in the last whole tile", 101, 1, [(350, 40.0)], True),
    ("jump 150 in the last whole tile", 40, 0, [(325, 150.0)], True),                                                  # wave 1
    ("all but tile 0 below -200", 5, 1, [(20, 210.0)], True),                                                          # wave 0
    ("jump 40 on the last key", 129, 0, [(420, 40.0)], True),                      # the partial tile; block 1 of the sequence
    ("masked 150 on the last key", 10, 1, [(420, 150.0)], False),
    ("jump 40 on the diagonal", 110, 0, [(110 + VARLEN_SHIFT, 40.0)], True),       # key 401, inside the partial tile
    ("masked 150 one past the diagonal", 60, 1, [(60 + VARLEN_SHIFT + 1, 150.0)], False),
)
# W = 100: row i sees [i + 192, i + 292) under the mask, [i + 192, 421) without
VARLEN_WINDOW_KINDS = (
    ("masked 150 just below the window", 50, 0, [(50 + VARLEN_SHIFT + 1 - WINDOW - 1, 150.0)], False),
    ("jump 40 on the window's first key", 51, 1, [(51 + VARLEN_SHIFT + 1 - WINDOW, 40.0)], True),
    ("jump 40 on the diagonal", 52, 0, [(52 + VARLEN_SHIFT, 40.0)], True),
    ("staircase", 100, 1, [(300, 0.0), (340, STEP), (386, 2 * STEP)], True),   # row 100 sees [292, 392): tiles 4, 5, 6
)


def varlen_kinds(feature):
    return VARLEN_WINDOW_KINDS if feature == "window" else VARLEN_KINDS


def varlen_scores(q, k, i, g, d, sk=0, ek=None):
    """[Lk] float64 log2 scores of row i (a token of the packed q), head g, against the packed keys [sk, ek)"""
    return (k[sk:ek, 0].astype(np.float64) @ q[i, g].astype(np.float64)) * (LOG2E / np.sqrt(d))


def _build_varlen(q, k, kinds, d, Lk):
    """q (total_q, 2, d), k (total_k, 1, d) float32, both changed in place (sequence 0 starts at row 0 of both): the hostile rows are
    made orthogonal, their span is projected out of every other query row, and the spiked keys are rebuilt from them"""
    hostile = [(i, g) for _, i, g, _, _ in kinds]
    assert len(hostile) <= 12 and len(set(hostile)) == len(hostile)
    H = fi._orthogonal_rows(np.stack([q[i, g] for i, g in hostile])).astype(np.float64)
    for (i, g), x in zip(hostile, H):
        q[i, g] = x
    unit = H / np.linalg.norm(H, axis=1, keepdims=True)
    flat = q.reshape(-1, d).astype(np.float64)
    keep = np.ones(flat.shape[0], bool)
    keep[[i * q.shape[1] + g for i, g in hostile]] = False
    flat[keep] -= (flat[keep] @ unit.T) @ unit
    q[...] = flat.reshape(q.shape).astype(np.float32)
    return hostile


def _spike_keys(q, k, kinds, d, Lk):
    rebuilt = {}
    for _, i, g, keys, _ in kinds:
        s = varlen_scores(q, k, i, g, d, 0, Lk)
        base = np.delete(s, [key for key, _ in keys]).max()
        qq = q[i, g].astype(np.float64)
        for key, lift in keys:
            rebuilt[key] = rebuilt.get(key, 0.0) + qq * ((base + lift) * LN2 * np.sqrt(d) / float(qq @ qq))
    for key, row in rebuilt.items():
        k[key, 0] = row


def measured_lifts(q, k, kinds, d, Lk):
    """[(kind, row, head, key, lift built, lift measured, visible under the mask)] on (rounded or quantised) values"""
    out = []
    for kind, i, g, keys, seen in kinds:
        s = varlen_scores(q, k, i, g, d, 0, Lk)
        base = np.delete(s, [key for key, _ in keys]).max()
        out += [(kind, i, g, key, lift, float(s[key] - base), seen) for key, lift in keys]
    return out


@functools.lru_cache(maxsize=None)
def varlen_case(d, fmt, feature="plain"):
    """-> dict on vi.make's conventions (q, k, v values with vi.TAIL NaN rows behind; qb, kb, vb; cu_q, cu_k; Hkv, G, d, fmt, scale; W,
    softcap, sinks) plus spikes = measured_lifts().  Sequence 1 (5 rows against 66 keys) is N(0,1): a block whose rows are all benign."""
    assert feature in FEATURES
    Hkv, G, lq, lk = VARLEN["Hkv"], VARLEN["G"], VARLEN["lq"], VARLEN["lk"]
    seed = 9400 + d + fmt
    q, _ = vi.packed(lq, Hkv * G, d, fmt, seed)
    k, _ = vi.packed(lk, Hkv, d, fmt, seed + 100)
    v, vb = vi.packed(lk, Hkv, d, fmt, seed + 200)
    nq, nk = sum(lq), sum(lk)
    q, k = q.copy(), k.copy()
    kinds = varlen_kinds(feature)
    _build_varlen(q[:nq], k[:nk], kinds, d, lk[0])
    q[:nq] = _round16(q[:nq], fmt)
    _spike_keys(q, k, kinds, d, lk[0])
    k[:nk] = _round16(k[:nk], fmt)
    qb, kb = np.full(q.shape, cm.NAN16, np.uint16), np.full(k.shape, cm.NAN16, np.uint16)
    qb[:nq], kb[:nk] = vi.encode16(q[:nq], fmt), vi.encode16(k[:nk], fmt)
    q, k = vi.decode16(qb, fmt), vi.decode16(kb, fmt)
    scale = 1.0 / np.sqrt(d)
    sinks = None
    if feature == "sinks":   # head 0: 60 above every key logit of the head (O near 0, lse near the sink); head 1: 60 below every one
        nat = [np.concatenate([(q[sq:eq, g].astype(np.float64) @ k[sk:ek, 0].astype(np.float64).T).ravel() * scale
                               for (sq, eq), (sk, ek) in zip(vi.bounds(vi.cu_of(lq), nq), vi.bounds(vi.cu_of(lk), nk))]) for g in range(G)]
        sinks = np.array([nat[0].max() + SINK_GAP, nat[1].min() - SINK_GAP], np.float32)
    out = dict(q=q, k=k, v=v, qb=qb, kb=kb, vb=vb, cu_q=vi.cu_of(lq), cu_k=vi.cu_of(lk), Hkv=Hkv, G=G, d=d, fmt=fmt, scale=scale, lq=lq,
               lk=lk, W=WINDOW if feature == "window" else 0, softcap=SOFTCAP if feature == "softcap" else 0.0, sinks=sinks,
               feature=feature, spikes=measured_lifts(q, k, kinds, d, lk[0]))
    _frozen(q, k, v, qb, kb, vb)
    return out


@functools.lru_cache(maxsize=None)
def varlen_reference(d, fmt, feature, causal):
    c = varlen_case(d, fmt, feature)
    out, lse = li.varlen_logits_f64(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["Hkv"], c["G"], causal, c["scale"], W=c["W"],
                                    softcap=c["softcap"], sinks=c["sinks"])
    _frozen(out, lse)
    return out, lse


def varlen_vmax(c):
    return float(np.abs(c["v"][:sum(c["lk"])]).max())


def varlen_cache(c, ncap=512):
    """the case's keys laid into a contiguous cache [B, Hkv, ncap, d] of encodings, cm.NAN16 in every row at or past a length ->
    (kc, vc, lens)"""
    lk = c["lk"]
    kc, vc = (np.full((len(lk), c["Hkv"], ncap, c["d"]), cm.NAN16, np.uint16) for _ in range(2))
    for b, (sk, ek) in enumerate(vi.bounds(c["cu_k"], sum(lk))):
        kc[b, :, :ek - sk] = c["kb"][sk:ek].transpose(1, 0, 2)
        vc[b, :, :ek - sk] = c["vb"][sk:ek].transpose(1, 0, 2)
    return kc, vc, np.array(lk, np.int32)


def varlen_problems(got, got_lse, want, want_lse, own, fmt, vmax, out_same, base=(vi.POISON, vi.POISON)):
    """vi.problems at bounds(): its findings on NaN, rows of no sequence, rows without a key and lse as they are, its two findings
    on O replaced by the same two at bounds(fmt, vmax, out_same) (for fp16 and fp32 output: the same numbers)"""
    found = [f for f in vi.problems(got, got_lse, want, want_lse, own, fmt, base) if not f.startswith("O")]
    got = np.asarray(got, np.float64)
    diff = np.where(np.isnan(got[own]), np.inf, np.abs(got[own] - want[own]))
    ma = float(diff.max(initial=0.0))
    with np.errstate(over="ignore", invalid="ignore"):
        rl = float(np.sqrt((diff ** 2).sum() / max((want[own] ** 2).sum(), 1e-300)))
    ma_b, rl_b = bounds(fmt, vmax, out_same)
    if ma > ma_b:
        found.append(f"O: max_abs {ma:.3e} > {ma_b:.3e}")
    if not rl <= rl_b:
        found.append(f"O: rel_l2 {rl:.3e} > {rl_b:.1e}")
    return found


def check_varlen(c, got, got_lse, want, want_lse, entry, case, out_same=False, base=(vi.POISON, vi.POISON)):
    """the GPU tier's check of a varlen result; prints the RANGE line first -> (max_abs, rel_l2, lse_abs)"""
    own = vi.owned(c["cu_q"], got.shape[0])
    with np.errstate(invalid="ignore"):
        ma, rl, le = vi.figures(np.nan_to_num(got, nan=np.inf), np.nan_to_num(got_lse, nan=np.inf), want, want_lse, own)
    ma_b, rl_b = bounds(c["fmt"], varlen_vmax(c), out_same)
    print(f"RANGE|{entry}|{case}|{ma:.3e}|{rl:.3e}|{le:.3e}   (bounds {ma_b:.3e} {rl_b:.1e} {2 * cm.P_EPS[c['fmt']]:.2e})")
    found = varlen_problems(got, got_lse, want, want_lse, own, c["fmt"], varlen_vmax(c), out_same, base)
    assert not found, f"{entry} {case}: {found}"
    return ma, rl, le


def varlen_model(c, causal, defect=None, events=None, out_same=False):
    """The scheme on a varlen case: 64-key tiles from key 0, one pass, waves of 32 consecutive rows of one (sequence, head, 128-row
    block); the soft-cap before the masks, the sink joined once at the end -> (O (total_q, Hq, d), lse (Hq, total_q)) float32 with
    vi.POISON in the rows of no sequence.  events receives {(b, row, head): rise array}"""
    q, k, v, d, G, fmt = c["q"], c["k"], c["v"], c["d"], c["G"], c["fmt"]
    total_q, Hq = q.shape[:2]
    out = np.full(q.shape, vi.POISON, np.float32)
    lse = np.full((Hq, total_q), vi.POISON, np.float32)
    for b, ((sq, eq), (sk, ek)) in enumerate(zip(vi.bounds(c["cu_q"], total_q), vi.bounds(c["cu_k"], k.shape[0]))):
        Lq, Lk = eq - sq, ek - sk
        lo, lim = li.limits(Lq, Lk, causal, c["W"])
        vis = (np.arange(Lk)[None, :] >= lo[:, None]) & (np.arange(Lk)[None, :] < lim[:, None])
        waves = [list(range(a, min(a + 32, Lq))) for a in range(0, Lq, 32)]
        for hq in range(Hq):
            s = (q[sq:eq, hq].astype(np.float64) @ k[sk:ek, hq // G].astype(np.float64).T) * (c["scale"] * LOG2E)
            if c["softcap"]:
                cap2 = c["softcap"] * LOG2E
                s = cap2 * np.tanh(s / cap2)
            part = lazy_pass(s, vis, v[sk:ek, hq // G], 0, Lk, cm.TILE, fmt, waves, defect)
            sink2 = None if c["sinks"] is None else np.full(Lq, np.float32(c["sinks"][hq]) * np.float32(LOG2E), np.float32)
            o, l = finish(part, defect, sink2)
            if sink2 is not None:
                o[part["m"] == -np.inf] = 0.0
            out[sq:eq, hq], lse[hq, sq:eq] = o, l
            if events is not None:
                for i in range(Lq):
                    events[b, i, hq] = part["rise"][i]
    if out_same:
        out = _round16(out, fmt)
    return out, lse


# ---- fp8 -----------------------------------------------------------------------------------------------------------------------------------
FP8_MIN_LIFT = 21.0


@functools.lru_cache(maxsize=None)
def varlen_fp8_case(d, fmt):
    """the plain case with K and V quantised to e4m3fn codes under varlen_cache_fp8_inputs' scales -> dict as varlen_case's with k, v the
    DECODED codes (the reference's inputs, scales apart), k8, v8 the codes, k_scale, v_scale, and spikes measured on k_scale * k8"""
    import fp8_inputs as f8
    import varlen_cache_fp8_inputs as v8
    c = dict(varlen_case(d, fmt, "plain"))
    ks, vs = v8.scales_for(c["Hkv"])
    nk = sum(c["lk"])
    k8 = np.full(c["k"].shape, v8.NAN8, np.uint8)
    v8c = k8.copy()
    k8[:nk] = f8.encode(c["k"][:nk] / ks[None, :, None])
    v8c[:nk] = f8.encode(c["v"][:nk] / vs[None, :, None])
    c.update(k=f8.decode(k8), v=f8.decode(v8c), k8=k8, v8=v8c, k_scale=ks, v_scale=vs)
    scaled = c["k"] * ks[None, :, None]
    c["spikes"] = measured_lifts(c["q"], scaled, VARLEN_KINDS, d, c["lk"][0])
    return c


def varlen_fp8_cache(c, ncap=512):
    lk = c["lk"]
    import varlen_cache_fp8_inputs as v8
    kc, vc = (np.full((len(lk), c["Hkv"], ncap, c["d"]), v8.NAN8, np.uint8) for _ in range(2))
    for b, (sk, ek) in enumerate(vi.bounds(c["cu_k"], sum(lk))):
        kc[b, :, :ek - sk] = c["k8"][sk:ek].transpose(1, 0, 2)
        vc[b, :, :ek - sk] = c["v8"][sk:ek].transpose(1, 0, 2)
    return kc, vc, np.array(lk, np.int32)
