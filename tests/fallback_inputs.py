"""Seeded hostile inputs for tests/test_gpu_fallback_paths.py, and the float64 measurements that show each input forces what
its case is named for (tests/test_fallback_inputs.py asserts them without a GPU; the GPU tests assert them again before they
trust a result).  Pure numpy plus the `oracle` fixture (tests/conftest.py); nothing here touches a GPU.

Scores are in log2 units (q.k * scale * log2 e), the unit of the kernels' references and thresholds, computed in float64
from the 16-bit-rounded values.  A row's LIFT is its largest visible score minus its largest visible score among the keys of
tile 0 (keys 0..63; under the mask `key <= row`): the exact optimistic pass of fa_fwd_rp16_kernel.hpp fixes its reference
at the maximum over the row's first 32 keys + 4, so fp16 weights overflow from a lift of 20 on (4 + 16), bf16 weights are
rejected from 2^96 and overflow past 2^128 (tests/test_gpu_parity.py::test_bf16_overflow_window_below_inf).  The maximum
over 32 keys is at most the one over 64, so a lift over tile 0 is a lower bound of the lift the kernel sees; the rows that
must STAY in a fast pass are measured against the first 32 keys as well (lift32).
"""
import functools

import numpy as np

import common_inputs as cm

LOG2E = 1.4426950408889634
LN2 = float(np.log(2.0))
F16, BF16 = 0, 1

# lifts (log2 units over the visible tile-0 maximum)
LIFT_FAIL = {F16: (40.0, 40.0), BF16: (150.0, 110.0)}   # must leave the fast passes: (overflow, bf16's finite window 2^96..2^127)
LIFT_STAY = 19.0                                          # must stay (below 4 + 16)
ROWS_PER_BLOCK = {64: 512, 128: 256}                      # full-width row block of algos 24 / 28; the redo kernel's is half
CHAIN_N = {64: (600, 800, 1024), 128: (300, 400, 512)}    # second half of block 1: missing / partial / whole


def scores_log2(q, k, b, rows=None):
    """[rows, Nk] float64 log2-scaled scores of head b."""
    d = q.shape[-1]
    qq = q[b].astype(np.float64) if rows is None else q[b][rows].astype(np.float64)
    return (qq @ k[b].astype(np.float64).T) * (LOG2E / np.sqrt(d))


def _visible(s, row0, causal):
    """-inf on the keys a row does not see (s holds rows row0, row0 + 1, ...)."""
    if not causal:
        return s
    rows = row0 + np.arange(s.shape[0])[:, None]
    return np.where(np.arange(s.shape[1])[None, :] <= rows, s, -np.inf)


def lifts(q, k, b, causal, width=64):
    """Per row of head b: (largest visible score) - (largest visible score among the first `width` keys)."""
    s = _visible(scores_log2(q, k, b), 0, causal)
    return s.max(-1) - s[:, :width].max(-1)


def spread_tile0(q, k, b, causal):
    """Per row of head b: (largest, smallest) visible score minus the visible tile-0 maximum."""
    s = scores_log2(q, k, b)
    vis = _visible(s, 0, causal)
    ref = vis[:, :64].max(-1)
    lo = np.where(np.isfinite(vis), s, np.inf).min(-1)
    return vis.max(-1) - ref, lo - ref


def spike(q, k, b, row, key, lift_log2, causal):
    """The spike() of test_optimistic_pass_overflow_fallback with the reference taken over the keys of tile 0 that the row
    SEES: key `key` of head b becomes a multiple of query row `row` whose score lies lift_log2 log2 units above that maximum."""
    d = q.shape[-1]
    assert key >= 64 and (not causal or key <= row), "the spiked key lies behind tile 0 and is visible to its row"
    last = min(row, 63) if causal else 63
    s0 = (q[b, row] @ k[b, :last + 1].T) / np.sqrt(d)
    target = (s0.max() + lift_log2 * LN2) * np.sqrt(d)
    k[b, key] = q[b, row] * (target / float(q[b, row] @ q[b, row]))


def _round(oracle, fmt, *xs):
    vals = tuple(oracle.decode16(oracle.encode16(x, fmt), fmt) for x in xs)
    bits = tuple(oracle.encode16(x, fmt) for x in vals)
    for a in vals + bits:
        a.setflags(write=False)
    return vals, bits


# ---- A. the fallback chain under the mask ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case(oracle, d, n, fmt):
    """Three heads of n rows, one launch with every kind of row block (R = ROWS_PER_BLOCK[d] rows, halves of R/2):
      head 0  benign N(0,1); its block 1 holds the must-stay row (lift 19, key two before the diagonal).  (Head 1 has two
              row blocks and needs both for rows that must fail, so the must-stay row sits in the benign head: its block is
              still one a fast pass has to keep.)
      head 1  block 0: one spiked row in the FIRST half only (the workgroup marks both halves for it);
              block 1: a spike on the diagonal (key == row, inside the masked tile) and one on the last visible key of the
              last row of the sequence
      head 2  every key after tile 0 x 6, and key R/2 + 10 made huge (x 200 fp16, x 1e5 bf16 -- beyond fp16's range):
              invisible to every row before it
    -> dict: q, k, v (16-bit-rounded fp32), bits, spikes [(b, row, key, lift)], stay (b, row, key), future_key,
       rows (R), fail [3, blocks] bool: the blocks built to leave the fast passes."""
    R = ROWS_PER_BLOCK[d]
    assert R < n <= 2 * R
    (q, k, v), _ = oracle.make_qkv(3, n, d, fmt, seed=1300 + 2 * d + n + fmt)
    q, k, v = q.copy(), k.copy(), v.copy()
    hi, window = LIFT_FAIL[fmt]
    spikes = [(1, R // 4 + 3, 65, hi), (1, R + 40, R + 40, window), (1, n - 1, n - 1, hi)]
    # the must-stay row: the first one from R + 20 on whose tile-0 maximum lies among its first 32 keys, so that the lift the
    # kernel sees (over 32 keys) is the lift it was built with (over 64)
    srow = next(r for r in range(R + 20, n) if int(np.argmax(q[0, r] @ k[0, :64].T)) < 32)
    stay = (0, srow, srow - 2)
    for (b, row, key, lift) in spikes:
        spike(q, k, b, row, key, lift, True)
    spike(q, k, stay[0], stay[1], stay[2], LIFT_STAY, True)
    future_key = R // 2 + 10
    k[2, 64:] *= 6.0
    k[2, future_key] *= 200.0 if fmt == F16 else 1e5
    (q, k, v), bits = _round(oracle, fmt, q, k, v)
    fail = np.zeros((3, (n + R - 1) // R), bool)
    fail[1:] = True
    return dict(q=q, k=k, v=v, bits=bits, spikes=spikes, stay=stay, future_key=future_key, rows=R, fail=fail, causal=True)


def large_grid_case(oracle, bh, n, d, fmt):
    """More row blocks (and more redo half-blocks) than CUs: every third head (b % 3 == 1) has one spiked row in each of its
    row blocks -- off the diagonal in block 0, on it in the last block -- so marked and unmarked blocks interleave in both
    directions of the causal grid's alternation.  (Not cached: a case holds about 200 MB and each tier uses it once.)"""
    R = ROWS_PER_BLOCK[d]
    (q, k, v), _ = oracle.make_qkv(bh, n, d, fmt, seed=1700 + d + fmt)
    k = k.copy()
    spikes = []
    for b in range(1, bh, 3):
        for blk in range((n + R - 1) // R):
            r0, r1 = blk * R, min(n, (blk + 1) * R)
            row = max(r0, 70) + (b * 13) % (r1 - max(r0, 70))
            key = row if blk else 64 + (b * 7) % (row - 63)
            spike(q, k, b, row, key, LIFT_FAIL[fmt][0], True)
            spikes.append((b, row, key, LIFT_FAIL[fmt][0]))
    (q, k, v), bits = _round(oracle, fmt, q, k, v)
    return dict(q=q, k=k, v=v, bits=bits, spikes=spikes, rows=R, causal=True)


@functools.lru_cache(maxsize=None)
def plain_case(oracle, d, n, fmt):
    """No mask.  d = 64: the two inputs of test_optimistic_pass_overflow_fallback (n = 640: three heads; n = 333: one head, the
    overflow in the partial last tile), value for value.  d = 128: their counterpart on 256-row blocks at n = 300 / 400 (block
    1's second half missing / partial): head 0 a lift-40 row on the last key and a must-stay row in block 1, head 1 a row just
    above the overflow point and one far above it in block 1, head 2 every key after tile 0 x 6."""
    far = 150.0 if fmt == BF16 else 60.0
    if d == 64 and n == 333:
        (q, k, v), _ = oracle.make_qkv(1, n, d, fmt, seed=9)
        k = k.copy()
        k[0, n - 1] = q[0, 200] * 40.0
        spikes, stay = [], None   # (not built with spike(): its lift is measured, see lifts())
    else:
        (q, k, v), _ = oracle.make_qkv(3, n, d, fmt, seed=777 + fmt + (0 if d == 64 else d + n))
        k = k.copy()
        if d == 64:
            assert n == 640
            spikes, stay = [(0, 5, n - 1, 40.0), (1, 77, 333, 21.5), (1, 78, 334, far)], (0, 300, 100)
            order = [spikes[0], stay + (LIFT_STAY,)] + spikes[1:]   # (the order of the parity test's calls)
        else:
            assert n in (300, 400)
            spikes, stay = [(0, 5, n - 1, 40.0), (1, 77, 200, 21.5), (1, n - 2, 201, far)], (0, 260, 100)
            order = spikes + [stay + (LIFT_STAY,)]
        for (b, row, key, lift) in order:
            spike(q, k, b, row, key, lift, False)
        k[2, 64:] *= 6.0
    (q, k, v), bits = _round(oracle, fmt, q, k, v)
    return dict(q=q, k=k, v=v, bits=bits, spikes=spikes, stay=stay, rows=ROWS_PER_BLOCK[d], causal=False)


# ---- B. split-KV and KV-cache ------------------------------------------------------------------------------------------------
def _orthogonal_rows(x):
    """Gram-Schmidt over the rows of x [rows, d] (rows <= d), norms kept: a key made parallel to one row scores ~0 with the others."""
    out = x.astype(np.float64).copy()
    for i in range(out.shape[0]):
        for j in range(i):
            out[i] -= (out[i] @ out[j]) / (out[j] @ out[j]) * out[j]
        out[i] *= np.linalg.norm(x[i]) / np.linalg.norm(out[i])
    return out.astype(np.float32)


def _set_key(q, k, bq, row, bk, key, score_log2):
    """key `key` of K/V head bk becomes the multiple of q[bq, row] that scores score_log2 with it (negative: antiparallel)."""
    d = q.shape[-1]
    k[bk, key] = q[bq, row] * (score_log2 * LN2 * np.sqrt(d) / float(q[bq, row] @ q[bq, row]))


STAIR_STEP = 7.0   # below kThr = 8 (fa_tile.hpp)
SPLIT_ROWS = ("staircase", "jump 40 in the last split", "jump 150 in the last split", "all but tile 0 below -200", "spike in the partial last tile")


@functools.lru_cache(maxsize=None)
def splitkv_case(oracle, d, fmt, nk):
    """(bh, nq) = (2, 5) against nk keys, one hostile row of each kind of SPLIT_ROWS per head (the query rows of a head are made
    orthogonal, so a key built for one row is benign for the others).  With base = the row's largest benign score:
      row 0  one key per tile 0, 1, 2, ... at base + 7 t: every tile's maximum is < kThr above the one before
      row 1  a key in the last split (among the last 128 keys, before the partial tile) at base + 40
      row 2  the same at base + 150
      row 3  a key in tile 0 at base + 210: every other score is more than 200 below the row's maximum
      row 4  the last key (inside the partial last tile) at base + 40
    Head 1 has the same kinds on other keys.  -> dict with q, k, v, bits, keys {(b, row): [keys]}, stairs (tiles of the staircase)."""
    bh, nq = 2, 5
    (q, _, _), _ = oracle.make_qkv(bh, nq, d, fmt=fmt, seed=2100 + d + fmt)
    (_, k, v), _ = oracle.make_qkv(bh, nk, d, fmt=fmt, seed=2200 + d + fmt + nk)
    q = np.stack([_orthogonal_rows(q[b]) for b in range(bh)])
    k = k.copy()
    tiles = (nk + 63) // 64
    assert nk % 64 != 0 and tiles >= 4
    stairs = min(6, tiles)
    last_full = (tiles - 1) * 64          # first key of the partial last tile
    keys = {}
    for b in range(bh):
        base = scores_log2(q, k, b).max(-1)   # benign maxima (before any key of this head is replaced)
        off = 3 + 11 * b
        keys[b, 0] = [64 * t + (off + t) % (min(64, nk - 64 * t) - 2) for t in range(stairs)]
        keys[b, 1] = [last_full - 100 + off]
        keys[b, 2] = [last_full - 40 + off]
        keys[b, 3] = [20 + off]
        keys[b, 4] = [nk - 1 - b]
        for t, key in enumerate(keys[b, 0]):
            _set_key(q, k, b, 0, b, key, base[0] + STAIR_STEP * t)
        _set_key(q, k, b, 1, b, keys[b, 1][0], base[1] + 40.0)
        _set_key(q, k, b, 2, b, keys[b, 2][0], base[2] + 150.0)
        _set_key(q, k, b, 3, b, keys[b, 3][0], base[3] + 210.0)
        _set_key(q, k, b, 4, b, keys[b, 4][0], base[4] + 40.0)
    (q, k, v), bits = _round(oracle, fmt, q, k, v)
    return dict(q=q, k=k, v=v, bits=bits, keys=keys, stairs=stairs, last_full=last_full)


KV_SHAPE = dict(B=3, Hkv=1, G=2, Nq=5, Ncap=4096)
KV_LENS = (66, 4096, 130)
KV_CUT = 100            # test_lse_merges_spiked_ranges: the dominant key of the full sequence's spiked row lies behind it
KV_SHIFT = 300.0        # log2 units


@functools.lru_cache(maxsize=None)
def kvcache_case(oracle, d, fmt):
    """B, Hkv, G, Nq, Ncap = 3, 1, 2, 5, 4096 with lengths (66, 4096, 130); q [B*G, Nq, d], k, v [B, Ncap, d].
      sequence 0 (66 keys)    under the end-aligned mask keys 64-65 are seen by the last rows only (key 64 by rows 3 and 4, key 65
                              by row 4): key 65 at +40 for (head 0, row 4), key 64 at +150 for (head 1, row 3)
      sequence 1 (4096 keys)  key 4000 (a late split, behind KV_CUT) at +40 for (head 0, row 2)
      sequence 2 (130 keys)   every key carries the same offset along the all-ones direction and so do the queries: head 0
                              against it (every logit about -300 log2 units, lse about -208), head 1 along it (+300).  The
                              random parts are made orthogonal to that direction, so the rows stay as flat as N(0,1) rows.
    The query rows that share a K/V head are made orthogonal to each other first."""
    B, G, Nq, Ncap = KV_SHAPE["B"], KV_SHAPE["G"], KV_SHAPE["Nq"], KV_SHAPE["Ncap"]
    (q, _, _), _ = oracle.make_qkv(B * G, Nq, d, fmt=fmt, seed=2500 + d + fmt)
    (_, k, v), _ = oracle.make_qkv(B, Ncap, d, fmt=fmt, seed=2600 + d + fmt)
    q, k = q.copy(), k.copy()
    for b in range(B):
        q[G * b:G * b + G] = _orthogonal_rows(q[G * b:G * b + G].reshape(G * Nq, d)).reshape(G, Nq, d)
    spikes = [(0, 4, 0, 65, 40.0), (1, 3, 0, 64, 150.0), (2, 2, 1, 4000, 40.0)]   # (query head, row, sequence, key, lift)
    for (h, row, seq, key, lift) in spikes:
        L = KV_LENS[seq]
        base = ((q[h, row].astype(np.float64) @ k[seq, :L].astype(np.float64).T) * (LOG2E / np.sqrt(d))).max()
        _set_key(q, k, h, row, seq, key, base + lift)
    u = np.ones(d, np.float32) / np.sqrt(d)
    alpha = np.sqrt(KV_SHIFT / (LOG2E * np.sqrt(d)))          # per-component offset: d * alpha^2 * scale * log2e = KV_SHIFT
    k[2] -= np.outer(k[2] @ u, u)
    k[2] += alpha
    for h, sign in ((4, -1.0), (5, 1.0)):
        q[h] -= np.outer(q[h] @ u, u)
        q[h] += sign * alpha
    (q, k, v), bits = _round(oracle, fmt, q, k, v)
    return dict(q=q, k=k, v=v, bits=bits, spikes=spikes, shifted=((4, -KV_SHIFT), (5, KV_SHIFT)))


# ---- the forcing conditions: asserted by tests/test_fallback_inputs.py and again by every GPU test that uses the input -------
def fails(lift, fmt):
    """a lift that the exact optimistic pass cannot survive: fp16 from 21 (20 + a margin), bf16 past 2^128 or inside the
    rejected finite window"""
    return lift >= 21.0 if fmt == F16 else (lift >= 129.0 or 96.0 < lift < 127.0)


def lift_at(q, k, b, row, key, causal, width=64):
    """score of (row, key) minus the row's largest visible score among its first `width` keys"""
    s = _visible(scores_log2(q, k, b, rows=slice(row, row + 1)), row, causal)[0]
    return s[key] - s[:width].max()


def assert_spiked_rows(case, fmt, must_fail=True):
    """every spiked key is visible to its row and lies as far above the row's tile-0 maximum as it was built to (must_fail: far
    enough to leave the fast passes); the must-stay key stays below 19.5"""
    q, k, causal = case["q"], case["k"], case["causal"]
    for (b, row, key, lift) in case["spikes"]:
        assert key >= 64 and (not causal or key <= row), (b, row, key)
        got = lift_at(q, k, b, row, key, causal)
        assert abs(got - lift) < 1.0 and fails(got, fmt) == fails(lift, fmt), f"head {b} row {row}: lift {got:.2f}, built for {lift}"
        assert fails(got, fmt) or not must_fail, f"head {b} row {row}: lift {got:.2f} does not force the fallback"
    if case.get("stay"):
        b, row, key = case["stay"]
        assert not causal or key <= row
        got = lift_at(q, k, b, row, key, causal)
        assert 18.0 <= got <= 19.5, f"must-stay row: lift {got:.2f}"


def assert_chain_case(case, fmt):
    q, k, R = case["q"], case["k"], case["rows"]
    n = q.shape[1]
    assert_spiked_rows(case, fmt)
    # head 0: every row but the must-stay one within +-16 of its tile-0 maximum, and below the overflow point of the exact pass
    # measured against the first 32 keys (so each of its blocks CAN be produced by a fast pass)
    hi, lo = spread_tile0(q, k, 0, True)
    benign = np.ones(n, bool)
    benign[case["stay"][1]] = False
    assert hi[benign].max() <= 16.0 and lo[benign].min() >= -16.0, (hi[benign].max(), lo[benign].min())
    assert lifts(q, k, 0, True, width=32).max() <= 19.5
    # head 1: the first-half-only spike really leaves the second half of block 0 (and the rest of the first) to the fast passes
    l1 = lifts(q, k, 1, True, width=32)
    first = case["spikes"][0][1]
    # (a bf16 row is rejected once its sum reaches 2^96, i.e. from a lift of 100 over its first 32 keys)
    assert first < R // 2 and np.delete(l1[:R], first).max() <= (19.5 if fmt == F16 else 90.0), np.delete(l1[:R], first).max()
    # head 2: the huge key is invisible to every row before it (key > row) and visible from its own row on; every block holds a
    # row that must fail
    fk = case["future_key"]
    s2 = _visible(scores_log2(q, k, 2), 0, True)
    assert R // 2 < fk < R and np.isinf(s2[:fk, fk]).all() and np.isfinite(s2[fk:, fk]).all()
    assert np.abs(s2[fk:, fk]).max() >= 1000.0
    l2 = lifts(q, k, 2, True)
    for blk in range(case["fail"].shape[1]):
        assert any(fails(x, fmt) for x in l2[blk * R:(blk + 1) * R]), f"head 2 block {blk}: no row forces the fallback"
    # the diagonal spike sits on the diagonal, the last-row spike on the last key of the last row
    assert case["spikes"][1][1] == case["spikes"][1][2] and case["spikes"][2][1:3] == (n - 1, n - 1)
    # block 1's second half: missing / partial / whole
    assert n in CHAIN_N[q.shape[2]]


def assert_large_grid_case(case, fmt):
    q, k, R = case["q"], case["k"], case["rows"]
    bh, n = q.shape[:2]
    nblk = (n + R - 1) // R
    assert len(case["spikes"]) == len(range(1, bh, 3)) * nblk
    for (b, row, key, lift) in case["spikes"]:
        assert b % 3 == 1 and 64 <= key <= row
        s = _visible(scores_log2(q, k, b, rows=slice(row, row + 1)), row, True)[0]
        got = s.max() - s[:64].max()
        assert fails(got, fmt) and abs(got - lift) < 1.0, (b, row, got)
    assert sorted({(b, row // R) for (b, row, _, _) in case["spikes"]}) == [(b, blk) for b in range(1, bh, 3) for blk in range(nblk)]


def assert_plain_case(case, fmt):
    q, k = case["q"], case["k"]
    assert_spiked_rows(case, fmt, must_fail=False)   # (the lift-21.5 row is "just above" fp16's overflow point only)
    assert any(fails(lift, fmt) for (_, _, _, lift) in case["spikes"]) or not case["spikes"]
    if not case["spikes"]:   # n = 333: the overflow sits on the last key, inside the partial last tile
        n = q.shape[1]
        s = scores_log2(q, k, 0)
        assert n % 64 != 0 and s[200].argmax() == n - 1 and fails(lifts(q, k, 0, False)[200], fmt)
    else:
        l2 = lifts(q, k, 2, False)
        R = case["rows"]
        for blk in range((q.shape[1] + R - 1) // R):
            assert any(fails(x, F16) for x in l2[blk * R:(blk + 1) * R])   # (x 6: beyond fp16's overflow point in every block)


def assert_splitkv_case(case):
    q, k = case["q"], case["k"]
    nk = k.shape[1]
    tiles, last_full = (nk + 63) // 64, case["last_full"]
    for b in range(q.shape[0]):
        s = scores_log2(q, k, b)
        pad = np.full((s.shape[0], tiles * 64 - nk), -np.inf)
        tmax = np.concatenate([s, pad], 1).reshape(s.shape[0], tiles, 64).max(-1)   # [row, tile]
        # row 0: the running maximum rises by less than kThr = 8 from each tile to the next, by more than 20 in total, and not at
        # all behind the staircase
        st = case["stairs"]
        rise = np.diff(tmax[0, :st])
        assert (rise > 0).all() and rise.max() < 8.0 and tmax[0, st - 1] - tmax[0, 0] > 20.0, rise
        assert tmax[0, st:].max(initial=-np.inf) < tmax[0, st - 1]
        assert [int(x) // 64 for x in case["keys"][b, 0]] == list(range(st))
        # rows 1, 2, 4: one key far above every other one
        for row, lift in ((1, 40.0), (2, 150.0), (4, 40.0)):
            key = case["keys"][b, row][0]
            rest = np.delete(s[row], key).max()
            assert s[row].argmax() == key and abs(s[row, key] - rest - lift) < 1.0, (b, row, s[row, key] - rest)
        if nk > 2 * 64 * 4:   # (the split shape) rows 1 and 2: among the last 128 keys in front of the partial tile
            assert all(last_full - 128 <= case["keys"][b, r][0] < last_full for r in (1, 2))
        assert last_full <= case["keys"][b, 4][0] < nk
        # row 3: everything outside tile 0 more than 200 below the row's maximum, which sits in tile 0
        assert s[3].argmax() < 64 and (s[3, 64:] < s[3].max() - 200.0).all()
        # a key built for one row is benign for the others (orthogonal query rows)
        own = {key: row for row in range(5) for key in case["keys"][b, row]}
        for key, row in own.items():
            others = np.delete(s[:, key], row)
            assert np.abs(others).max() < 2.0, (b, key, others)


def assert_kvcache_case(case, causal):
    q, k = case["q"], case["k"]
    G, Nq = KV_SHAPE["G"], KV_SHAPE["Nq"]
    for (h, row, seq, key, lift) in case["spikes"]:
        L = KV_LENS[seq]
        c = cm.row_limits(L, Nq, Nq, causal)[1][row]
        assert key < c, "the spiked key is visible to its row"
        s = scores_log2(q[h:h + 1], k[seq:seq + 1, :c], 0)[row]
        assert s.argmax() == key and abs(s[key] - np.delete(s, key).max() - lift) < 1.0, (h, row, s[key] - np.delete(s, key).max())
    # sequence 0 under the mask: keys 64 and 65 are seen by the last rows only
    assert [c > 64 for c in cm.row_limits(KV_LENS[0], Nq, Nq, True)[1]] == [False, False, False, True, True]
    assert [c > 65 for c in cm.row_limits(KV_LENS[0], Nq, Nq, True)[1]] == [False, False, False, False, True]
    # the full sequence's spike lies behind the cut of the two-range merge, in a late part of the keys
    assert case["spikes"][2][3] >= max(KV_CUT, KV_LENS[1] * 3 // 4)
    for (h, shift) in case["shifted"]:
        seq = h // G
        s = scores_log2(q[h:h + 1], k[seq:seq + 1, :KV_LENS[seq]], 0)
        assert np.abs(s - shift).max() < 16.0, (h, np.abs(s - shift).max())
