"""Inputs and the numpy model of fa_kvcache_commit (tests/test_commit_inputs.py, tests/test_gpu_kvcache_commit.py).  Pure numpy;
nothing here touches a GPU.

The rule, from include/fa_mi355.h: cap = Ncap or max_pages * page_size; L_b = clamp(seqlens_k[b], 0, cap) (no lengths: 0); w_b = the
word restricted to the bits i < max_new with L_b + i < cap; a_b = popcount(w_b); with i_0 < i_1 < ... the set bits of w_b, row
L_b + i_j goes to row L_b + j in every head of K and of V, as if every source were read before any destination is written; a move
with i_j == j touches nothing, not even the table; a move whose source or destination page is outside [0, num_pages) is skipped and
still counts; seqlens_out[b] = L_b + a_b.

Two batches of B = 6 sequences, Hkv = 2, Ncap = 128 or pages of 16: "wide" (max_new = 64) and "narrow" (max_new = 8, every word with
bits at and above bit 8).  Between them: the words 0, a prefix, {1,3}, {0,2,5,6}, bit 63 alone and all 64 bits; a sequence 3 below the
capacity, so that bits are dropped there; sequences at L = 13, so that moves cross the boundary of a page of 16; raw lengths below 0
and above the capacity.  A paged form comes with two tables: "good" names a page in every entry; "holes" keeps only the entries the
rule reads and puts garbage in all others -- the whole row of a sequence whose word is a prefix -- and, in one sequence of each
batch, in an entry the rule does read, so that a move is skipped.  The pools have three guard pages that no entry names.
"""
import functools

import numpy as np

import common_inputs as cm

B, HKV, NCAP, PS = 6, 2, 128, 16
MAX_PAGES = NCAP // PS
NUM_PAGES = B * MAX_PAGES + 3
ALL = (1 << 64) - 1


def _w(*bits):
    return sum(1 << i for i in bits)


CASES = {
    "wide": dict(max_new=64,
                 words=(0, _w(0, 1, 2, 3, 4), _w(1, 3), _w(0, 2, 5, 6), _w(63), ALL),
                 lens=(20, 40, 13, NCAP - 3, 30, 64),
                 bad=((4, 5),)),           # (sequence, page): the SOURCE page of the move 93 -> 30
    "narrow": dict(max_new=8,
                   words=(_w(0, 2, 5, 6, 9, 12, 40, 63), _w(0, 2, 3, 8), _w(0, 3, 8, 33, 62), _w(0, 1, 2, 10), _w(2, 7, 8, 9), ALL),
                   lens=(13, 47, -5, NCAP - 3, NCAP - 6, 1000),
                   bad=((0, 0),)),         # the DESTINATION page of 15 -> 14 and 18 -> 15; 19 -> 16 stays
}
NAMES = tuple(CASES)
LENS_MODES = ("in_place", "disjoint", "null")
FORMS = [(paged, fp8) for paged in (False, True) for fp8 in (False, True)]


def form_id(paged, fp8):
    return ("paged" if paged else "contiguous") + ("_fp8" if fp8 else "_16bit")


def right_moves(word, L, max_new, cap):
    """the (source slot, destination slot) pairs of one sequence by the rule, identity moves included"""
    bits = [i for i in range(max_new) if (int(word) >> i) & 1 and L + i < cap]
    return [(L + i, L + j) for j, i in enumerate(bits)]


@functools.lru_cache(maxsize=None)
def inputs(name, d, paged, fp8, table="good", lens_mode="in_place"):
    """-> dict(k0, v0 [B,Hkv,Ncap,d] or pools [num_pages,Hkv,16,d] of uint16 encodings or uint8 codes, words uint64 [B], lens (a
    tuple, or None: no lengths), table int32 [B, max_pages] or None, max_new).  Every byte of the caches is random, so NaN patterns
    (16 bit: about one value in 32; e4m3fn: 0x7F and 0xFF) and all their payloads occur, and every row differs from every other.
    Arrays are read-only."""
    c = CASES[name]
    rng = np.random.default_rng(9900 + NAMES.index(name) * 8 + d // 64 + 2 * paged + 4 * fp8)
    shape = (NUM_PAGES, HKV, PS, d) if paged else (B, HKV, NCAP, d)
    dt, top = (np.uint8, 256) if fp8 else (np.uint16, 65536)
    k0, v0 = (rng.integers(0, top, shape).astype(dt) for _ in range(2))
    lens = None if lens_mode == "null" else c["lens"]
    tb = None
    if paged:
        tb = np.random.default_rng(9950 + NAMES.index(name)).permutation(NUM_PAGES)[:B * MAX_PAGES].astype(np.int32).reshape(B, MAX_PAGES)
        if table == "holes":
            garbage = cm.GARBAGE + (NUM_PAGES, cm.INT_MIN)
            for b in range(B):
                L = 0 if lens is None else cm.clamp(lens[b], NCAP)
                read = {p // PS for s, t in right_moves(c["words"][b], L, c["max_new"], NCAP) if s != t for p in (s, t)}
                for pi in range(MAX_PAGES):
                    if pi not in read or (b, pi) in c["bad"]:
                        tb[b, pi] = garbage[(b + pi) % len(garbage)]
        else:
            assert table == "good"
    x = dict(k0=k0, v0=v0, words=np.array([w & ALL for w in c["words"]], np.uint64), lens=lens, table=tb, max_new=c["max_new"])
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
WRONG = ("no_barrier", "no_compaction", "dropped_counted", "rank_off_by_one", "high32_dropped", "bits_ge_max_new_honoured", "k_only",
         "head0_only", "dst_through_src_page", "identity_needs_its_page")


def model(k0, v0, words, lens, max_new, table=None, wrong=None):
    """what the entry leaves -> (k, v, lens_out int32 [B]).  wrong: one of WRONG in the place of the rule:
      no_barrier               the moves in place in DESCENDING order: what stores that do not wait for every load can give
      no_compaction            destination L_b + i: nothing moves, the lengths are the rule's
      dropped_counted          the bits of tokens dropped at the capacity count in a_b
      rank_off_by_one          destination j takes the source of rank j + 1
      high32_dropped           the word read as 32 bits
      bits_ge_max_new_honoured no restriction to max_new
      k_only, head0_only       V, resp. every head but 0, left alone
      dst_through_src_page     (paged) the destination row addressed through the source slot's table entry
      identity_needs_its_page  (paged) identity moves go through the table too.  Rewriting a row with its own bytes is invisible, so the
                               visible form is taken: a bad entry under an identity move cancels the sequence's other moves"""
    k, v = np.array(k0), np.array(v0)
    paged = table is not None
    ps, pool_pages = k.shape[2], k.shape[0]
    cap = table.shape[1] * ps if paged else k.shape[2]
    out = np.zeros(len(words), np.int32)
    for b in range(len(words)):
        L = 0 if lens is None else cm.clamp(lens[b], cap)
        w = int(words[b])
        if wrong == "high32_dropped":
            w &= 0xFFFFFFFF
        named = [i for i in range(64 if wrong == "bits_ge_max_new_honoured" else max_new) if (w >> i) & 1]
        bits = [i for i in named if L + i < cap]
        out[b] = L + (len(named) if wrong == "dropped_counted" else len(bits))
        moves = [(L + i, L + j) for j, i in enumerate(bits)]
        if wrong == "rank_off_by_one":
            moves = [(L + bits[j + 1], L + j) for j in range(len(bits) - 1)]
        if wrong == "no_compaction":
            moves = []

        def loc(p, via=None):
            if not paged:
                return b, p
            e = int(table[b, (p if via is None else via) // ps])
            return (e, p % ps) if 0 <= e < pool_pages else None

        todo = []
        for s, t in moves:
            if s == t:
                continue
            ls, ld = loc(s), loc(t, s if wrong == "dst_through_src_page" else None)
            if ls is not None and ld is not None:
                todo.append((ls, ld))
        if wrong == "identity_needs_its_page" and any(s == t and loc(s) is None for s, t in moves):
            todo = []
        for arr in ((k,) if wrong == "k_only" else (k, v)):
            for h in ((0,) if wrong == "head0_only" else range(arr.shape[1])):
                if wrong == "no_barrier":
                    for ls, ld in reversed(todo):
                        arr[ld[0], h, ld[1]] = arr[ls[0], h, ls[1]]
                else:
                    rows = [arr[ls[0], h, ls[1]].copy() for ls, _ in todo]
                    for (_, ld), r in zip(todo, rows):
                        arr[ld[0], h, ld[1]] = r
    return k, v, out


def brute(k0, v0, words, lens, max_new, table=None):
    """the same by one sequential pass in ASCENDING order, in place, element loops only: i_j >= j, so no source is overwritten before
    it is read"""
    k, v = np.array(k0), np.array(v0)
    ps = k.shape[2]
    cap = ps * table.shape[1] if table is not None else k.shape[2]
    out = []
    for b, word in enumerate(words):
        L = 0 if lens is None else min(max(int(lens[b]), 0), cap)
        j = 0
        for i in range(64):
            if i >= max_new or L + i >= cap or not (int(word) >> i) & 1:
                continue
            src, dst = L + i, L + j
            j += 1
            if src == dst:
                continue
            if table is None:
                for arr in (k, v):
                    for h in range(arr.shape[1]):
                        arr[b, h, dst] = arr[b, h, src]
                continue
            es, ed = int(table[b, src // ps]), int(table[b, dst // ps])
            if not (0 <= es < k.shape[0] and 0 <= ed < k.shape[0]):
                continue
            for arr in (k, v):
                for h in range(arr.shape[1]):
                    arr[ed, h, dst % ps] = arr[es, h, src % ps]
        out.append(L + j)
    return k, v, np.array(out, np.int32)


def expected(name, d, paged, fp8, table="good", lens_mode="in_place", wrong=None):
    x = inputs(name, d, paged, fp8, table, lens_mode)
    return model(x["k0"], x["v0"], x["words"], x["lens"], x["max_new"], x["table"], wrong)


def gpu_cases(paged):
    """the (name, table, lens_mode) runs of the GPU tier for one form: both batches, in-place, disjoint and no lengths, and on pages both
    tables"""
    tables = ("good", "holes") if paged else ("good",)
    return [(n, t, m) for n in NAMES for t in tables for m in LENS_MODES]
