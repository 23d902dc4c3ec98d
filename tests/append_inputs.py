"""Inputs and expected results for the KV-cache append tests (tests/test_gpu_kvcache_append.py, tests/test_append_inputs.py): the
placement rules of fa_kvcache_append restated as plain numpy indexing, block tables with room for the appended tokens, and the
value set that drives the e4m3fn quantisation through every code and every tie.  Pure numpy; nothing here touches a GPU.

Placement, from include/fa_mi355.h: L_b = min(max(lens[b], 0), Ncap) (None: 0); token t of sequence b goes to position p = L_b + t;
p >= Ncap is dropped; on a paged cache p is row p % ps of page table[b][p // ps], and a page number outside [0, num_pages) drops the
token.  Everything else in the cache or pool stays as it was.
"""
import numpy as np

import common_inputs as cm
import fp8_inputs as f8

# the common shape of the GPU tier: empty, mid-page, nearly full, full, clamped up, clamped down
SHAPE = dict(B=6, Hkv=2, Ncap=128)
LENS = (0, 17, 123, 128, -3, 1000)


def start_lens(lens, B, ncap):
    return [0] * B if lens is None else [cm.clamp(L, ncap) for L in lens]


def lens_after(lens, B, nnew, ncap):
    """what seqlens_out receives: min(L_b + Nnew, Ncap)"""
    return np.array([min(L + nnew, ncap) for L in start_lens(lens, B, ncap)], np.int32)


def expected_contiguous(cache, new, lens):
    """cache [B, Hkv, Ncap, d], new [B, Hkv, Nnew, d] of one dtype -> the cache after the append (a copy)"""
    out = np.array(cache)
    B, _, ncap, _ = cache.shape
    for b, L in enumerate(start_lens(lens, B, ncap)):
        for t in range(new.shape[2]):
            p = L + t
            if p < ncap:
                out[b, :, p] = new[b, :, t]
    return out


def expected_paged(pool, new, lens, table):
    """pool [num_pages, Hkv, ps, d], new [B, Hkv, Nnew, d], table [B, max_pages] -> the pool after the append (a copy)"""
    out = np.array(pool)
    num_pages, _, ps, _ = pool.shape
    B, max_pages = table.shape
    ncap = max_pages * ps
    for b, L in enumerate(start_lens(lens, B, ncap)):
        for t in range(new.shape[2]):
            p = L + t
            if p >= ncap:
                continue
            page = int(table[b, p // ps])
            if 0 <= page < num_pages:
                out[page, :, p % ps] = new[b, :, t]
    return out


def make_table(lens, B, ncap, nnew, ps, seed, spare=3):
    """-> (table [B, max_pages] int32, num_pages).  The method of tests/decode_inputs.py::scatter: pages dealt out by a seeded
    permutation of a pool with `spare` pages more than B * max_pages.  Live: every page below the length AFTER the append (pages the
    sequence already fills and pages the new tokens reach); every other entry holds garbage."""
    max_pages = ncap // ps
    assert max_pages * ps == ncap
    num_pages = B * max_pages + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    table = np.empty((B, max_pages), np.int32)
    after = lens_after(lens, B, nnew, ncap)
    nxt = 0
    for b in range(B):
        for pi in range(max_pages):
            if pi * ps >= after[b]:
                table[b, pi] = cm.GARBAGE[pi % 2]
            else:
                table[b, pi] = perm[nxt]
                nxt += 1
    return table, num_pages


def written_pages(lens, B, ncap, nnew, ps):
    """{(b, page index)} of the table entries that receive at least one kept token"""
    out = set()
    for b, L in enumerate(start_lens(lens, B, ncap)):
        out |= {(b, p // ps) for p in range(L, min(L + nnew, ncap))}
    return out


def random_bytes(shape, itemsize, seed):
    """seeded random bits as uint16 (itemsize 2) or uint8 (itemsize 1): every pattern, NaN payloads included"""
    rng = np.random.default_rng(seed)
    if itemsize == 2:
        return rng.integers(0, 1 << 16, shape, dtype=np.uint16)
    return rng.integers(0, 1 << 8, shape, dtype=np.uint8)


# ---- the fp8 value set ------------------------------------------------------------------------------------------------------------
FP8_EXTRAS = (456.0, 464.0, 480.0, 1000.0, 65504.0)   # between 448 and the next would-be value, its midpoint, and far beyond


def fp8_magnitudes():
    """every non-negative e4m3fn magnitude (codes 0x00 .. 0x7E), ascending"""
    return f8.TABLE[:0x7F].astype(np.float64)


def fp8_midpoints():
    """the midpoint between every two adjacent magnitudes: the ties of round-to-nearest-even (126 of them)"""
    m = fp8_magnitudes()
    return (m[:-1] + m[1:]) / 2


def fp8_value_set():
    """-> float64 [516]: magnitudes, midpoints and FP8_EXTRAS, both signs of each (+0 and -0 too)"""
    pos = np.concatenate([fp8_magnitudes(), fp8_midpoints(), np.array(FP8_EXTRAS)])
    return np.concatenate([pos, -pos])


def round16_bits(x, fmt):
    """fp32 values -> the uint16 encodings of their fp16 (fmt 0) or bf16 (fmt 1) roundings, to nearest even; no NaN expected"""
    x = np.asarray(x, np.float32)
    if fmt == 0:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen16(bits, fmt):
    """uint16 encodings -> fp32 values, exact"""
    bits = np.asarray(bits, np.uint16)
    if fmt == 0:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def fp8_sources(scale, fmt):
    """the value set times `scale`, rounded to the 16-bit format: what a caller holds before the append divides by the scale again.
    -> (uint16 encodings [516], their fp32 values)"""
    with np.errstate(over="ignore"):
        bits = round16_bits((fp8_value_set() * float(scale)).astype(np.float32), fmt)
    return bits, widen16(bits, fmt)


def fp8_ties(x, scale):
    """how many of the fp32 sources x, divided by the fp32 scale, are exactly a midpoint between two adjacent magnitudes"""
    q = np.abs(np.asarray(x, np.float32) / np.float32(scale)).astype(np.float64)
    return int(np.isin(q, fp8_midpoints()).sum())


def fp8_new_rows(B, Hkv, nnew, d, scales, fmt, seed):
    """New rows [B, Hkv, Nnew, d] (uint16 encodings) for an fp8 append: head h holds fp8_sources(scales[h]) in a seeded shuffle,
    repeated to fill the head."""
    out = np.empty((B, Hkv, nnew, d), np.uint16)
    rng = np.random.default_rng(seed)
    for h in range(Hkv):
        bits, _ = fp8_sources(scales[h], fmt)
        for b in range(B):
            flat = np.resize(bits, nnew * d)
            rng.shuffle(flat)
            out[b, h] = flat.reshape(nnew, d)
    return out
