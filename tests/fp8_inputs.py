"""Inputs for the fp8 KV-cache decode tests (tests/test_gpu_kvcache_fp8.py, tests/test_kvcache_fp8_host.py): the OCP e4m3fn format
restated from its definition, independent of torch and of the library, and builders for caches whose bytes run through every
finite code (their poison and page scatter are tests/common_inputs.py's, with the NaN code 0x7F).  Pure numpy;
tests/test_fp8_inputs.py checks it against torch's CPU conversion without a GPU.

OCP e4m3fn: 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits.  Exponent field 0: subnormals, m / 8 * 2^-6.  No infinities: the
exponent field 15 holds ordinary numbers up to 1.75 * 2^8 = 448, except mantissa 7 (codes 0x7F and 0xFF), which is NaN.
"""
import numpy as np

BIAS, MANT_BITS = 7, 3
NAN_CODES = (0x7F, 0xFF)
MAX = 448.0            # code 0x7E
MIN_SUBNORMAL = 2.0 ** -9
MIN_NORMAL = 2.0 ** -6
REL_EPS = 2.0 ** -4    # largest relative rounding error of a value that is normal in e4m3fn: half an ulp of 2^-3


def _decode_one(code):
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> MANT_BITS) & 0xF, code & 0x7
    if e == 0xF and m == 0x7:
        return float("nan")
    if e == 0:
        return sign * (m / 8.0) * 2.0 ** (1 - BIAS)
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - BIAS)


TABLE = np.array([_decode_one(c) for c in range(256)], np.float32)   # code -> value
TABLE.setflags(write=False)
FINITE_CODES = np.array([c for c in range(256) if c not in NAN_CODES], np.uint8)   # 254 codes, +0 and -0 among them
FINITE_CODES.setflags(write=False)


def decode(codes):
    """uint8 codes -> fp32 values (exact: every e4m3fn value is an fp32 value)"""
    return TABLE[np.asarray(codes, np.uint8)]


def encode(x):
    """fp32 values -> uint8 codes: round to nearest, ties to the even mantissa, saturating at +-448; NaN -> 0x7F."""
    x = np.asarray(x, np.float64)
    mags = TABLE[:0x7F].astype(np.float64)            # codes 0 .. 0x7E: the non-negative values, ascending
    a = np.minimum(np.abs(np.nan_to_num(x, nan=0.0)), MAX)
    hi = np.clip(np.searchsorted(mags, a, side="left"), 1, 0x7E)   # first code with a value >= a
    lo = hi - 1
    d_lo, d_hi = a - mags[lo], mags[hi] - a
    code = np.where(d_lo < d_hi, lo, np.where(d_hi < d_lo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a == 0.0, 0, code).astype(np.uint8)
    code |= (np.signbit(x).astype(np.uint8) << 7)
    return np.where(np.isnan(x), np.uint8(0x7F), code).astype(np.uint8)


def all_codes(shape, seed):
    """uint8 array of `shape` whose bytes run through all 254 finite codes, as evenly as the size allows, in a seeded shuffle"""
    n = int(np.prod(shape))
    assert n >= FINITE_CODES.size, "too small to hold every finite code"
    rng = np.random.default_rng(seed)
    flat = np.resize(FINITE_CODES, n)
    rng.shuffle(flat)
    return flat.reshape(shape)


def all_codes_cache(B, Hkv, Ncap, d, lens, seed):
    """Cache [B, Hkv, Ncap, d] of codes: every head's rows below its sequence's length run through all finite codes where they can
    hold them (a length of 1 holds d codes); rows at and past the length hold the NaN code 0x7F."""
    out = np.full((B, Hkv, Ncap, d), NAN_CODES[0], np.uint8)
    for b in range(B):
        L = min(max(int(lens[b]), 0), Ncap)
        for h in range(Hkv):
            if L * d >= FINITE_CODES.size:
                out[b, h, :L] = all_codes((L, d), seed + 131 * b + h)
            elif L:
                out[b, h, :L] = np.random.default_rng(seed + 131 * b + h).choice(FINITE_CODES, (L, d), replace=False)
    return out
