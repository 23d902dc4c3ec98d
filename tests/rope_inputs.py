"""Inputs and expected results for the rotary-append tests (tests/test_gpu_kvcache_append_rope.py, tests/test_rope_inputs.py): the
arithmetic of the fa_kvcache_append*_rope entries restated in numpy, the cos / sin tables the tests use, and inputs on which a fused
multiply-add changes the stored bytes.  Pure numpy; nothing here touches a GPU.

The contract, from include/fa_mi355.h: token t of sequence b sits at p = L_b + t (L_b clamped to [0, Ncap], None: 0) and uses table
row r = min(p, max_pos - 1).  Half-split: pair i is (x[i], x[i + rot_dim/2]); interleaved: (x[2i], x[2i+1]); both use cos[r][i],
sin[r][i].  y1 = fp32(x1*c) - fp32(x2*s), y2 = fp32(x2*c) + fp32(x1*s): every product and every sum rounded to fp32 on its own (what
numpy's float32 operators do), then ONE rounding to the 16-bit type -- or, for an fp8 cache, the fp32 value divided by the head's
scale, clamped and rounded to e4m3fn.  Elements [rot_dim, d) pass through.  Placement is append_inputs'.
"""
import numpy as np

import append_inputs as ai
import fp8_inputs as f8


# ---- positions and table rows -------------------------------------------------------------------------------------------------------
def positions(lens, B, ncap, nnew):
    """-> int64 [B, Nnew]: p = L_b + t, dropped tokens (p >= Ncap) included: their Q rows are rotated too"""
    return np.array([[L + t for t in range(nnew)] for L in ai.start_lens(lens, B, ncap)], np.int64).reshape(B, nnew)


def table_rows(pos, max_pos):
    """the table row of every position: min(p, max_pos - 1)"""
    return np.minimum(np.asarray(pos, np.int64), max_pos - 1)


# ---- the rotation -------------------------------------------------------------------------------------------------------------------
def pair_slices(rot_dim, interleaved):
    """-> (index of x1 of pair i, index of x2 of pair i), i = 0 .. rot_dim/2 - 1"""
    half = rot_dim // 2
    i = np.arange(half)
    return (2 * i, 2 * i + 1) if interleaved else (i, i + half)


def rotate_fp32(x, cos, sin, interleaved):
    """x fp32 [..., d]; cos, sin fp32 [..., rot_dim/2], broadcast against x's leading axes -> fp32 [..., d]: the rotated part in
    stepwise fp32, elements [rot_dim, d) as they are."""
    x = np.asarray(x, np.float32)
    cos, sin = np.asarray(cos, np.float32), np.asarray(sin, np.float32)
    i1, i2 = pair_slices(2 * cos.shape[-1], interleaved)
    x1, x2 = x[..., i1], x[..., i2]
    y = x.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = x1 * cos, x2 * sin      # float32 * float32 -> float32: each product rounded on its own
        y[..., i1] = a - b
        a, b = x2 * cos, x1 * sin
        y[..., i2] = a + b
    assert y.dtype == np.float32
    return y


def rotated_rows_fp32(bits, fmt, lens, ncap, cos, sin, interleaved):
    """Rows [B, H, Nnew, d] (uint16 encodings; H any multiple of the K/V heads: K and Q alike) -> their fp32 rotation at
    p = L_b + t with the clamped table row, [B, H, Nnew, d]."""
    B, _, nnew, _ = bits.shape
    r = table_rows(positions(lens, B, ncap, nnew), cos.shape[0])            # [B, Nnew]
    return rotate_fp32(ai.widen16(bits, fmt), cos[r][:, None], sin[r][:, None], interleaved)


def rotated_rows16(bits, fmt, lens, ncap, cos, sin, interleaved):
    """The same, as the 16-bit encodings Q and a 16-bit cache receive: the rotated part rounded once to nearest even, the
    pass-through part with every bit of the source (NaN payloads included)."""
    rot_dim = 2 * cos.shape[1]
    y = rotated_rows_fp32(bits, fmt, lens, ncap, cos, sin, interleaved)
    out = np.array(bits, np.uint16)
    out[..., :rot_dim] = ai.round16_bits(y[..., :rot_dim], fmt)
    return out


def fp8_codes(y, scales):
    """fp32 rows [*, Hkv, N, d] -> the codes an fp8 cache receives: e4m3fn_RNE(clamp(y / scale[h], +-448)) with an fp32 division;
    scales None: 1.0.  The recipe of fa.quantize_kv_fp8, restated on tests/fp8_inputs.py's encoder."""
    y = np.asarray(y, np.float32)
    sc = np.ones(y.shape[1], np.float32) if scales is None else np.asarray(scales, np.float32)
    q = y / sc.reshape(1, -1, 1, 1)
    assert q.dtype == np.float32
    return f8.encode(np.clip(q, -f8.MAX, f8.MAX))


def expected_cache(cache, rows, lens, table=None):
    """The cache [B, Hkv, Ncap, d] (table None) or pool [num_pages, Hkv, ps, d] after the append of `rows` (already rotated, in the
    cache's element type): append_inputs' placement."""
    return ai.expected_contiguous(cache, rows, lens) if table is None else ai.expected_paged(cache, rows, lens, table)


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def scrambled_table(max_pos, half, seed):
    """-> (cos, sin) fp32 [max_pos, half]: every one of the 2 * max_pos * half entries a DISTINCT seeded uniform(-1, 1) value, so a
    wrong position, pair index or head divisor changes bytes."""
    rng = np.random.default_rng(seed)
    n = 2 * max_pos * half
    vals = np.unique(rng.uniform(-1.0, 1.0, 2 * n + 64).astype(np.float32))
    vals = vals[(vals > -1.0) & (vals < 1.0) & (vals != 0.0)]
    assert vals.size >= n
    vals = rng.permutation(vals)[:n]
    assert np.unique(vals).size == n
    return vals[:n // 2].reshape(max_pos, half).copy(), vals[n // 2:].reshape(max_pos, half).copy()


def identity_table(max_pos, half):
    """cos = 1, sin = 0: the rotation of the identity -- still not a plain copy (x1 = -0 and a negative x2: -0 - (-0) = +0)"""
    return np.ones((max_pos, half), np.float32), np.zeros((max_pos, half), np.float32)


def real_table(max_pos, rot_dim, theta=10000.0):
    """the table of a model: angle(p, i) = p * theta^(-2i / rot_dim), computed in float64 and rounded to fp32"""
    inv_freq = theta ** (-np.arange(0, rot_dim, 2, dtype=np.float64) / rot_dim)
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * inv_freq[None]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


# ---- inputs a fused multiply-add gets wrong -----------------------------------------------------------------------------------------
def pinned_y1(x1, x2, c, s):
    """fp32(x1*c) - fp32(x2*s), stepwise"""
    x1, x2, c, s = (np.asarray(a, np.float32) for a in (x1, x2, c, s))
    return (x1 * c) - (x2 * s)


def contracted_y1(x1, x2, c, s):
    """What a compiler that contracts a*b + c makes of y1, emulated in float64 (a product of two fp32 is exact there):
    -> (fma(x1, c, -fp32(x2*s)), fma(-x2, s, fp32(x1*c))) as fp32"""
    x1, x2, c, s = (np.asarray(a, np.float32) for a in (x1, x2, c, s))
    f = np.float64
    a = (x1.astype(f) * c.astype(f) - (x2 * s).astype(f)).astype(np.float32)
    b = (-(x2.astype(f)) * s.astype(f) + (x1 * c).astype(f)).astype(np.float32)
    return a, b


def contraction_witnesses(fmt, n, seed=7, draws=1 << 22):
    """Seeded rejection sampling of (x1, x2, c, s): x from N(0, 1) rounded to the 16-bit format, c and s uniform(-1, 1) fp32.
    -> (A, B), fp32 [n, 4] each: tuples whose pinned y1 and whose contracted y1 -- A: fma(x1, c, -fp32(x2*s)); B:
    fma(-x2, s, fp32(x1*c)) -- differ AFTER the rounding to the 16-bit format.  On ordinary data that is about one element in
    30 000, which is why the GPU tier places these."""
    rng = np.random.default_rng(seed)
    x1 = ai.widen16(ai.round16_bits(rng.standard_normal(draws).astype(np.float32), fmt), fmt)
    x2 = ai.widen16(ai.round16_bits(rng.standard_normal(draws).astype(np.float32), fmt), fmt)
    c = rng.uniform(-1.0, 1.0, draws).astype(np.float32)
    s = rng.uniform(-1.0, 1.0, draws).astype(np.float32)
    want = ai.round16_bits(pinned_y1(x1, x2, c, s), fmt)
    out = []
    for got in contracted_y1(x1, x2, c, s):
        idx = np.nonzero(ai.round16_bits(got, fmt) != want)[0]
        assert idx.size >= n, (fmt, idx.size, n)
        idx = idx[:n]
        out.append(np.stack([x1[idx], x2[idx], c[idx], s[idx]], axis=1))
    return out[0], out[1]


def witness_case(fmt, d, rot_dim, interleaved, per_form=64, seed=7):
    """The witnesses as an append: one sequence, one head, lengths (0,), token t at position t.  Pair i of token t holds witness
    t * half + i: its x1, x2 in the row and its c, s in table row t.  Everything outside the rotated part is zero.
    -> (rows uint16 [1, 1, Nnew, d], cos, sin fp32 [Nnew, half])"""
    A, Bw = contraction_witnesses(fmt, per_form, seed)
    w = np.concatenate([A, Bw])
    half = rot_dim // 2
    nnew = w.shape[0] // half
    assert nnew * half == w.shape[0]
    w = w.reshape(nnew, half, 4)
    i1, i2 = pair_slices(rot_dim, interleaved)
    x = np.zeros((nnew, d), np.float32)
    x[:, i1], x[:, i2] = w[:, :, 0], w[:, :, 1]
    bits = ai.round16_bits(x, fmt)
    assert np.array_equal(ai.widen16(bits, fmt), x)   # the witnesses are values of the format
    return bits.reshape(1, 1, nnew, d), np.ascontiguousarray(w[:, :, 2]), np.ascontiguousarray(w[:, :, 3])
