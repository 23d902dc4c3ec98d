"""The helpers of tests/append_inputs.py without a GPU: the fp8 value set drives quantize_kv_fp8 through every finite code and every
tie, and on it torch's CPU recipe equals the restated encoder on a correctly rounded fp32 quotient -- the definition the append
kernel is held to bit for bit on the GPU.  The placement helpers are checked on a case small enough to read."""
import numpy as np
import pytest

import append_inputs as ai
import common_inputs as cm
import fp8_inputs as f8

SCALES = (1.0, 0.5, 4.0, 0.37, 1.9)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _torch16(torch, bits, fmt):
    return torch.from_numpy(np.array(bits).view(np.int16)).view(torch.float16 if fmt == 0 else torch.bfloat16)


def test_value_set():
    v = ai.fp8_value_set()
    assert v.size == 2 * (127 + 126 + 5)
    assert np.array_equal(f8.encode(ai.fp8_magnitudes().astype(np.float32)), np.arange(0x7F))
    m = ai.fp8_midpoints()
    assert m.size == 126 and (m > ai.fp8_magnitudes()[:-1]).all() and (m < ai.fp8_magnitudes()[1:]).all()
    assert np.signbit(v).sum() == v.size // 2   # -0 among them


@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("scale", SCALES)
def test_quantize_kv_fp8_is_the_encoder_on_the_fp32_quotient(fa, torch, scale, fmt):
    bits, x = ai.fp8_sources(scale, fmt)
    assert np.array_equal(_torch16(torch, bits, fmt).float().numpy().view(np.uint32), x.view(np.uint32))   # widen16 is torch's widening
    x8, s = fa.quantize_kv_fp8(_torch16(torch, bits, fmt).view(1, 1, -1, 1), torch.tensor([scale], dtype=torch.float32))
    got = x8.view(torch.uint8).numpy().ravel()
    with np.errstate(over="ignore"):
        want = f8.encode(np.float32(x) / np.float32(scale))
    mismatches = int((got != want).sum())
    codes = set(got.tolist())
    ties = ai.fp8_ties(x, scale)
    print(f"scale {scale} fmt {fmt}: {mismatches} mismatches, {len(codes)} codes, {ties} ties")
    assert mismatches == 0
    assert codes == set(f8.FINITE_CODES.tolist())   # all 254 finite codes, and no NaN code
    if scale in (1.0, 0.5, 4.0):
        assert ties >= 252                           # a power of two commutes with the rounding to 16 bits: every tie survives
    # what lies beyond 448 saturates, infinities (65504 * 4 in fp16) included
    big = np.abs(x / np.float32(scale)) >= 448
    assert big.sum() >= 10 and set((got[big] & 0x7F).tolist()) == {0x7E}


def test_round16_is_torchs_rounding(torch):
    x = np.random.default_rng(3).standard_normal(5000).astype(np.float32) * np.float32(50.0)
    x = np.concatenate([x, ai.fp8_value_set().astype(np.float32) * np.float32(0.37)])
    for fmt, dt in ((0, torch.float16), (1, torch.bfloat16)):
        want = torch.from_numpy(x).to(dt).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(ai.round16_bits(x, fmt), want), fmt


def test_placement_helpers():
    B, Hkv, ncap, d, nnew = 4, 2, 8, 2, 3
    lens = (0, 6, -5, 99)
    cache = np.zeros((B, Hkv, ncap, d), np.uint16)
    new = np.arange(1, B * Hkv * nnew * d + 1, dtype=np.uint16).reshape(B, Hkv, nnew, d)
    out = ai.expected_contiguous(cache, new, lens)
    assert np.array_equal(out[0, :, :3], new[0]) and not out[0, :, 3:].any()
    assert np.array_equal(out[1, :, 6:8], new[1, :, :2]) and not out[1, :, :6].any()      # the third token is dropped
    assert np.array_equal(out[2, :, :3], new[2])                                          # clamped up to 0
    assert not out[3].any()                                                               # clamped down to full: nothing fits
    assert np.array_equal(ai.lens_after(lens, B, nnew, ncap), [3, 8, 3, 8])
    assert np.array_equal(ai.lens_after(None, B, nnew, ncap), [3, 3, 3, 3])
    assert np.array_equal(ai.expected_contiguous(cache, new, None)[:, :, :3], new)
    assert not cache.any()                                                                # the input is left alone


def test_paged_helpers():
    B, Hkv, ncap, d, nnew, ps = ai.SHAPE["B"], ai.SHAPE["Hkv"], ai.SHAPE["Ncap"], 4, 37, 16
    table, num_pages = ai.make_table(ai.LENS, B, ncap, nnew, ps, seed=7)
    assert table.shape == (B, 8) and num_pages == B * 8 + 3
    after = ai.lens_after(ai.LENS, B, nnew, ncap)
    assert list(after) == [37, 54, 128, 128, 37, 128]
    live = [int(table[b, pi]) for b in range(B) for pi in range(8) if pi * ps < after[b]]
    assert len(set(live)) == len(live) and all(0 <= p < num_pages for p in live)
    assert all(int(table[b, pi]) in cm.GARBAGE for b in range(B) for pi in range(8) if pi * ps >= after[b])
    written = ai.written_pages(ai.LENS, B, ncap, nnew, ps)
    assert {pi for (b, pi) in written if b == 1} == {1, 2, 3}            # 17 .. 53 crosses two page boundaries
    assert {pi for (b, pi) in written if b == 2} == {7} and not {1 for (b, _) in written if b in (3, 5)}
    pool = ai.random_bytes((num_pages, Hkv, ps, d), 2, seed=1)
    new = ai.random_bytes((B, Hkv, nnew, d), 2, seed=2)
    out = ai.expected_paged(pool, new, ai.LENS, table)
    # the same tokens through the contiguous helper, gathered page by page
    cache = np.zeros((B, Hkv, ncap, d), np.uint16)
    flat = ai.expected_contiguous(cache, new, ai.LENS)
    changed = np.zeros(num_pages, bool)
    for (b, pi) in written:
        page = table[b, pi]
        changed[page] = True
        L = cm.clamp(ai.LENS[b], ncap)
        for r in range(ps):
            p = pi * ps + r
            want = flat[b, :, p] if L <= p < L + nnew else pool[page, :, r]
            assert np.array_equal(out[page, :, r], want)
    assert np.array_equal(out[~changed], pool[~changed])
    # a bad entry drops its page's tokens and nothing else
    bad = table.copy()
    bad[1, 2] = num_pages + 5
    out_bad = ai.expected_paged(pool, new, ai.LENS, bad)
    assert np.array_equal(out_bad[table[1, 2]], pool[table[1, 2]])
    keep = np.ones(num_pages, bool)
    keep[table[1, 2]] = False
    assert np.array_equal(out_bad[keep], out[keep])
