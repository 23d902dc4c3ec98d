"""CPU tier of the rotary-append tests: tests/rope_inputs.py -- the restatement the GPU tier compares bytes with -- against independent
formulations (torch's element-wise fp32 operators, the HF rotate_half formula, fa.quantize_kv_fp8), and the search for inputs on
which a fused multiply-add changes the stored 16-bit value.  Without the last the GPU equality could not see a contracted kernel."""
import numpy as np
import pytest

import append_inputs as ai
import rope_inputs as ri

FMTS = [pytest.param(0, id="fp16"), pytest.param(1, id="bf16")]


def _rows(fmt, shape, seed):
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * 3
    return ai.round16_bits(x, fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rot_dim", [16, 64, 128])
def test_restatement_is_torch_fp32_and_rotate_half(fmt, rot_dim):
    torch = pytest.importorskip("torch")
    B, H, N, d, ncap, max_pos = 3, 4, 5, 128, 64, 40
    lens = (0, 17, 38)   # the last sequence runs into the table's clamp: positions 38 .. 42 use rows 38, 39, 39, 39, 39
    bits = _rows(fmt, (B, H, N, d), 1)
    cos, sin = ri.scrambled_table(max_pos, rot_dim // 2, 2)
    got = ri.rotated_rows_fp32(bits, fmt, lens, ncap, cos, sin, False)
    pos = torch.tensor(ri.positions(lens, B, ncap, N)).clamp(max=max_pos - 1)
    assert pos.tolist()[2] == [38, 39, 39, 39, 39]
    x = torch.from_numpy(ai.widen16(bits, fmt))
    c, s = torch.from_numpy(cos)[pos][:, None], torch.from_numpy(sin)[pos][:, None]   # [B, 1, N, half]
    half = rot_dim // 2
    x1, x2 = x[..., :half], x[..., half:rot_dim]
    want = x.clone()
    want[..., :half] = x1 * c - x2 * s
    want[..., half:rot_dim] = x2 * c + x1 * s
    assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    # HF: q * cos + rotate_half(q) * sin with cos, sin repeated over the two halves
    xr = x[..., :rot_dim]
    hf = xr * torch.cat([c, c], -1) + torch.cat([-x2, x1], -1) * torch.cat([s, s], -1)
    assert np.array_equal(got[..., :rot_dim].view(np.uint32), hf.numpy().view(np.uint32))
    assert np.array_equal(got[..., rot_dim:], ai.widen16(bits, fmt)[..., rot_dim:])
    # the 16-bit form: torch's own rounding of the fp32 result
    dt = torch.float16 if fmt == 0 else torch.bfloat16
    want16 = want[..., :rot_dim].to(dt).view(torch.int16).numpy().view(np.uint16)
    got16 = ri.rotated_rows16(bits, fmt, lens, ncap, cos, sin, False)
    assert np.array_equal(got16[..., :rot_dim], want16) and np.array_equal(got16[..., rot_dim:], bits[..., rot_dim:])


@pytest.mark.parametrize("fmt", FMTS)
def test_interleaved_is_half_split_under_the_permutation(fmt):
    B, H, N, d, rot_dim = 2, 2, 3, 64, 32
    bits = _rows(fmt, (B, H, N, d), 3)
    cos, sin = ri.scrambled_table(50, rot_dim // 2, 4)
    half = rot_dim // 2
    perm = np.arange(d)
    perm[0:rot_dim:2], perm[1:rot_dim:2] = np.arange(half), np.arange(half) + half   # interleaved slot -> half-split slot
    split = ri.rotated_rows16(_to_split(bits, perm), fmt, (0, 9), 48, cos, sin, False)
    inter = ri.rotated_rows16(bits, fmt, (0, 9), 48, cos, sin, True)
    assert np.array_equal(_to_split(inter, perm), split)
    assert not np.array_equal(inter, bits)


def _to_split(rows, perm):
    """rows in the interleaved order -> the same pairs laid out half-split"""
    out = np.empty_like(rows)
    out[..., perm] = rows
    return out


def test_identity_and_real_tables():
    cos, sin = ri.identity_table(7, 8)
    assert cos.dtype == np.float32 and (cos == 1).all() and (sin == 0).all() and cos.shape == (7, 8)
    # not a plain copy: -0 in x1 and a negative x2 give -0 - (-0) = +0
    x = np.zeros((1, 1, 1, 16), np.float32)
    x[..., 0], x[..., 8] = -0.0, -1.0
    y = ri.rotate_fp32(x, cos[:1], sin[:1], False)
    assert not np.signbit(y[..., 0]).any()
    cos, sin = ri.real_table(100, 64)
    assert cos.shape == (100, 32) and (cos[0] == 1).all() and (sin[0] == 0).all()
    assert abs(float(cos[1, 0]) - np.cos(1.0)) < 1e-7 and abs(float(sin[3, 31]) - np.sin(3 * 10000.0 ** (-62 / 64))) < 1e-7
    a, b = ri.scrambled_table(165, 64, 5)
    assert np.unique(np.concatenate([a.ravel(), b.ravel()])).size == 2 * 165 * 64 and np.abs(a).max() < 1


def test_table_row_clamp():
    assert ri.table_rows([0, 98, 99, 100, 127, 1000], 100).tolist() == [0, 98, 99, 99, 99, 99]
    assert ri.positions(ai.LENS, 6, 128, 2).tolist() == [[0, 1], [17, 18], [123, 124], [128, 129], [0, 1], [128, 129]]
    assert ri.positions(None, 2, 128, 3).tolist() == [[0, 1, 2]] * 2


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_recipe_on_the_fp32_value_is_quantize_kv_fp8(fmt):
    torch = pytest.importorskip("torch")
    import flashattention_kernel_project_amd as fa
    B, H, N, d = 2, 2, 9, 64
    bits = _rows(fmt, (B, H, N, d), 6)
    cos, sin = ri.scrambled_table(32, 16, 7)
    y = ri.rotated_rows_fp32(bits, fmt, (3, 20), 64, cos, sin, False)
    for scales in ((0.011, 0.37), None):
        s = torch.tensor(list(scales) if scales else [1.0] * H, dtype=torch.float32)
        want = fa.quantize_kv_fp8(torch.from_numpy(y), s)[0].view(torch.uint8).numpy()
        assert np.array_equal(ri.fp8_codes(y, scales), want)
    # rounding to 16 bit first (the unfused path) is another function: some code differs
    y16 = ai.widen16(ri.rotated_rows16(bits, fmt, (3, 20), 64, cos, sin, False), fmt)
    assert not np.array_equal(ri.fp8_codes(y16, (0.011, 0.37)), ri.fp8_codes(y, (0.011, 0.37)))


@pytest.mark.parametrize("fmt", FMTS)
def test_contraction_witnesses(fmt):
    """At least 64 witnesses per format and per contracted form from 2^22 draws; each is a value of the format, and the pinned and the
    contracted y1 differ after the rounding."""
    A, Bw = ri.contraction_witnesses(fmt, 64)
    for form, w in enumerate((A, Bw)):
        assert w.shape == (64, 4) and w.dtype == np.float32
        x1, x2, c, s = w.T
        assert np.array_equal(ai.widen16(ai.round16_bits(x1, fmt), fmt), x1) and np.array_equal(ai.widen16(ai.round16_bits(x2, fmt), fmt), x2)
        assert (np.abs(c) < 1).all() and (np.abs(s) < 1).all()
        pinned = ai.round16_bits(ri.pinned_y1(x1, x2, c, s), fmt)
        contracted = ai.round16_bits(ri.contracted_y1(x1, x2, c, s)[form], fmt)
        assert (pinned != contracted).all()
    rng = np.random.default_rng(7)   # the count behind the bar of 64, printed for the record
    n = 1 << 22
    x1 = ai.widen16(ai.round16_bits(rng.standard_normal(n).astype(np.float32), fmt), fmt)
    x2 = ai.widen16(ai.round16_bits(rng.standard_normal(n).astype(np.float32), fmt), fmt)
    c, s = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    want = ai.round16_bits(ri.pinned_y1(x1, x2, c, s), fmt)
    counts = [int((ai.round16_bits(g, fmt) != want).sum()) for g in ri.contracted_y1(x1, x2, c, s)]
    print(f"fmt {fmt}: {counts} witnesses in 2^22 draws")
    assert min(counts) >= 64


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_witness_case_places_every_witness(fmt, interleaved):
    rows, cos, sin = ri.witness_case(fmt, 64, 16, interleaved)
    assert rows.shape == (1, 1, 16, 64) and cos.shape == (16, 8) == sin.shape
    got = ri.rotated_rows16(rows, fmt, (0,), 128, cos, sin, interleaved)
    i1, _ = ri.pair_slices(16, interleaved)
    x = ai.widen16(rows, fmt)[0, 0]
    _, i2 = ri.pair_slices(16, interleaved)
    a, b = ri.contracted_y1(x[:, i1], x[:, i2], cos, sin)
    a16, b16 = ai.round16_bits(a, fmt), ai.round16_bits(b, fmt)
    y1 = got[0, 0][:, i1]
    assert (y1[:8] != a16[:8]).all() and (y1[8:] != b16[8:]).all()   # tokens 0..7 hold form A's witnesses, 8..15 form B's
