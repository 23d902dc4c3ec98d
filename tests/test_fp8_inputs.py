"""The e4m3fn table, encoder and all-codes builders of tests/fp8_inputs.py against torch's CPU conversion, and the fact the fp8
decode kernels rest on: every finite e4m3fn value survives a round trip through fp16 and through bf16 unchanged.  No GPU."""
import numpy as np
import pytest

import common_inputs as cm
import fp8_inputs as f8


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _torch_decode(torch, codes, dtype):
    return torch.from_numpy(np.asarray(codes, np.uint8).copy()).view(torch.float8_e4m3fn).to(dtype)


def test_table_is_torchs_conversion_on_all_256_codes(torch):
    want = _torch_decode(torch, np.arange(256), torch.float32).numpy()
    assert np.array_equal(np.isnan(want), np.isnan(f8.TABLE))
    assert [c for c in range(256) if np.isnan(f8.TABLE[c])] == list(f8.NAN_CODES)
    fin = f8.FINITE_CODES
    assert fin.size == 254 and np.array_equal(want[fin].view(np.uint32), f8.TABLE[fin].view(np.uint32))   # signs of zero too
    assert np.isfinite(f8.TABLE[fin]).all()                                    # no infinities
    mags = np.abs(f8.TABLE[fin])
    assert mags.max() == f8.MAX == 448.0 and mags[mags > 0].min() == f8.MIN_SUBNORMAL == 2.0 ** -9
    assert f8.TABLE[0x08] == f8.MIN_NORMAL


def test_every_finite_value_is_exact_in_fp16_and_bf16(torch):
    fin = f8.FINITE_CODES
    for dt in (torch.float16, torch.bfloat16):
        wide = _torch_decode(torch, fin, dt)
        assert np.array_equal(wide.float().numpy().view(np.uint32), f8.TABLE[fin].view(np.uint32)), dt
        assert np.array_equal(wide.to(torch.float8_e4m3fn).view(torch.uint8).numpy(), fin), dt   # and back
    # none of them is an fp16 subnormal: the smallest is 2^-9, fp16's smallest normal number is 2^-14
    assert f8.MIN_SUBNORMAL >= 2.0 ** -14
    for c in f8.NAN_CODES:
        assert torch.isnan(_torch_decode(torch, [c], torch.float16)).all() and torch.isnan(_torch_decode(torch, [c], torch.bfloat16)).all()


def test_encoder_round_trips_and_rounds_like_torch(torch):
    fin = f8.FINITE_CODES
    assert np.array_equal(f8.encode(f8.TABLE[fin]), fin)
    x = np.random.default_rng(5).standard_normal(20000).astype(np.float32) * np.float32(60.0)
    x = np.concatenate([x, (f8.TABLE[1:0x7E] + f8.TABLE[2:0x7F]) / 2, [448.0, -448.0, 460.0, 1e9, -1e9, 2.0 ** -10, 2.0 ** -11]]).astype(np.float32)
    want = torch.from_numpy(x).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()   # ties included
    assert np.array_equal(f8.encode(x), want)
    assert f8.encode(np.array([np.nan], np.float32))[0] == 0x7F


def test_all_codes_builders():
    a = f8.all_codes((3, 100), seed=1)
    assert a.dtype == np.uint8 and a.shape == (3, 100) and set(a.ravel().tolist()) == set(f8.FINITE_CODES.tolist())
    assert np.array_equal(a, f8.all_codes((3, 100), seed=1)) and not np.array_equal(a, f8.all_codes((3, 100), seed=2))
    lens = (1, 5, 40)
    c = f8.all_codes_cache(3, 2, 40, 64, lens, seed=9)
    for b, L in enumerate(lens):
        assert (c[b, :, L:] == 0x7F).all() and not np.isin(c[b, :, :L], f8.NAN_CODES).any()
        for h in range(2):
            got = set(c[b, h, :L].ravel().tolist())
            assert got == set(f8.FINITE_CODES.tolist()) if L * 64 >= 254 else len(got) == L * 64


def test_scatter_and_poison():
    B, Hkv, Ncap, d, ps, lens = 3, 2, 64, 16, 16, (0, 17, 64)
    k8, v8 = f8.all_codes((B, Hkv, Ncap, d), 1), f8.all_codes((B, Hkv, Ncap, d), 2)
    pk = cm.poisoned(k8, lens, nan=f8.NAN_CODES[0])
    for b, L in enumerate(lens):
        assert (pk[b, :, L:] == 0x7F).all() and np.array_equal(pk[b, :, :L], k8[b, :, :L])
    kp, vp, table = cm.scatter(k8, v8, lens, ps, seed=4, nan=f8.NAN_CODES[0])
    assert kp.shape == vp.shape == (B * 4 + 3, Hkv, ps, d) and kp.dtype == np.uint8 and table.shape == (B, 4)
    live = []
    for b, L in enumerate(lens):
        n_live = (L + ps - 1) // ps
        assert all(int(t) in cm.GARBAGE for t in table[b, n_live:])
        for pi in range(n_live):
            n = min(ps, L - pi * ps)
            page = table[b, pi]
            live.append(int(page))
            assert np.array_equal(kp[page, :, :n], k8[b, :, pi * ps:pi * ps + n]) and np.array_equal(vp[page, :, :n], v8[b, :, pi * ps:pi * ps + n])
            assert (kp[page, :, n:] == 0x7F).all() and (vp[page, :, n:] == 0x7F).all()
    assert len(set(live)) == len(live) == 6
    dead = [p for p in range(kp.shape[0]) if p not in live]
    assert (kp[dead] == 0x7F).all() and (vp[dead] == 0x7F).all()
