"""CPU tier of the fp8 MLA entries: the float64 reference of tests/mla_fp8_inputs.py stays inside the project's bounds under the right
numpy kernel on every family, the check rejects ten numpy stand-ins of wrong fp8 kernels, each on a named family, and
fa.quantize_mla_fp8 agrees with tests/fp8_inputs.py code for code.  No GPU here."""
import numpy as np
import pytest

import common_inputs as cm
import fp8_inputs as f8
import mla_fp8_inputs as m8
import mla_inputs as mi


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", mi.NAMES)
def test_check_accepts_the_right_kernel(oracle, name, fmt, causal):
    """the entry as specified on the poisoned codes, in float64 and merged from two key splits: the reference alone is inside the bounds"""
    po, pl = m8.numpy_kernel(oracle, name, fmt, causal=causal)
    want, want_lse = m8.reference(oracle, name, fmt, causal)
    mi.check(oracle, name, po, pl, want, want_lse, fmt, f"numpy fp8 kernel {name} causal={causal}")


@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("wrong", list(m8.WRONG))
def test_check_rejects_wrong_kernels(oracle, wrong, fmt):
    """each wrong rule on the family mla_fp8_inputs.WRONG names for it; the tile-rounded split end shows without the causal mask"""
    name = m8.WRONG[wrong]
    causal = wrong != "nan_code_as_448"
    po, pl = m8.numpy_kernel(oracle, name, fmt, causal=causal, wrong=wrong)
    want, want_lse = m8.reference(oracle, name, fmt, causal)
    with pytest.raises(AssertionError):
        mi.check(oracle, name, po, pl, want, want_lse, fmt, f"{wrong} on {name}")


def test_codes_hold_what_the_tier_relies_on(oracle):
    """the boosted element is the top code, the other elements lie well inside the range, and the poison is the NaN code"""
    for name in mi.NAMES:
        f = mi.family(name)
        cb = m8.codes(oracle, name, 0)
        assert cb.dtype == np.uint8 and cb.shape == (f["B"], f["Ncap"], mi.DQK) and not np.isin(cb, f8.NAN_CODES).any()
        assert (cb == 0x7E).sum() == sum(min(f["max_q"], cm.clamp(L, f["Ncap"])) for L in f["lens"])
        other = np.abs(f8.decode(cb[:, :, :mi.DC]))
        assert other.max() < 256.0 and np.median(other) > 8.0   # N(0,1) * 448 / 12: far from the subnormals and from the top
        p = m8.poisoned_cache(oracle, name, 0)
        for b in range(f["B"]):
            L = cm.clamp(f["lens"][b], f["Ncap"])
            assert (p[b, L:] == m8.NAN_CODE).all() and np.array_equal(p[b, :L], cb[b, :L])
    pool, table = m8.paged_cache(oracle, "h5", 0, 16)
    assert pool.dtype == np.uint8 and pool.shape[1:] == (16, mi.DQK) and (pool == m8.NAN_CODE).any()
    assert np.isclose(float(m8.C_SCALE) * 448.0, mi.BOOST_K)


def _hard_values():
    """ties between neighbouring codes, +-448 and beyond, subnormals and their ties, +-0, NaN; the row is padded to 576 with zeros"""
    mags = f8.TABLE[:0x7F].astype(np.float64)
    ties = (mags[:-1] + mags[1:]) / 2.0                      # exactly representable in fp32: ties to the even code
    near = np.concatenate([np.nextafter(ties.astype(np.float32), np.float32(0)), np.nextafter(ties.astype(np.float32), np.float32(1e9))])
    special = np.array([448.0, 464.0, 480.0, 1e6, 3e38, 2.0 ** -9, 2.0 ** -10, 2.0 ** -11, 1.5 * 2.0 ** -10, 0.0, 1e-30], np.float64)
    pos = np.concatenate([mags, ties, near.astype(np.float64), special])
    vals = np.concatenate([pos, -pos, [np.nan]]).astype(np.float32)
    rows = -(-vals.size // mi.DQK)
    out = np.zeros(rows * mi.DQK, np.float32)
    out[:vals.size] = vals
    return out.reshape(rows, mi.DQK)


def test_quantize_mla_fp8_agrees_with_the_format_code_for_code(fa):
    import torch
    x = _hard_values()
    want = f8.encode(x)
    assert (want == 0x7F).sum() == 1 and (want == 0x80).any() and (want == 0x7E).any() and (want == 0xFE).any()
    c8, scale = fa.quantize_mla_fp8(torch.from_numpy(x), torch.ones(1))
    assert c8.dtype == torch.float8_e4m3fn and c8.shape == x.shape and scale.dtype == torch.float32 and scale.tolist() == [1.0]
    got = c8.view(torch.uint8).numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    back = f8.decode(got)
    fin = ~np.isnan(x)
    assert np.array_equal(f8.encode(back[fin.reshape(back.shape)]), got[fin.reshape(got.shape)])   # decode -> encode is the identity
    # a scale that is no power of two: the IEEE fp32 quotient, then the same rounding
    s = np.float32(12.0 / 448.0)
    with np.errstate(over="ignore"):   # 3e38 * 3.7 is +inf: beyond the range like the other large values
        y = (x * np.float32(3.7)).astype(np.float32)
    c8, _ = fa.quantize_mla_fp8(torch.from_numpy(y), torch.tensor([float(s)]))
    assert np.array_equal(c8.view(torch.uint8).numpy(), f8.encode(y / s))


def test_quantize_mla_fp8_chooses_amax_over_448(fa):
    import torch
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 7, mi.DQK)).astype(np.float32)
    x[1, 2, 3] = -9.5
    c8, scale = fa.quantize_mla_fp8(torch.from_numpy(x).to(torch.bfloat16))
    amax = np.float32(torch.from_numpy(x).to(torch.bfloat16).float().abs().max().item())
    assert scale.shape == (1,) and scale.dtype == torch.float32 and scale.item() == np.float32(amax / np.float32(448.0))
    codes = c8.view(torch.uint8).numpy()
    assert codes[1, 2, 3] == 0xFE and np.array_equal(codes, f8.encode(torch.from_numpy(x).to(torch.bfloat16).float().numpy() / np.float32(scale.item())))
    z8, zs = fa.quantize_mla_fp8(torch.zeros(2, mi.DQK))
    assert zs.tolist() == [1.0] and not z8.view(torch.uint8).any()
    with pytest.raises(ValueError):
        fa.quantize_mla_fp8(torch.zeros(2, 512))
    with pytest.raises(ValueError):
        fa.quantize_mla_fp8(torch.zeros(2, mi.DQK), torch.ones(2))


# ---- the wide-logit-range inputs on codes: which events of tests/test_softmax_range_inputs.py still fire --------------------------------
@pytest.mark.parametrize("S", [1, 3, 0])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_range_events_survive_the_e4m3_rounding(fmt, S):
    """The scheme's model on the DECODED codes of mla_fp8_inputs.range_case, under the conditions test_softmax_range_inputs.py puts on
    the 16-bit inputs: the staircase moves the reference at least twice and has a quiet step, each jump moves it once by about its lift
    unless its tile opens a split, nothing moves after the fall by 210, and the masked spike moves it only without the mask.  All of
    them hold, so the GPU tier (test_gpu_mla_fp8.py::test_wide_logit_range) leaves none out."""
    import softmax_range_inputs as sr
    import test_softmax_range_inputs as tsr
    f = sr.MLA
    rc = m8.range_case(fmt)
    assert rc["c_scale"] > 0 and not np.isin(rc["codes"], f8.NAN_CODES).any() and (rc["codes"] & 0x7F).max() == 0x7E
    for causal in (True, False):
        ev = m8.range_events(fmt, causal, S)
        rise = {k: np.concatenate(v) for k, v in ev.items()}
        kinds = {kind: (0, i, h) for kind, i, h, _ in sr.MLA_KINDS}
        kinds.update({kind: (1, i, h) for kind, i, h, _ in sr.MLA_SEQ1})
        stair = rise[kinds["staircase"]]
        assert tsr._votes(stair) >= 2 and tsr._quiet_steps(stair) >= 1, stair
        jumps = [(kind, b, keys[0]) for b, table in ((0, sr.MLA_KINDS[1:3] + sr.MLA_KINDS[4:5]), (1, sr.MLA_SEQ1)) for kind, _, _, keys in table]
        for kind, b, (key, lift) in jumps:
            r = rise[kinds[kind]]
            if tsr._opens_a_split(f["lens"][b], S, key):
                assert tsr._votes(r) == 0, (kind, S, r)
            else:
                assert tsr._votes(r) == 1 and abs(np.nanmax(r) - lift) < 6.0, (kind, S, r)
        r = rise[kinds["all but tile 0 below -200"]]
        assert tsr._votes(r) == 0 and np.nanmax(r[:len(ev[kinds["all but tile 0 below -200"]][0])]) < -200.0
        assert tsr._votes(rise[kinds["masked 150 on the last key"]]) == (0 if causal else 1)
        want, want_lse = m8.range_reference(fmt, causal)
        Hq = f["Hq"]
        assert np.isfinite(want).all()
        assert abs(want_lse[2 * Hq].mean() + sr.SHIFT * sr.LN2) < 15 and abs(want_lse[2 * Hq + 1].mean() - sr.SHIFT * sr.LN2) < 15
