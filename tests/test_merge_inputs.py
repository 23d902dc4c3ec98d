"""CPU tier of tests/merge_inputs.py: the float64 restatement of the merge rule is the rule; the composed call's two float64 states,
merged by it through their strides, are the float64 reference on the concatenated keys; the derived fp32 bound is small enough to
mean something; and on EVERY parity launch of tests/test_gpu_kvcache_merge.py each wrong merge -- a part dropped, the prefix counted
twice, lse taken for log2 units, the prefix part's strides ignored -- misses a bound that launch applies, so no launch can pass on a
kernel that merges wrongly.  No GPU."""
import numpy as np
import pytest

import common_inputs as cm
import merge_inputs as mi

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
CASES = [pytest.param(*c, id=f"Nq{c[0]}-{'causal' if c[1] else 'full'}-{c[2]}") for c in mi.CASES]


def test_rule_restated():
    """merge_f64 against the rule written out for one row, the neutral part, the empty row and the three layouts"""
    rng = np.random.default_rng(1)
    B, H, rows, d, R = 2, 3, 4, 8, 5
    o = rng.normal(size=(R, B, H, rows, d))
    l = rng.uniform(-5, 5, (R, B, H, rows))
    l[1, 0, 1] = -np.inf                       # a neutral part on some rows, NaN in its O rows
    o[1, 0, 1] = np.nan
    l[:, 1, 2, 3] = -np.inf                    # a row with no live part
    parts = [(o[r].reshape(-1, d), l[r].reshape(-1), H * rows, rows) for r in range(R)]
    got, got_lse = mi.merge_f64(parts, B, H, rows)
    assert np.isfinite(got).all() and not np.isnan(got_lse).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.log(np.exp(l).sum(0))
        w = np.exp(l - lse)
    want = np.where(np.isfinite(l)[..., None], w[..., None] * np.nan_to_num(o), 0.0).sum(0)
    want[1, 2, 3] = 0.0
    assert np.abs(got - want).max() < 1e-13 and (got[1, 2, 3] == 0).all() and got_lse[1, 2, 3] == -np.inf
    live = np.isfinite(lse)
    assert np.abs(got_lse[live] - lse[live]).max() < 1e-13
    # the same parts through the [H, B, rows] strides and through padded ones
    for lay in ("hb", "padded"):
        sb, sh, X = mi.layout(lay, B, H, rows)
        x = mi.rows_of(sb, sh, B, H, rows)
        assert len(np.unique(x)) == x.size and x.max() < X
        moved = []
        for r in range(R):
            oo, ll = np.full((X, d), np.nan), np.full(X, np.nan)
            oo[x], ll[x] = o[r], l[r]
            moved.append((oo, ll, sb, sh))
        g2, l2 = mi.merge_f64(moved, B, H, rows)
        assert np.array_equal(g2, got) and np.array_equal(l2, got_lse)
    # one part: the part itself; one finite part among neutral ones: the same
    g1, l1 = mi.merge_f64(parts[:1], B, H, rows)
    assert np.array_equal(g1[0, 0], o[0, 0, 0]) and np.array_equal(l1[0, 0], l[0, 0, 0])
    dead = [(np.full((B * H * rows, d), np.nan), np.full(B * H * rows, -np.inf), H * rows, rows)] * 3
    g1, l1 = mi.merge_f64(dead[:2] + parts[:1] + dead[2:], B, H, rows)
    assert np.array_equal(g1[0, 0], o[0, 0, 0]) and np.array_equal(l1[0, 0], l[0, 0, 0])


def test_derived_bound():
    """the fp32 bound grows with R, stays below 1e-5 max|O| at the largest R -- above that it could not tell a wrong merge from a
    right one at the sizes of the parity cases -- and is no smaller than what the fp32 format itself imposes"""
    assert all(mi.f32_bound(a, 1.0) < mi.f32_bound(b, 1.0) for a, b in zip(mi.MERGE_R, mi.MERGE_R[1:]))
    assert mi.f32_bound(max(mi.MERGE_R), 1.0) <= 1e-5 and max(mi.MERGE_R) == 16
    assert mi.f32_bound(1, 1.0) >= 3 * mi.U
    assert mi.lse_bound(16, 70.0) <= 1e-5
    # a float32 restatement of the kernel's steps stays inside it (numpy's exp2 is not the hardware's: this checks the algebra)
    for R in mi.MERGE_R:
        worst = 0.0
        for d in (64, 128):
            for lay in mi.LAYOUTS:
                parts = mi.merge_parts(_Codec, R, d, "f32", lay)
                want, want_lse = mi.merge_f64(parts, **mi.MERGE_SHAPE)
                got, got_lse = _merge_f32(parts, **mi.MERGE_SHAPE)
                worst = max(worst, float(np.abs(got - want).max()))
                assert np.abs(got_lse - want_lse).max() <= mi.lse_bound(R, np.abs(want_lse).max())
        assert worst <= mi.f32_bound(R, 4.0), (R, worst)
    assert mi.out_bound(2, 4.0, np.float64(3.0), "f16") > mi.out_bound(2, 4.0, np.float64(3.0), "f32") + 3.0 * 2.0 ** -12


class _Codec:
    """merge_parts needs the oracle only to round to a 16-bit type; the fp32 parts of test_derived_bound do not"""


def _merge_f32(parts, B, H, rows):
    """the kernel's steps in numpy float32"""
    f = np.float32
    lses = np.stack([l[mi.rows_of(sb, sh, B, H, rows)] for (_, l, sb, sh) in parts]).astype(f)
    M = lses.max(0)
    w = np.where(lses == -np.inf, f(0), np.exp2(((lses - M).astype(f) * f(1.4426950408889634)).astype(f)).astype(f))
    L = w.sum(0, dtype=f)
    acc = np.zeros((B, H, rows, parts[0][0].shape[1]), f)
    for (o, _, sb, sh), wr in zip(parts, w):
        acc = (acc + wr[..., None] * o[mi.rows_of(sb, sh, B, H, rows)]).astype(f)
    return (acc / L[..., None]).astype(f), (M + np.log2(L).astype(f) * f(0.6931471805599453)).astype(f)


@pytest.mark.parametrize("lay", mi.LAYOUTS)
def test_merge_parts(oracle, lay):
    """the drawn parts: the stated spread with both ends present, NaN wherever the layout names no row, the dtype's values"""
    B, H, rows = (mi.MERGE_SHAPE[k] for k in ("B", "H", "rows"))
    sb, sh, X = mi.layout(lay, B, H, rows)
    x = mi.rows_of(sb, sh, B, H, rows)
    assert len(np.unique(x)) == x.size and x.max() < X
    assert (lay == "padded") == (X > x.size)
    for R in mi.MERGE_R:
        for dtype in mi.STATE_DTYPES:
            parts = mi.merge_parts(oracle, R, 64, dtype, lay)
            assert len(parts) == R
            lses = np.stack([p[1][x] for p in parts]).astype(np.float64)
            spread = lses.max(0) - lses.min(0)
            assert (spread <= mi.SPREAD + 1e-4).all() and (R <= 2 or (spread >= mi.SPREAD - 1e-4).all())
            if R > 1:   # rows whose second-largest part weighs in, and (with two parts) rows where it all but vanishes
                second = np.sort(lses, 0)[-2] - lses.max(0)
                assert (second >= -mi.NEAR).sum() >= 4 and (R > 2 or (second <= -mi.NEAR).sum() >= 1)
            gap = np.ones(X, bool)
            gap[x.reshape(-1)] = False
            for o, l, _, _ in parts:
                assert np.isnan(o[gap]).all() and np.isnan(l[gap]).all() and np.isfinite(o[~gap]).all()
                assert np.array_equal(mi.round_to(o[~gap], dtype, oracle), o[~gap])


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "fp8"))
@pytest.mark.parametrize("Nq,causal,variant", CASES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_composition_is_the_reference_and_wrong_merges_miss(oracle, fmt, d, Nq, causal, variant, fp8):
    """The two float64 states of the composed call, merged by the rule through their strides, are expected_f64 on the concatenated
    keys; each of the wrong merges misses a bound of the GPU parity launch of this case."""
    c = mi.SHAPE
    B, Hkv, G = c["B"], c["Hkv"], c["G"]
    rows = G * Nq
    x = mi.inputs(oracle, "base", Nq, d, fmt, fp8)
    want, want_lse = mi.reference(oracle, "base", Nq, d, fmt, causal, variant, fp8)
    parts = mi.parts_f64(oracle, "base", Nq, d, fmt, causal, variant, fp8)
    got, got_lse = mi.merge_f64(parts, B, Hkv, rows)
    live = np.isfinite(want_lse)
    assert live.all()                          # P > 0: every row sees the prefix
    assert np.abs(got.reshape(want.shape) - want).max() < 1e-12 and np.abs(got_lse.reshape(want_lse.shape) - want_lse).max() < 1e-12
    vmax = mi.vmax_of(x)
    assert not mi.misses(oracle, got, got_lse, want, want_lse, fmt, vmax)
    for kind in mi.WRONG:
        o, l = mi.wrong_merge(kind, parts, B, Hkv, rows)
        assert mi.misses(oracle, o, l, want, want_lse, fmt, vmax), kind


def test_causal_rows_keep_the_prefix(oracle):
    """with L_b < Nq a causal row sees no suffix key and the whole prefix: the reference is the prefix part's row, not a prefix
    cut short by a mask aligned to the end of P + L_b keys; for L_b >= Nq it is expected_f64 with causal on P + L_b keys"""
    c = mi.SHAPE
    B, Hkv, G, P, Ncap = (c[k] for k in ("B", "Hkv", "G", "P", "Ncap"))
    Nq, d, fmt = 3, 64, 0
    lim = mi.suffix_limits(c["lens"], Nq, Ncap, True)
    assert lim[0] == [0, 0, 0] and lim[1] == [0, 0, 1] and lim[2] == [148, 149, 150]
    x = mi.inputs(oracle, "base", Nq, d, fmt)
    want, want_lse = mi.reference(oracle, "base", Nq, d, fmt, True, "none")
    pre = mi.parts_f64(oracle, "base", Nq, d, fmt, True, "none")[0]
    o_p = pre[0].reshape(Hkv, B, G, Nq, d).transpose(1, 0, 2, 3, 4).reshape(B * Hkv * G, Nq, d)
    Hq = Hkv * G
    assert np.abs(want[:Hq] - o_p[:Hq]).max() < 1e-12 and np.abs(want[Hq:2 * Hq, :2] - o_p[Hq:2 * Hq, :2]).max() < 1e-12
    k, v = mi.concatenated(x, c)
    full, full_lse = cm.expected_f64(x["q"], k, v, [P + L for L in c["lens"]], B, Hkv, G, Nq, True, 0)
    assert np.abs(full[2 * Hq:] - want[2 * Hq:]).max() < 1e-12 and np.abs(full_lse[2 * Hq:] - want_lse[2 * Hq:]).max() < 1e-12
    assert np.abs(full[:Hq] - want[:Hq]).max() > 1e-3      # the cut prefix is another result


def test_long_prefix_splits(oracle):
    """the LONG shape is the one whose prefix decode splits, by the library's rule restated in tests/window_inputs.py"""
    import window_inputs as wi
    for c, want in ((mi.SHAPE, False), (mi.LONG, True)):
        for Nq in mi.NQS:
            assert (wi.split_count(c["Hkv"], c["B"] * c["G"] * Nq, c["Pcap"]) > 1) == want


@pytest.mark.parametrize("causal", (False, True))
def test_census_case(oracle, causal):
    """the census inputs: integer sums over the P prefix keys and the visible suffix keys, met exactly by a float64 model of the
    composed call and missed by a merge that drops or doubles a part"""
    import census_inputs as ci
    c = mi.SHAPE
    B, Hkv, G, P = c["B"], c["Hkv"], c["G"], c["P"]
    Nq, d, fmt = 3, 64, 0
    z = mi.census_case(oracle, Nq, d, fmt, causal)
    assert (z["cnt"] >= P).all() and (z["cnt"] == P).any() and z["S"].max() >= 3
    rows = G * Nq
    ones = np.ones(B * Hkv * G)
    zero_k = [np.zeros_like(v) for v in z["v"]]
    o_p, l_p = cm.expected_f64(mi.folded_q(z["q"], B, Hkv, G), zero_k[0], z["v"][0], [P], 1, Hkv, B * G, Nq, False, 0)
    o_s, l_s = cm.expected_f64(z["q"], zero_k[1], z["v"][1], c["lens"], B, Hkv, G, Nq, causal, 0)
    parts = ((o_p.reshape(-1, d), l_p.reshape(-1), rows, B * rows), (o_s.reshape(-1, d), l_s.reshape(-1), Hkv * rows, rows))
    got, _ = mi.merge_f64(parts, B, Hkv, rows)
    assert ci.census_check(got.reshape(z["S"].shape), z["S"], z["cnt"], ones) < 1e-9
    for kind in ("drops the prefix", "prefix twice", "strides ignored"):
        o, _ = mi.wrong_merge(kind, parts, B, Hkv, rows)
        with pytest.raises(AssertionError):
            ci.census_check(o.reshape(z["S"].shape), z["S"], z["cnt"], ones)
