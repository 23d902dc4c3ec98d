"""CPU tier of tests/logit_inputs.py: the reference agrees with the oracle where the features are off and with hand values where they are on, every parity launch of
tests/test_gpu_kvcache_logits.py would fail on a kernel that ignores the feature, the launches reach the split counts they are
named for, and the sink census is exact on the shapes it uses.  No GPU."""
import numpy as np
import pytest

import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import logit_inputs as li
import window_inputs as wi

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]


def test_sinks_are_distinct_and_in_range():
    for Hq in (1, 4, 8, 16):
        s = li.sinks_for(Hq)
        assert s.dtype == np.float32 and ((s >= 6.5) & (s < 9.5)).all()
        assert (np.diff(s) != 0).all()
    c = li.census_sinks(8)
    assert (c[0::2] == 0.0).all() and (c[1::2] == -np.inf).all()


def test_reference_without_a_sink_is_the_oracle_reference(oracle):
    """no sink and no cap, and sinks of -inf: the oracle's cm.expected (O within 1e-5 of the value scale, lse within 1e-9: the bounds of
    tests/test_decode_inputs.py and tests/test_window_inputs.py), and the same bits as each other; a sink of -200: the same to
    float64 rounding, but for the rows without a key"""
    c = wi.CASES["rows"]
    B, Hkv, G, Nq, Ncap = (c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
    (q, k, v), _ = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, 64, 0, c["seed"])
    for W in (0, 3):
        want, want_lse = cm.expected(oracle, q, k, v, c["lens"], B, Hkv, G, Nq, True, W)
        live = np.isfinite(want_lse)
        assert (~live).any()   # the row without a key
        base, base_lse = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, True, W)
        assert np.abs(base - want).max() <= 1e-5 * max(1.0, np.abs(v).max()) and np.array_equal(np.isfinite(base_lse), live)
        assert np.abs(base_lse[live] - want_lse[live]).max() < 1e-9
        o, lse = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, True, W, sinks=np.full(Hkv * G, -np.inf, np.float32))
        assert np.array_equal(o, base) and np.array_equal(lse, base_lse)
        o, lse = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, True, W, sinks=np.full(Hkv * G, -200.0, np.float32))
        assert np.allclose(o, base, rtol=0, atol=1e-12) and np.allclose(lse[live], base_lse[live], rtol=0, atol=1e-12)
        assert (lse[~live] == -200.0).all() and (o[~live[..., None].repeat(64, -1)] == 0).all()   # no key: O = 0, lse = a


def test_sinks_and_softcap_by_hand():
    """One head, d = 2, a cache of three keys, q = (1, 0) at scale 1: a key's logit is its first component.  Every figure below is
    exact in float64 but where a tolerance is written."""
    q2 = np.array([[[1.0, 0.0], [1.0, 0.0]]], np.float32)
    k = np.array([[[0.0, 5.0], [0.0, -3.0], [40.0, 40.0]]], np.float32)       # logits 0, 0 and 40
    v = np.array([[[2.0, 4.0], [6.0, -8.0], [1e6, 1e6]]], np.float32)
    # two rows under the mask at length 1: row 0 sees no key, row 1 sees key 0.  With a sink of 0.25 row 0 is O = 0 and lse = the
    # sink; row 1 holds a key at logit 0 beside the sink: with a sink of 0 the two share the weight, O = v_0 / 2 and lse = ln 2
    o, lse = cm.expected_f64(q2, k, v, [1], 1, 1, 1, 2, True, 0, scale=1.0, sinks=np.array([0.25], np.float32))
    assert (o[0, 0] == 0).all() and lse[0, 0] == 0.25
    o, lse = cm.expected_f64(q2, k, v, [1], 1, 1, 1, 2, True, 0, scale=1.0, sinks=np.array([0.0], np.float32))
    assert (o[0, 0] == 0).all() and lse[0, 0] == 0.0
    assert o[0, 1].tolist() == [1.0, 2.0] and lse[0, 1] == np.log(2.0)
    # without a sink, and with a sink of -inf: row 0 is 0 and -inf, row 1 is v_0 and lse 0
    for sinks in (None, np.array([-np.inf], np.float32)):
        o, lse = cm.expected_f64(q2, k, v, [1], 1, 1, 1, 2, True, 0, scale=1.0, sinks=sinks)
        assert (o[0, 0] == 0).all() and lse[0, 0] == -np.inf and o[0, 1].tolist() == [2.0, 4.0] and lse[0, 1] == 0.0
    # one row, length 2, no mask: keys 0 and 1 weigh 1/2 each, the key past the length is not read; a sink of 0 makes it thirds
    q1 = q2[:, :1]
    o, lse = cm.expected_f64(q1, k, v, [2], 1, 1, 1, 1, False, 0, scale=1.0)
    assert o[0, 0].tolist() == [4.0, -2.0] and lse[0, 0] == np.log(2.0)
    o, lse = cm.expected_f64(q1, k, v, [2], 1, 1, 1, 1, False, 0, scale=1.0, sinks=np.array([0.0], np.float32))
    assert np.abs(o[0, 0] - np.array([8.0, -4.0]) / 3).max() <= 1e-15 and abs(lse[0, 0] - np.log(3.0)) <= 1e-15
    # a cap that saturates: tanh(1000 / 2) is 1 in float64, so logits of 1000, -1000 and 0 become 2, -2 and 0 -- and logits five
    # times as large give the same bits
    kc = np.array([[[1000.0, 0.0], [-1000.0, 0.0], [0.0, 7.0]]], np.float32)
    vc = np.array([[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]], np.float32)
    o, lse = cm.expected_f64(q1, kc, vc, [3], 1, 1, 1, 1, False, 0, scale=1.0, softcap=2.0)
    w = np.exp(np.array([0.0, -4.0, -2.0]))                                    # exp(t - 2)
    assert np.abs(o[0, 0] - np.array([w[0] + w[2], w[1] + w[2]]) / w.sum()).max() <= 1e-15 and abs(lse[0, 0] - (2.0 + np.log(w.sum()))) <= 1e-15
    o5, lse5 = cm.expected_f64(q1, 5 * kc, vc, [3], 1, 1, 1, 1, False, 0, scale=1.0, softcap=2.0)
    assert np.array_equal(o5, o) and np.array_equal(lse5, lse)
    # the sink is not capped: at 10 it outweighs the capped keys by e^8 and more
    o, lse = cm.expected_f64(q1, kc, vc, [3], 1, 1, 1, 1, False, 0, scale=1.0, softcap=2.0, sinks=np.array([10.0], np.float32))
    assert abs(lse[0, 0] - (10.0 + np.log1p(np.exp(-8.0) * w.sum()))) <= 1e-14 and np.abs(o[0, 0]).max() < np.exp(-7.0)


def test_reference_rules_by_hand():
    """one head, one row, three keys: the two formulas written out"""
    q = np.array([[[1.0, 0.0]]], np.float32)
    k = np.array([[[2.0, 0.0], [-1.0, 0.0], [0.5, 0.0], [9.0, 9.0]]], np.float32)
    v = np.array([[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [7.0, 7.0]]], np.float32)
    a, cap = 0.3, 1.5
    o, lse = cm.expected_f64(q, k, v, [3], 1, 1, 1, 1, False, 0, scale=1.0, softcap=cap, sinks=np.array([a], np.float32))
    t = cap * np.tanh(np.array([2.0, -1.0, 0.5]) / cap)
    den = np.exp(np.float64(np.float32(a))) + np.exp(t).sum()
    assert np.allclose(lse[0, 0], np.log(den), rtol=0, atol=1e-14)
    assert np.allclose(o[0, 0], (np.exp(t) / den) @ v[0, :3].astype(np.float64), rtol=0, atol=1e-14)
    # a negative scale negates the logits: tanh is odd
    o2, lse2 = cm.expected_f64(q, -k, v, [3], 1, 1, 1, 1, False, 0, scale=-1.0, softcap=cap, sinks=np.array([a], np.float32))
    assert np.allclose(o2, o, rtol=0, atol=1e-14) and np.allclose(lse2, lse, rtol=0, atol=1e-14)
    # +200 and -200: finite, the sink takes (nearly) all of the weight resp. none of it
    for big in (200.0, -200.0):
        o3, lse3 = cm.expected_f64(q, k, v, [3], 1, 1, 1, 1, False, 0, scale=1.0, sinks=np.array([big], np.float32))
        assert np.isfinite(lse3).all() and np.isfinite(o3).all()
    assert abs(lse3[0, 0] - np.log(np.exp([2.0, -1.0, 0.5]).sum())) < 1e-12


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_every_parity_launch_fails_on_a_kernel_that_ignores_the_feature(oracle, fmt, d):
    """sinks alone: lse moves by >= 0.05 on EVERY live row; the soft-cap alone: on at least half of them, and O by >= 3 * MAX_ABS
    somewhere.  Both together are held against the launch with ONE option taken away (the two move lse in opposite directions, so
    against neither they can cancel): without the sinks lse moves on every live row; without the cap O moves by >= 3 * MAX_ABS --
    lse need not, because a sink above the keys' logits holds most of the sum whatever the cap does to the keys."""
    for (name, W, causal, variant) in li.LAUNCHES:
        if variant == "sinks":
            frac, _ = li.feature_shows(oracle, name, d, fmt, W, causal, variant)
            assert frac == 1.0, (name, W, causal, variant, frac)
        elif variant == "softcap":
            frac, o_move = li.feature_shows(oracle, name, d, fmt, W, causal, variant)
            assert frac >= 0.5 and o_move >= 3 * cm.MAX_ABS, (name, W, causal, variant, frac, o_move)
        else:
            frac, _ = li.feature_shows(oracle, name, d, fmt, W, causal, variant, without="softcap")
            _, o_move = li.feature_shows(oracle, name, d, fmt, W, causal, variant, without="sinks")
            assert frac == 1.0 and o_move >= 3 * cm.MAX_ABS, (name, W, causal, variant, frac, o_move)


def test_softcap_50_would_not_be_a_parity_value(oracle):
    """why SOFTCAP is 1.0: at 50 the outputs move by less than the max-abs bound, so a kernel without the cap would pass"""
    c = wi.CASES["one_pass"]
    B, Hkv, G, Nq, Ncap = (c[x] for x in ("B", "Hkv", "G", "Nq", "Ncap"))
    (q, k, v), _ = wi.inputs(oracle, B, Hkv, G, Nq, Ncap, 64, 0, c["seed"])
    o0, _ = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, False, 0)
    o1, _ = cm.expected_f64(q, k, v, c["lens"], B, Hkv, G, Nq, False, 0, softcap=50.0)
    assert np.abs(o1 - o0).max() < cm.MAX_ABS


def test_split_counts_of_the_launches():
    """the windowed launches are the window tier's (one pass, S = 4 with empty splits, one pass); without a window the same shapes
    split 2, 16 and 4 ways, and the short sequences leave splits empty"""
    for name, c in wi.CASES.items():
        assert li.want_S(name, li.WINDOWED[name]) == c["S"]
        assert li.WINDOWED[name] in c["windows"]
    assert [li.want_S(n, 0) for n in ("one_pass", "split", "rows")] == [2, 16, 4]
    c = wi.CASES["rows"]
    assert di.live_splits(4, 4) == 1 and di.live_splits(1000, 4) == 4          # rows, no window: three empty splits behind 4 keys
    assert "empty split" in wi.categories(wi.CASES["split"]["lens"], 1, 4096, 1024, 4, False)
    assert "row without keys" in wi.categories(c["lens"], c["Nq"], c["Ncap"], 64, 1, True)


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_census_is_exact_and_discriminates(oracle, fmt, d):
    S_seen = set()
    for (name, W, causal) in li.CENSUS:
        c = wi.CASES[name]
        z = li.census_case(oracle, name, d, fmt, W, causal)
        S_seen.add(li.want_S(name, W))
        assert ci.z_exact(fmt, z["s_max"]) and ci.z_exact(fmt, z["s_max"] + z["m"].max())   # P_BITS + log2(S) <= 24, the sink included
        Hq = c["Hkv"] * c["G"]
        assert z["sink"].reshape(c["B"], Hq).any(1).all()
        assert Hq == 1 or (1 - z["sink"]).reshape(c["B"], Hq).any(1).all()   # "split" has one head: a sink of 0
        if c["G"] > 1:   # both kinds inside one folded group
            grp = z["sink"].reshape(-1, c["G"])
            assert ((grp == 1).any(1) & (grp == 0).any(1)).all()
        # the float64 model passes; a sink counted twice (per split), dropped, or taken from the neighbouring head does not
        den = z["cnt"] + z["sink"][:, None]

        def model(n):   # O and lse of a kernel that divides by n
            with np.errstate(divide="ignore"):
                return np.where(n[..., None] > 0, z["S"] / np.maximum(n, 1)[..., None], 0.0), np.log(n.astype(np.float64))
        li.sink_census_check(*model(den), z)
        for wrong in (z["cnt"] + 2 * z["sink"][:, None], z["cnt"], z["cnt"] + (1 - z["sink"])[:, None]):
            assert (wrong != den).any()
            with pytest.raises(AssertionError):
                li.sink_census_check(*model(wrong), z)
    assert {1, 4} <= S_seen
