"""CPU tier of tests/ragged_inputs.py: the restated rules by hand, the reference against the oracle where the counts are
full, and the property that makes the GPU parity meaningful -- no causal parity case passes on a kernel that ignores seqlens_q."""
import numpy as np
import pytest

import common_inputs as cm
import logit_inputs as li
import ragged_inputs as ri

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]


def test_limits_by_hand():
    # L = 10, n = 3 of 5 padded rows, causal: the LAST live row sees the whole sequence
    lo, c, live = cm.row_limits(10, 3, 5, True, 0)
    assert c.tolist() == [8, 9, 10, 0, 0] and lo.tolist() == [0] * 5 and live.tolist() == [True] * 3 + [False] * 2
    lo, c, _ = cm.row_limits(10, 3, 5, True, 4)
    assert lo.tolist() == [4, 5, 6, 0, 0] and c.tolist() == [8, 9, 10, 0, 0]
    lo, c, _ = cm.row_limits(10, 3, 5, False, 4)           # the lower limit is the same without the mask
    assert lo.tolist() == [4, 5, 6, 0, 0] and c.tolist() == [10, 10, 10, 0, 0]
    lo, c, live = cm.row_limits(2, 5, 5, True, 0)          # L < n: the first rows see nothing, and are live all the same
    assert c.tolist() == [0, 0, 0, 1, 2] and live.all()
    assert not cm.row_limits(10, 0, 5, True, 0)[2].any()   # an idle slot
    assert cm.counts((-3, 0, 4, 9, 1 << 30), 5, 8) == [0, 0, 4, 8, 8] and cm.counts(None, 2, 8) == [8, 8]


def test_counts_that_cover_every_row_change_nothing(oracle):
    """no vector, full counts and counts beyond Nq give the same bits; negative counts are the count 0: every row dead, sinks or not"""
    f = ri.FAMILIES["spec"]
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = ri.inputs(oracle, "spec", 64, 0)
    for causal, W, variant in ((True, 0, "none"), (False, 100, "both"), (True, 100, "sinks")):
        sinks, cap = li.options(variant, Hkv * G)
        want = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, causal, W, softcap=cap, sinks=sinks)
        for nq in ([Nq] * B, [Nq + 5] * B):
            got = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, causal, W, softcap=cap, sinks=sinks, nq=nq)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    o, lse = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, True, 0, sinks=li.sinks_for(Hkv * G), nq=[-1] * B)
    assert (o == 0).all() and (lse == -np.inf).all()


@pytest.mark.parametrize("name", list(ri.FAMILIES) + list(ri.EXTRA))
def test_reference_with_full_counts_agrees_with_the_oracle(oracle, name):
    """cm.expected_f64 with n_b = Nq against the oracle's cm.expected, an implementation of its own, on every family, window and mask:
    O within 1e-5 of the value scale (the bound of tests/test_decode_inputs.py), lse within 1e-9 (tests/test_window_inputs.py), -inf on
    the same rows"""
    f = ri.family(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = ri.inputs(oracle, name, 64, 0)
    for W in ri.WINDOWS:
        for causal in (False, True):
            want, want_lse = cm.expected(oracle, q, k, v, f["lens"], B, Hkv, G, Nq, causal, W)
            got, got_lse = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, causal, W, nq=[Nq] * B)
            live = np.isfinite(want_lse)
            assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(v).max()), (name, W, causal)
            assert np.array_equal(np.isfinite(got_lse), live) and np.abs(got_lse[live] - want_lse[live]).max() < 1e-9, (name, W, causal)
            assert (got[~live] == 0).all() and (got_lse[~live] == -np.inf).all()


@pytest.mark.parametrize("name", list(ri.FAMILIES))
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_every_causal_case_fails_on_a_kernel_that_ignores_seqlens_q(oracle, fmt, d, name):
    f = ri.FAMILIES[name]
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    Hq = Hkv * G
    live = ri.live_rows(name)
    for W in ri.WINDOWS:
        o1, l1 = ri.reference(oracle, name, d, fmt, W, True)
        o0, l0 = ri.reference(oracle, name, d, fmt, W, True, ragged=False)
        f1, f0 = np.isfinite(l1), np.isfinite(l0)
        both = f1 & f0
        lse_moved = f1 != f0                                     # -inf against finite: moved; -inf against -inf: not
        lse_moved[both] = np.abs(l1[both] - l0[both]) >= li.LSE_MOVES
        moved = (np.abs(o1 - o0).max(-1) >= 3 * cm.MAX_ABS) | lse_moved
        some = 0
        for b, n in enumerate(cm.counts(f["nq"], B, Nq)):
            if not 0 < n < Nq:
                continue
            rows = slice(b * Hq, (b + 1) * Hq)
            frac = moved[rows][live[rows]].mean()
            assert frac >= 0.5, (name, W, b, frac)
            some += 1
        assert some >= 1, name


@pytest.mark.parametrize("name", list(ri.FAMILIES))
def test_every_case_has_dead_rows_and_what_its_row_says(oracle, name):
    f = ri.FAMILIES[name]
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    live = ri.live_rows(name)
    assert (~live).any() and live.any()
    o, lse = ri.reference(oracle, name, 64, 0, 0, True)
    assert (o[~live] == 0).all() and (lse[~live] == -np.inf).all()
    n = cm.counts(f["nq"], B, Nq)
    if name == "spec":
        assert 0 in n and any(cm.clamp(L, Ncap) < m for L, m in zip(f["lens"], n))
        assert (live & ~np.isfinite(lse)).any()            # a live row without a key
        # ... which has the sink's logit with sinks, while a dead row of the same head stays at -inf
        s = li.sinks_for(Hkv * G)
        _, lse_s = ri.reference(oracle, name, 64, 0, 0, True, variant="sinks")
        r, i = np.argwhere(live & ~np.isfinite(lse))[0]
        assert lse_s[r, i] == pytest.approx(float(s[r % (Hkv * G)])) and (lse_s[~live] == -np.inf).all()
    if name == "blocks":
        assert [G * m for m in n] == [128, 132] and G * Nq > cm.ROWS
    if name == "split":
        assert 0 in n
        for W in ri.WINDOWS:
            assert (ri.want_S(f, W) > 1) == (W == 0)       # the split rule, restated: S > 1 on the capacity, one pass under the window
        assert ri.want_S(f, 0) > 1


def test_the_extra_shape_has_lanes_without_a_peer():
    """ri.EXTRA["tail"]: one pass, full counts, and in the last wave the lanes past Nq carry limits no live row of the wave has"""
    f = ri.EXTRA["tail"]
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    assert ri.want_S(f, 0) == 1 and G == 1 and cm.counts(f["nq"], B, Nq) == [Nq] * B and cm.ROWS > Nq > 32
    lim = cm.row_limits(f["lens"][0], Nq, Nq, True)[1].tolist()
    live, phantom = {lim[r] for r in range(32, Nq)}, {lim[r % Nq] for r in range(Nq, 64)}
    assert not live & phantom
    assert max(phantom) // cm.TILE < min(x - 1 for x in live) // cm.TILE       # they meet their last key in an earlier tile


def test_append_placement_by_hand():
    cache = np.zeros((3, 1, 6, 2), np.uint16)
    rows = np.arange(3 * 1 * 4 * 2, dtype=np.uint16).reshape(3, 1, 4, 2) + 100
    out = ri.place(cache, rows, (1, 4, 0), (2, 4, 0))
    assert (out[0, 0, 1:3] == rows[0, 0, :2]).all() and (out[0, 0, [0, 3, 4, 5]] == 0).all()
    assert (out[1, 0, 4:6] == rows[1, 0, :2]).all() and (out[1, 0, :4] == 0).all()     # tokens 2 and 3: past the capacity
    assert (out[2] == 0).all()
    assert ri.lens_after((1, 4, 0), (2, 4, 0), 3, 4, 6).tolist() == [3, 6, 0]
    assert ri.lens_after((1, 4, 0), None, 3, 4, 6).tolist() == [5, 6, 4]
    assert ri.lens_after(None, (9, -1, 1), 3, 4, 6).tolist() == [4, 0, 1]
    # paged: a slot only padding would reach is never looked up
    pool = np.zeros((4, 1, 2, 2), np.uint16)
    table = np.array([[0, 1, 3], [2, 3, -1], [3, 3, 3]], np.int32)
    out = ri.place(pool, rows, (1, 2, 0), (2, 1, 0), table)
    assert (out[0, 0, 1] == rows[0, 0, 0]).all() and (out[1, 0, 0] == rows[0, 0, 1]).all() and (out[3, 0, 0] == rows[1, 0, 0]).all()
    assert (out[2] == 0).all() and (out[3, 0, 1] == 0).all()
    q = np.arange(3 * 2 * 4 * 2, dtype=np.uint16).reshape(3, 2, 4, 2)
    kept = ri.keep_dead_q(q + 1000, q, (2, 4, 0))
    assert (kept[0, :, :2] == q[0, :, :2] + 1000).all() and (kept[0, :, 2:] == q[0, :, 2:]).all() and (kept[2] == q[2]).all()
