"""CPU tier of the MLA entries: the float64 reference of tests/mla_inputs.py against two independent statements of the same
arithmetic, and the check against numpy stand-ins of wrong kernels, each of which it must reject (as the other *_inputs tiers do).
No GPU and no library call here."""
import math

import numpy as np
import pytest

import common_inputs as cm
import decode_varlen_inputs as dv
import mla_inputs as mi


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("name", ["h1", "h5"])
def test_reference_against_brute_force(oracle, name, causal):
    """every live row once more, key by key with scalar sums: no matrix product, no shared maximum"""
    f, lay = mi.family(name), mi.layout(name)
    (q, c), _ = mi.inputs(oracle, name, 0)
    want, want_lse = mi.reference(oracle, name, 0, causal)
    Hq, Ncap = f["Hq"], f["Ncap"]
    seen = 0
    for b in range(f["B"]):
        L = min(max(f["lens"][b], 0), Ncap)
        n = lay.n[b]
        for h in range(Hq):
            for i in range(f["max_q"]):
                row, row_lse = want[b * Hq + h, i], want_lse[b * Hq + h, i]
                lim = 0 if i >= n else (max(0, L - n + 1 + i) if causal else L)
                if lim == 0:
                    assert not row.any() and row_lse == -np.inf
                    continue
                qq = q[b * Hq + h, i].astype(np.float64)
                logits = [mi.SCALE * math.fsum(qq * c[b, j].astype(np.float64)) for j in range(lim)]
                den = math.fsum(math.exp(s) for s in logits)
                o = sum(math.exp(s) / den * c[b, j, :mi.DC].astype(np.float64) for j, s in enumerate(logits))
                assert np.abs(o - row).max() <= 1e-12 * max(1.0, np.abs(row).max())
                assert abs(math.log(den) - row_lse) <= 1e-12 * max(1.0, abs(row_lse))
                seen += 1
    assert seen > 0


def test_reference_against_unabsorbed_mha(oracle):
    """Absorption is exact algebra: with W_UK_h [128, 512] and W_UV_h [512, 128] per head, attention of q_h = [q_nope | q_rope] over
    K_h = [C[:, :512] W_UK_h^T | C[:, 512:]] with V_h = C[:, :512] W_UV_h equals the up-projection of the absorbed reference's O for
    q_abs = [q_nope W_UK_h | q_rope].  float64 on both sides, 1e-10 relative."""
    rng = np.random.default_rng(4242)
    B, Hq, Nq, Ncap, dn = 2, 3, 2, 96, 128
    lens, n = (96, 41), [2, 1]
    c = rng.standard_normal((B, Ncap, mi.DQK))
    q_nope, q_rope = rng.standard_normal((B * Hq, Nq, dn)), rng.standard_normal((B * Hq, Nq, mi.DR))
    w_uk, w_uv = rng.standard_normal((Hq, dn, mi.DC)) / 16.0, rng.standard_normal((Hq, mi.DC, dn)) / 16.0
    scale = (dn + mi.DR) ** -0.5   # the model's own scale, which the absorbed call is handed as it is
    q_abs = np.concatenate([np.einsum("rin,rnc->ric", q_nope, np.tile(w_uk, (B, 1, 1))), q_rope], axis=-1)
    o_abs, lse_abs = mi.expected_f64(q_abs, c, lens, n, Nq, Hq, True, scale=scale)
    for b in range(B):
        for h in range(Hq):
            k_h = np.concatenate([c[b, :, :mi.DC] @ w_uk[h].T, c[b, :, mi.DC:]], axis=-1)   # [Ncap, 192]
            v_h = c[b, :, :mi.DC] @ w_uv[h]
            for i in range(n[b]):
                lim = max(0, lens[b] - n[b] + 1 + i)
                s = (k_h[:lim] @ np.concatenate([q_nope[b * Hq + h, i], q_rope[b * Hq + h, i]])) * scale
                p = np.exp(s - s.max())
                o = (p / p.sum()) @ v_h[:lim]
                got = o_abs[b * Hq + h, i] @ w_uv[h]
                assert np.abs(got - o).max() <= 1e-10 * np.abs(o).max()
                assert abs(lse_abs[b * Hq + h, i] - (s.max() + np.log(p.sum()))) <= 1e-10 * max(1.0, abs(s.max()))


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", mi.NAMES)
def test_check_accepts_the_right_kernel(oracle, name, fmt):
    """the entry as specified, in float64 and merged from two key splits, passes the check with its sentinels in place"""
    po, pl = mi.numpy_kernel(oracle, name, fmt)
    want, want_lse = mi.reference(oracle, name, fmt, True)
    mi.check(oracle, name, po, pl, want, want_lse, fmt, f"numpy kernel {name}")


# the family in which each wrong rule changes a live row: two rows per sequence for the fold and the limits, a raw length above the
# capacity for the clamp, more than 64 visible keys for the merge
WHERE = {"v_all_576": "h5", "v_last_512": "h5", "logits_512": "h16", "scale_512_only": "h16", "causal_at_start": "h48",
         "max_q_in_the_limit": "h5", "fold_transposed": "h48", "no_length_clamp": "h16", "lse_log2": "h1", "merge_without_l": "h5"}


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("wrong", mi.WRONG)
def test_check_rejects_wrong_kernels(oracle, wrong, fmt):
    name = WHERE[wrong]
    po, pl = mi.numpy_kernel(oracle, name, fmt, wrong=wrong)
    want, want_lse = mi.reference(oracle, name, fmt, True)
    with pytest.raises(AssertionError):
        mi.check(oracle, name, po, pl, want, want_lse, fmt, f"{wrong} on {name}")


def test_check_rejects_written_free_tokens_and_lost_zero_rows(oracle):
    """a kernel that writes a token of no sequence, and one that leaves something in a row without a key"""
    name = "h5"
    want, want_lse = mi.reference(oracle, name, 0, True)
    lay = mi.layout(name)
    po, pl = mi.numpy_kernel(oracle, name, 0)
    bad = po.copy()
    bad[np.flatnonzero(~lay.owned)[0]] = 0.0
    with pytest.raises(AssertionError):
        mi.check(oracle, name, bad, pl, want, want_lse, 0, "free token written")
    nokey = np.argwhere(dv.live_mask(lay, 5) & ~np.isfinite(want_lse))
    assert len(nokey), "h5 has rows without a key (L = 3 < n_b = 4)"
    r, i = nokey[0]
    bad = po.copy()
    bad[lay.tok[r // 5, i], r % 5, 7] = 1e-30
    with pytest.raises(AssertionError):
        mi.check(oracle, name, bad, pl, want, want_lse, 0, "row without a key not zero")


def test_families_hold_the_edges():
    """the shapes the GPU tier relies on: idle slot, overlong sequence, rows without a key, lengths at tile edges, clamps both ways"""
    lens = [x for f in mi.FAMILIES.values() for x in f["lens"]]
    for L in (1, 63, 64, 65, 200):
        assert L in lens
    assert min(lens) < 0 and any(f["lens"][b] > f["Ncap"] for f in mi.FAMILIES.values() for b in range(f["B"]))
    assert any(L == f["Ncap"] for f in mi.FAMILIES.values() for L in f["lens"])
    assert {f["Hq"] for f in mi.FAMILIES.values()} == {1, 5, 16, 48, 128}
    f = mi.family("h5")
    assert 0 in f["spans"] and max(f["spans"]) > f["max_q"] and any(0 < L < f["max_q"] for L in f["lens"])
    assert mi.family("h48")["Hq"] * max(mi.layout("h48").n) == 144
    for f in mi.FAMILIES.values():
        assert 256 <= f["Ncap"] <= 512 and f["B"] <= 4


def test_append_model_drops_and_skips():
    """the numpy model of fa_mla_append: drops at the capacity, a -1 table entry skips the write, lengths are clamped"""
    new = np.arange(6 * mi.DQK, dtype=np.uint16).reshape(6, mi.DQK)
    cache = np.zeros((2, 32, mi.DQK), np.uint16)
    out, after = mi.append_model(cache, new, [0, 4, 6], [30, -2], 6)
    assert (out[0, 30] == new[0]).all() and (out[0, 31] == new[1]).all() and list(after) == [32, 2]
    assert (out[1, 0] == new[4]).all() and (out[1, 1] == new[5]).all() and not out[1, 2:].any()
    pool = np.zeros((4, 16, mi.DQK), np.uint16)
    table = np.array([[2, -1], [0, 3]], np.int32)
    out, after = mi.append_model(pool, new, [0, 4, 6], [14, 16], 6, table=table)
    assert (out[2, 14] == new[0]).all() and (out[2, 15] == new[1]).all() and (out[3, 0] == new[4]).all()
    assert not out[1].any() and list(after) == [18, 18]
    assert cm.clamp(-2, 32) == 0
