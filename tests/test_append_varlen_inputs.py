"""CPU tier of tests/append_varlen_inputs.py: the case is the one the module describes, the packing and the composed expectation do
what they say, and every wrong kernel the module names changes at least one expected byte in every case it applies to -- so the GPU
tier's byte comparison tells each of them from the right kernel."""
import numpy as np
import pytest

import append_inputs as ai
import append_varlen_inputs as av
import common_inputs as cm
import rope_inputs as rp

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
FORMS = [pytest.param(*f, id=av.form_id(*f)) for f in av.FORMS]


def test_the_case_is_the_one_described():
    c, cu, total = av.CASE, av.cu_of(), av.total_of()
    assert cu.tolist() == [3, 40, 40, 41, 111, 123] and total == 132 and cu.dtype == np.int32
    bd = av.bounds(cu, total)
    assert [e - s for s, e in bd] == list(c["m"]) and bd[0][0] == 3 and total - bd[-1][1] == 9
    own = av.owned(cu, total)
    assert own.sum() == sum(c["m"]) and not own[:3].any() and not own[-9:].any()
    after = [min(L + m, c["Ncap"]) for L, m in zip(c["lens"], c["m"])]
    assert after == [42, 40, 96, 96, 12]
    assert c["lens"][3] + c["m"][3] > c["Ncap"] and c["lens"][2] + c["m"][2] == c["Ncap"]      # an overflow, and the last row
    # at d = 64 a workgroup of 256 chunks spans 32 (token, head) rows, 16 tokens of K or V: no boundary falls between two workgroups
    assert all(int(x) % (256 // 8 // c["Hkv"]) for x in cu)
    table, num_pages = av.make_table(c, cu, total)
    live = table[(table >= 0) & (table < num_pages)]
    assert num_pages == c["B"] * c["Ncap"] // c["ps"] + 3 and len(set(live.tolist())) == live.size == 3 + 3 + 6 + 6 + 1
    assert live.tolist() != sorted(live.tolist())                                                  # permuted
    assert (table[1, 3:] < 0).any() or (table[1, 3:] >= num_pages).any()                           # garbage behind the empty sequence


def test_clamps():
    assert av.bounds([-5, 10, 10, 500], 64) == [(0, 10), (10, 10), (10, 64)]
    assert av.bounds([7, 3, 200, 20], 64) == [(7, 7), (3, 64), (64, 64)]                          # e_b never below s_b, never past total
    assert av.owned([-5, 10, 10, 500], 64).all() and av.owned([5, 9], 16).sum() == 4


def test_gather_is_the_padded_head_major_copy():
    packed = np.arange(10 * 3 * 4, dtype=np.uint16).reshape(10, 3, 4)
    rows = av.token_rows(np.array([1, 4, 4, 9]), 10)
    assert rows == [[1, 2, 3], [], [4, 5, 6, 7, 8]]
    pad = av.gather(packed, rows, fill=7)
    assert pad.shape == (3, 3, 5, 4)
    for b, r in enumerate(rows):
        for i, t in enumerate(r):
            assert np.array_equal(pad[b, :, i], packed[t])
        assert (pad[b, :, len(r):] == 7).all()
    assert av.gather(packed, [[], []]).shape == (2, 3, 1, 4)                                       # Nnew = max m_b is at least 1


@pytest.mark.parametrize("paged,fp8,rope", FORMS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_expectation_token_by_token(fmt, d, paged, fp8, rope):
    """the composed expectation against the contract restated directly: one token at a time, nothing padded"""
    x, c = av.inputs(fmt, d, paged, fp8, rope), av.CASE
    want = av.model(fmt, d, paged, fp8, rope)
    k, v = np.array(x["kc0"]), np.array(x["vc0"])
    qout = np.full(x["qsrc"].shape, av.QOUT_NAN, np.uint16)
    ncap, ps, il = c["Ncap"], c["ps"], rope == 2
    kept = 0
    for b, (s, e) in enumerate(av.bounds(x["cu"], x["total"])):
        L = cm.clamp(c["lens"][b], ncap)
        for t in range(s, e):
            p = L + (t - s)
            r = min(p, x["cos"].shape[0] - 1)
            krow, vrow = x["knb"][t], x["vnb"][t]                                                  # [Hkv, d]
            if rope:
                kf = rp.rotate_fp32(ai.widen16(krow, fmt), x["cos"][r], x["sin"][r], il)
                qf = rp.rotate_fp32(ai.widen16(x["qsrc"][t], fmt), x["cos"][r], x["sin"][r], il)
                qout[t] = x["qsrc"][t]
                qout[t, :, :d // 2] = ai.round16_bits(qf[:, :d // 2], fmt)
                if not fp8:
                    krow = krow.copy()
                    krow[:, :d // 2] = ai.round16_bits(kf[:, :d // 2], fmt)
            else:
                kf = ai.widen16(krow, fmt)
            if fp8:
                krow = rp.fp8_codes(kf[None, :, None], x["ks"])[0, :, 0]
                vrow = rp.fp8_codes(ai.widen16(vrow, fmt)[None, :, None], x["vs"])[0, :, 0]
            if p >= ncap:
                continue
            if paged:
                page = int(x["table"][b, p // ps])
                assert 0 <= page < x["num_pages"]                                                  # every kept token has a page of its own
                k[page, :, p % ps], v[page, :, p % ps] = krow, vrow
            else:
                k[b, :, p], v[b, :, p] = krow, vrow
            kept += 1
    assert kept == sum(c["m"]) - 4
    assert np.array_equal(want["k"], k) and np.array_equal(want["v"], v)
    assert want["lens"].tolist() == [42, 40, 96, 96, 12]
    if rope:
        assert np.array_equal(want["qout"], qout)
        own = av.owned(x["cu"], x["total"])
        assert (want["qout"][~own] == av.QOUT_NAN).all() and not (want["qout"][own] == av.QOUT_NAN).any()
    else:
        assert want["qout"] is None
    nan = 0x7F if fp8 else cm.NAN16
    untouched = (want["k"] == nan).all(-1)
    assert untouched.sum() == untouched.size - kept * c["Hkv"]                                      # everything else is as it was


@pytest.mark.parametrize("paged,fp8,rope", FORMS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_every_wrong_kernel_changes_a_byte(fmt, d, paged, fp8, rope):
    right = av.model(fmt, d, paged, fp8, rope)
    for wrong in av.WRONG:
        if wrong in av.ROTARY_ONLY and not rope:
            continue
        got = av.model(fmt, d, paged, fp8, rope, wrong=wrong)
        differs = [name for name in ("k", "v", "qout", "lens") if right[name] is not None and not np.array_equal(right[name], got[name])]
        assert differs, wrong
        if wrong in ("writes_dead_qout", "hkv_for_hq"):
            assert differs == ["qout"], (wrong, differs)
        if wrong == "rotates_at_i":
            assert "k" in differs and "qout" in differs and "v" not in differs
