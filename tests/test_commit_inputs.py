"""CPU tier of fa_kvcache_commit's test inputs: the numpy model of tests/commit_inputs.py agrees with a sequential ascending-order move
written from the header's sentences alone, and the inputs the GPU tier runs reject every wrong kernel of commit_inputs.WRONG: for
each one some run's bytes or lengths differ from the rule's.  No GPU, no library."""
import numpy as np
import pytest

import commit_inputs as cmi

FORM_D = [pytest.param(p, f, d, id=f"{cmi.form_id(p, f)}-d{d}") for p, f in cmi.FORMS for d in (64, 128)]


@pytest.mark.parametrize("paged,fp8,d", FORM_D)
def test_model_is_the_sequential_move(paged, fp8, d):
    for name, table, mode in cmi.gpu_cases(paged):
        x = cmi.inputs(name, d, paged, fp8, table, mode)
        got = cmi.expected(name, d, paged, fp8, table, mode)
        want = cmi.brute(x["k0"], x["v0"], x["words"], x["lens"], x["max_new"], x["table"])
        for g, w, n in zip(got, want, ("k", "v", "lens")):
            assert np.array_equal(g, w), (name, table, mode, n)


def test_the_inputs_hold_what_the_module_says():
    for name in cmi.NAMES:
        c = cmi.CASES[name]
        assert len(c["words"]) == len(c["lens"]) == cmi.B
        assert cmi.NCAP - 3 in c["lens"] and 13 in c["lens"]
    w = cmi.CASES["wide"]["words"]
    assert 0 in w and cmi.ALL in w and 1 << 63 in w and 0b1010 in w and 0b1100101 in w and 0b11111 in w
    assert all(x >> 8 for x in cmi.CASES["narrow"]["words"]), "every narrow word carries bits at or above max_new"
    assert min(cmi.CASES["narrow"]["lens"]) < 0 and max(cmi.CASES["narrow"]["lens"]) > cmi.NCAP
    for paged, fp8 in cmi.FORMS:
        x = cmi.inputs("wide", 64, paged, fp8)
        rows = x["k0"].reshape(-1, 64)
        assert len({r.tobytes() for r in rows}) == len(rows), "every row differs from every other"
        if fp8:
            assert (x["k0"] == 0x7F).any() and (x["k0"] == 0xFF).any()
        else:
            nan = ((x["k0"] & 0x7C00) == 0x7C00) & ((x["k0"] & 0x03FF) != 0)        # fp16 NaN patterns (bf16: exponent 0x7F80)
            assert nan.sum() > 100 and (((x["k0"] & 0x7F80) == 0x7F80) & ((x["k0"] & 0x7F) != 0)).sum() > 100
        if paged:
            named = set(x["table"].ravel().tolist())
            assert len(named) == cmi.B * cmi.MAX_PAGES and len(set(range(cmi.NUM_PAGES)) - named) == 3, "three guard pages"
            holes = cmi.inputs("wide", 64, paged, fp8, "holes")["table"]
            assert ((holes[1] < 0) | (holes[1] >= cmi.NUM_PAGES)).all(), "the whole row of a prefix word is garbage"
            assert not 0 <= holes[4, 5] < cmi.NUM_PAGES


def test_moves_cross_a_page_and_overlap():
    """{1,3} at L = 13: slot 14 is the source of move 0 and the destination of move 1, and 16 -> 14 crosses the boundary of a page"""
    c = cmi.CASES["wide"]
    moves = cmi.right_moves(c["words"][2], c["lens"][2], 64, cmi.NCAP)
    assert moves == [(14, 13), (16, 14)]
    assert cmi.right_moves(c["words"][3], c["lens"][3], 64, cmi.NCAP) == [(125, 125), (127, 126)], "bits 5 and 6 dropped at the capacity"
    assert cmi.right_moves(c["words"][4], c["lens"][4], 64, cmi.NCAP) == [(93, 30)]
    n = cmi.CASES["narrow"]
    assert cmi.right_moves(n["words"][0], n["lens"][0], 8, cmi.NCAP) == [(13, 13), (15, 14), (18, 15), (19, 16)]


@pytest.mark.parametrize("wrong", cmi.WRONG)
def test_wrong_kernels_are_rejected(wrong):
    paged_only = wrong in ("dst_through_src_page", "identity_needs_its_page")
    caught = []
    for paged, fp8 in cmi.FORMS:
        for name, table, mode in cmi.gpu_cases(paged):
            good = cmi.expected(name, 64, paged, fp8, table, mode)
            bad = cmi.expected(name, 64, paged, fp8, table, mode, wrong)
            if not all(np.array_equal(g, b) for g, b in zip(good, bad)):
                caught.append((paged, fp8, name, table, mode))
    assert caught, f"no run tells the rule from {wrong}"
    if not paged_only:
        assert {c[:2] for c in caught} == set(cmi.FORMS), f"{wrong} passes on a form: {caught}"
    else:
        assert {c[1] for c in caught} == {False, True} and all(c[0] for c in caught)
