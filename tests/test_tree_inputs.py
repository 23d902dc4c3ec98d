"""CPU tier of the tree step's inputs (tests/tree_inputs.py): the float64 reference against a brute-force visibility and against
cm.expected_f64 on the triangle, fa.tree_from_parents against a python walk, and the wrong kernels: for each mistake the tree tier
names, a numpy model of that kernel FAILS the check the GPU tests apply (dv.check, the project's bounds) on at least one family while
the reference's own kernel passes it.  That pins the inputs: the right rule stays inside the tolerance, every listed mistake outside.
"""
import numpy as np
import pytest

import append_varlen_inputs as av
import common_inputs as cm
import decode_varlen_inputs as dv
import ragged_inputs as ri
import tree_inputs as ti

D, FMT = 64, 0
SMALL = ("chain_and_fan", "wide")     # split's 8000 keys add nothing to the rule and cost the reference seconds


@pytest.mark.parametrize("name", ti.NAMES)
def test_visibility_is_the_brute_force_rule(name):
    f, lay = ti.family(name), ti.layout(name)
    for kind in ti.TREES:
        words = ti.tree(name, kind)[0]
        for W in ti.WINDOWS:
            got = ti.visibility(lay, f["lens"], f["Ncap"], f["G"], words, W)
            want = ti.brute_visibility(lay, f["lens"], f["Ncap"], words, W)
            for b, (g, w) in enumerate(zip(got, want)):
                assert (g == w[None]).all(), (name, kind, W, b)
                if lay.n[b] and f["lens"][b] >= lay.n[b]:
                    assert g[0].any(axis=1).all(), "a row with its own key in range sees at least itself"


def test_families_cover_the_edges():
    f, lay = ti.family("chain_and_fan"), ti.layout("chain_and_fan")
    base = [L - n for L, n in zip(f["lens"], lay.n)]
    assert lay.n == [8, 3, 1, 0, 8] and base == [292, 126, 63, 7, -3]
    assert 0 in lay.n and min(base) < 0                          # an idle slot; base < 0
    assert base[1] // 64 != (f["lens"][1] - 1) // 64             # a tail across a tile edge
    w = ti.family("wide")
    assert ti.layout("wide").n == [64, 33] and w["G"] * w["Nq"] == 256
    assert int(ti.tree("wide", "chain")[0][ti.layout("wide").s[0] + 63]) >> 63 == 1      # bit 63 in use
    words = ti.tree("wide", "random")[0]
    s1 = ti.layout("wide").s[1]
    assert any(int(words[s1 + i]) >> 33 for i in range(33)), "junk above n_b"
    assert any(int(words[s1 + i]) & ((1 << 33) - 1) >> (i + 1) for i in range(33)), "a bit above the row's own"
    assert any(not (int(words[s1 + i]) >> i) & 1 for i in range(33)), "a row without its self bit"
    assert ri.want_S(ti.family("split"), 0) > 1                  # the tail (keys 7997 .. 7999) lies in the last split's last tile


@pytest.mark.parametrize("W", ti.WINDOWS)
@pytest.mark.parametrize("name", SMALL)
def test_triangle_is_the_causal_reference(oracle, name, W):
    f = ti.family(name)
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), _ = ti.inputs(oracle, name, D, FMT)
    want = cm.expected_f64(q, k, v, f["lens"], B, Hkv, G, Nq, True, W, nq=f["nq"])
    got = ti.reference(oracle, name, D, FMT, "triangle", W)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _walk(parents, cu):
    mask, depth = np.zeros(len(parents), np.uint64), np.zeros(len(parents), np.int32)
    for b in range(len(cu) - 1):
        par = [int(x) for x in parents[cu[b]:cu[b + 1]]]
        w, dp = ti.closed_masks(par)
        mask[cu[b]:cu[b + 1]], depth[cu[b]:cu[b + 1]] = np.array(w, np.uint64), dp
    return mask, depth


def test_tree_from_parents(fa):
    import torch
    rng = np.random.default_rng(5)
    cu = [2, 10, 10, 74, 79]                    # two tokens of no sequence in front, an empty sequence, one of 64, three behind
    parents = np.full(82, -1, np.int32)
    for (s, e), kind in zip(zip(cu[:-1], cu[1:]), ("chain", "star", "random", "star")):
        parents[s:e] = ti.parents_of(kind, e - s, rng)
    mask, depth = fa.tree_from_parents(torch.from_numpy(parents), torch.tensor(cu, dtype=torch.int32))
    assert mask.dtype == torch.int64 and depth.dtype == torch.int32 and mask.shape == depth.shape == (82,)
    want_m, want_d = _walk(parents, cu)
    assert np.array_equal(mask.numpy().view(np.uint64), want_m) and np.array_equal(depth.numpy(), want_d)
    chain = mask.numpy().view(np.uint64)[2:10]
    assert [int(x) for x in chain] == [(1 << (i + 1)) - 1 for i in range(8)], "a chain is the triangle"
    assert int(want_m[10 + 63]) >> 63 == 1 and int(mask[10 + 63]) < 0, "bit 63 is the word's sign bit"
    assert (mask[:2] == 0).all() and (mask[79:] == 0).all()
    with pytest.raises(ValueError):
        fa.tree_from_parents(torch.full((65,), -1, dtype=torch.int32), torch.tensor([0, 65], dtype=torch.int32))
    for bad in ([-1, 1], [-1, 0, 2], [-2]):
        with pytest.raises(ValueError):
            fa.tree_from_parents(torch.tensor(bad, dtype=torch.int32), torch.tensor([0, len(bad)], dtype=torch.int32))


def _passes(oracle, name, kind, W, wrong):
    lay = ti.layout(name)
    want, want_lse = ti.reference(oracle, name, D, FMT, kind, W)
    o, lse = ti.numpy_kernel(oracle, name, D, FMT, kind, W, wrong)
    try:
        dv.check(oracle, lay, o, lse, want, want_lse, FMT, f"{name} {kind} W={W} {wrong}")
    except AssertionError:
        return False
    return True


def test_the_reference_kernel_passes_the_check(oracle):
    for name in SMALL:
        for kind in ti.TREES:
            for W in ti.WINDOWS:
                assert _passes(oracle, name, kind, W, None), (name, kind, W)


@pytest.mark.parametrize("wrong", ti.WRONG)
def test_wrong_kernels_fail_the_check(oracle, wrong):
    failed = [(name, kind, W) for name in SMALL for kind in ti.TREES for W in ti.WINDOWS if not _passes(oracle, name, kind, W, wrong)]
    print(wrong, "fails on", failed)
    assert failed, f"a kernel with the rule `{wrong}` passes every family: the inputs do not pin it"


# ---- the append with positions ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("k", "v", "lens", "qout"))


@pytest.mark.parametrize("rope", [1, 2])
def test_append_positions_model(rope):
    x = av.inputs(FMT, D, False, False, rope)
    slot = ti.append_model(FMT, D, False, False, rope, ti.append_positions(x, "slot"))
    assert _same(slot, av.model(FMT, D, False, False, rope)), "positions = L_b + i is the plain append"
    pos = ti.append_positions(x)
    assert (pos[av.owned(x["cu"], x["total"])] >= av.CASE["max_pos"]).any() and (pos < 0).any()
    right = ti.append_model(FMT, D, False, False, rope, pos)
    assert not _same(right, slot)
    assert np.array_equal(right["v"], slot["v"]) and np.array_equal(right["lens"], slot["lens"]), "V and the lengths do not depend on positions"
    for wrong in ti.APPEND_WRONG:
        assert not _same(ti.append_model(FMT, D, False, False, rope, pos, wrong), right), wrong
