"""CPU tier of tests/decode_varlen_inputs.py: the packing by hand, the check on the entry as specified, and the property that makes the
GPU tier meaningful -- each of six numpy "wrong kernels" is rejected by the very check the GPU test applies."""
import numpy as np
import pytest

import common_inputs as cm
import decode_varlen_inputs as dv
import ragged_inputs as ri


def test_layouts_by_hand():
    lay = dv.layout("spec")                      # n = (8, 3, 1, 0, 8), max_q = 8; sequence 0 owns 2 tokens more than it has rows
    assert lay.cu.tolist() == [3, 13, 16, 17, 17, 25] and lay.total_q == 27 and lay.max_q == 8
    assert lay.tok[0].tolist() == list(range(3, 11)) and lay.tok[1].tolist() == [13, 14, 15] + [-1] * 5 and (lay.tok[3] == -1).all()
    assert np.flatnonzero(~lay.owned).tolist() == [0, 1, 2, 11, 12, 25, 26]
    lay = dv.layout("split")                     # no sequence at max_q: lead and trail only
    assert lay.cu.tolist() == [3, 6, 6] and np.flatnonzero(~lay.owned).tolist() == [0, 1, 2, 6, 7]
    lay = dv.layout("tail")                      # every n_b = max_q
    assert lay.n == [40, 40] and lay.cu.tolist() == [3, 45, 85] and not lay.owned[43:45].any()
    lay = dv.layout("overlong")                  # spans (9, 2, 0, 6) against max_q = 4
    assert lay.n == [4, 2, 0, 4] and lay.cu.tolist() == [3, 12, 14, 14, 20] and lay.total_q == 22
    assert np.flatnonzero(~lay.owned).tolist() == [0, 1, 2, 7, 8, 9, 10, 11, 18, 19, 20, 21]
    assert any(e - s > lay.max_q for s, e in zip(lay.cu[:-1], lay.cu[1:]))


def test_pack_and_unpack_are_inverse():
    lay = dv.layout("overlong")
    padded = np.arange(4 * 4 * 4 * 2, dtype=np.float32).reshape(16, 4, 2) + 1
    packed = dv.pack_rows(lay, padded, -1.0)
    assert packed.shape == (22, 4, 2) and (packed[~lay.owned] == -1).all()
    assert np.array_equal(packed[3 + 2, 1], padded[1, 2]) and np.array_equal(packed[14 + 3, 2], padded[3 * 4 + 2, 3])
    back = dv.unpack_rows(lay, packed, 4)
    live = dv.live_mask(lay, 4)
    assert np.array_equal(back[live], padded[live]) and (back[~live] == 0).all()
    assert dv.pack_lse(lay, padded[..., 0], 0.0).shape == (4, 22)


CASES = [("spec", True, 0, "none"), ("spec", True, 100, "both"), ("blocks", True, 0, "none"), ("split", True, 0, "sinks"),
         ("overlong", True, 0, "none"), ("overlong", False, 100, "sinks")]


@pytest.mark.parametrize("name,causal,W,variant", CASES)
def test_the_specified_entry_passes_the_check(oracle, name, causal, W, variant):
    want, want_lse = dv.reference(oracle, name, 64, 0, W, causal, variant)
    po, pl = dv.numpy_kernel(oracle, name, 64, 0, W, causal, variant)
    dv.check(oracle, dv.layout(name), po, pl, want, want_lse, 0, f"{name} as specified")


# the family on which each wrong rule is judged: one whose shape makes the rule differ from the right one
WRONG_ON = {
    "ignores_s_b": ("spec", "none"),               # LEAD = 3 shifts every token
    "max_q_in_the_limit": ("spec", "none"),        # n_b < max_q for sequences 1 and 2 (the boosted tail keys decide)
    "ignores_q_stride_h": ("spec", "none"),        # G = 4 heads per group
    "lse_token_major": ("spec", "none"),
    "zeros_in_free_tokens": ("overlong", "none"),
    "sink_per_split": ("split", "sinks"),          # S > 1
}


@pytest.mark.parametrize("fmt,d", [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)])
@pytest.mark.parametrize("wrong", dv.WRONG)
def test_every_wrong_kernel_is_rejected(oracle, wrong, fmt, d):
    name, variant = WRONG_ON[wrong]
    S = dv.want_S(name, 0)
    assert name != "split" or S > 1
    want, want_lse = dv.reference(oracle, name, d, fmt, 0, True, variant)
    right = dv.numpy_kernel(oracle, name, d, fmt, 0, True, variant)
    dv.check(oracle, dv.layout(name), *right, want, want_lse, fmt, "the entry as specified")
    po, pl = dv.numpy_kernel(oracle, name, d, fmt, 0, True, variant, wrong=wrong, S=S)
    with pytest.raises(AssertionError):
        dv.check(oracle, dv.layout(name), po, pl, want, want_lse, fmt, wrong)


def test_the_overlong_family_cuts_at_max_q(oracle):
    """rows past max_q of an over-long sequence are no rows: the reference has n_b = max_q live rows, whose causal limits end at L_b"""
    f = dv.family("overlong")
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    lo, c, live = ri.limits(f["lens"], f["nq"], B, Hkv, G, Nq, Ncap, True, 0)
    assert c[0].tolist() == [197, 198, 199, 200] and c[Hkv * G].tolist() == [76, 77, 0, 0] and not live[2 * Hkv * G].any()
    assert c[3 * Hkv * G].tolist() == [0, 1, 2, 3]   # L = 3 < n = 4: the first row sees nothing and is live all the same
    want, want_lse = dv.reference(oracle, "overlong", 64, 0, 0, True)
    assert (want_lse[3 * Hkv * G:, 0] == -np.inf).all() and np.isfinite(want_lse[3 * Hkv * G:, 1:]).all()
