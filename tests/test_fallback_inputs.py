"""CPU tier of tests/test_gpu_fallback_paths.py: the hostile inputs do what they claim.  For every input the GPU tests build, the
log2-scaled scores are computed in float64 numpy from the 16-bit-rounded values and the forcing condition the case is named
for is asserted (fallback_inputs.assert_*: the same assertions the GPU tests repeat before they trust a result), and the
oracle's output for it is finite everywhere.  These are conditions on seeded inputs, not measurements of a kernel."""
import numpy as np
import pytest

import fallback_inputs as fi

FMT_D = [pytest.param(fmt, d, id=f"{'fp16' if fmt == 0 else 'bf16'}-d{d}") for d in (64, 128) for fmt in (0, 1)]


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_chain_inputs(oracle, fmt, d):
    """Lift >= 21 (fp16) / >= 129 or in (96, 127) (bf16) on every spiked row, <= 19.5 on the must-stay row, head 0 within +-16 of
    its tile-0 maxima, spiked keys visible, the huge key invisible to the rows before it."""
    for n in fi.CHAIN_N[d]:
        case = fi.chain_case(oracle, d, n, fmt)
        fi.assert_chain_case(case, fmt)
        want = oracle.forward(case["q"], case["k"], case["v"], causal=True, accum=1, nthreads=8)
        assert np.isfinite(want).all()
        # row 0 sees one key
        assert np.array_equal(want[:, 0], case["v"][:, 0])


@pytest.mark.parametrize("fmt", [0, 1])
def test_large_grid_inputs(oracle, fmt):
    for (bh, n, d) in ((300, 600, 64), (300, 300, 128)):
        case = fi.large_grid_case(oracle, bh, n, d, fmt)
        fi.assert_large_grid_case(case, fmt)
        for b in (0, 151, 299):
            want = oracle.forward(case["q"][b:b + 1], case["k"][b:b + 1], case["v"][b:b + 1], causal=True, accum=1, nthreads=8)
            assert np.isfinite(want).all()


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_plain_inputs(oracle, fmt, d):
    for n in ((640, 333) if d == 64 else (300, 400)):
        case = fi.plain_case(oracle, d, n, fmt)
        fi.assert_plain_case(case, fmt)
        assert np.isfinite(oracle.forward(case["q"], case["k"], case["v"], accum=1, nthreads=8)).all()


def test_plain_inputs_match_the_parity_test(oracle):
    """plain_case(d = 64, n = 640) rebuilds the input of test_optimistic_pass_overflow_fallback value for value."""
    for fmt in (0, 1):
        n, d, bh = 640, 64, 3
        (q, k, v), _ = oracle.make_qkv(bh, n, d, fmt, seed=777 + fmt)
        ln2 = float(np.log(2.0))

        def spike(b, qi, key, log2_above):
            s0 = (q[b, qi] @ k[b, :64].T) / np.sqrt(d)
            target = (s0.max() + log2_above * ln2) * np.sqrt(d)
            k[b, key] = q[b, qi] * (target / float(q[b, qi] @ q[b, qi]))

        spike(0, 5, n - 1, 40.0)
        spike(0, 300, 100, 19.0)
        spike(1, 77, 333, 21.5)
        spike(1, 78, 334, 150.0 if fmt == 1 else 60.0)
        k[2, 64:] *= 6.0
        case = fi.plain_case(oracle, d, n, fmt)
        for mine, theirs in zip(case["bits"], (q, k, v)):
            assert np.array_equal(mine, oracle.encode16(oracle.decode16(oracle.encode16(theirs, fmt), fmt), fmt))


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_splitkv_inputs(oracle, fmt, d):
    """The staircase rises by < 8 per tile and by > 20 in total; the jumps are 40 / 150 / 210; each key is benign for the other rows."""
    for nk in (8229, 200):
        case = fi.splitkv_case(oracle, d, fmt, nk)
        fi.assert_splitkv_case(case)
        assert np.isfinite(oracle.forward_cross(case["q"], case["k"], case["v"], accum=1, nthreads=8)).all()


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_kvcache_inputs(oracle, fmt, d):
    """Spikes on keys only the last rows see at length 66 and in a late split of the full sequence; one head near -300 and one
    near +300 log2 units."""
    case = fi.kvcache_case(oracle, d, fmt)
    G = fi.KV_SHAPE["G"]
    for causal in (False, True):
        fi.assert_kvcache_case(case, causal)
    for h in range(case["q"].shape[0]):
        L = fi.KV_LENS[h // G]
        want = oracle.forward_cross(case["q"][h:h + 1], case["k"][h // G:h // G + 1, :L], case["v"][h // G:h // G + 1, :L], accum=1, nthreads=8)
        assert np.isfinite(want).all()
