"""CPU tier of fa_forward_varlen_kvcache_d256_fp8, through the C ABI with a null stream: every refusal of the 16-bit entry
(tests/test_varlen256_host.py's bad fields, imported), a misaligned scale and a null descriptor hold before the device is touched.
Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes

import pytest

import test_varlen256_host as base


def _cache8(fa, k_scale=None, v_scale=None, **kw):
    return fa.lib().fa_forward_varlen_kvcache_d256_fp8(ctypes.byref(base._cache_desc(fa, **kw)), k_scale, v_scale)


@pytest.mark.parametrize("bad", base.BAD_BOTH + base.BAD_CACHE, ids=base.ids)
def test_refused_before_the_device(fa, bad):
    assert _cache8(fa, **bad) == base.INVALID and _cache8(fa, 64, 128, **bad) == base.INVALID
    if "paged" not in bad and "Ncap" not in bad:
        assert _cache8(fa, paged=True, **bad) == base.INVALID


@pytest.mark.parametrize("scales", [(6, None), (None, 10), (64, 129), (4097, 4096)])
def test_misaligned_scales_and_a_null_descriptor(fa, scales):
    assert _cache8(fa, *scales) == base.INVALID and _cache8(fa, *scales, paged=True) == base.INVALID
    assert fa.lib().fa_forward_varlen_kvcache_d256_fp8(None, None, None) == base.INVALID

