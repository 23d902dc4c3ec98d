"""CPU tier of the fp8 MLA entries fa_mla_decode_fp8 and fa_mla_append_fp8, through the C ABI: the symbols are exported and bound,
every refusal of the 16-bit entries (the lists of tests/test_mla_host.py, imported as they are) holds for the new entries with and
without a scale, a misaligned c_scale is refused, and the workspace size is the 16-bit entry's for the same descriptor.  Only calls
that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os
import subprocess

import pytest

import test_mla_host as host

INVALID = host.INVALID
SCALES = [None, 256]   # no scale (1.0), and a made-up 4-byte-aligned address


def _call(fa, paged=False, c_scale=None, **kw):
    return fa.lib().fa_mla_decode_fp8(ctypes.byref(host._desc(fa, paged, **kw)), c_scale)


def _bytes8(fa, paged=False, **kw):
    return fa.lib().fa_mla_decode_fp8_workspace_bytes(ctypes.byref(host._desc(fa, paged, **kw)))


def _append(fa, paged=False, c_scale=None, **kw):
    return fa.lib().fa_mla_append_fp8(ctypes.byref(host._adesc(fa, paged, **kw)), c_scale)


def test_symbols(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    D, A = fa.capi.MlaDecodeDesc, fa.capi.MlaAppendDesc
    for n in ("fa_mla_decode_fp8_workspace_bytes", "fa_mla_decode_fp8", "fa_mla_append_fp8"):
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
    assert L.fa_mla_decode_fp8.argtypes == [ctypes.POINTER(D), ctypes.c_void_p] and L.fa_mla_decode_fp8.restype is ctypes.c_int
    assert L.fa_mla_append_fp8.argtypes == [ctypes.POINTER(A), ctypes.c_void_p] and L.fa_mla_append_fp8.restype is ctypes.c_int
    assert L.fa_mla_decode_fp8_workspace_bytes.argtypes == [ctypes.POINTER(D)]
    assert L.fa_mla_decode_fp8_workspace_bytes.restype is ctypes.c_size_t
    for name in ("fa_mla_decode_fp8", "fa_mla_append_fp8", "quantize_mla_fp8"):
        assert callable(getattr(fa, name)) and name in fa.__all__


def test_header_is_plain_c(tmp_path):
    """the three declarations compile as C99 and take the 16-bit entries' descriptors"""
    src = tmp_path / "hdr8.c"
    src.write_text('#include "fa_mi355.h"\nint main(void) { fa_mla_decode_desc d = {0}; fa_mla_append_desc a = {0}; const float* s = 0; '
                   'int (*f)(const fa_mla_decode_desc*, const float*) = fa_mla_decode_fp8; '
                   'int (*g)(const fa_mla_append_desc*, const float*) = fa_mla_append_fp8; '
                   'size_t (*w)(const fa_mla_decode_desc*) = fa_mla_decode_fp8_workspace_bytes; '
                   'd.size = sizeof d; a.size = sizeof a; return f == 0 || g == 0 || w == 0 || s != 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(host.ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "hdr8.o")])


@pytest.mark.parametrize("scale", SCALES, ids=["no_scale", "scale"])
def test_the_good_descriptor_is_only_short_of_a_workspace(fa, scale):
    for paged in (False, True):
        need = _bytes8(fa, paged)
        assert need > 0
        assert _call(fa, paged, scale) == INVALID
        assert _call(fa, paged, scale, workspace=4096, workspace_bytes=need - 1) == INVALID
        assert _call(fa, paged, scale, workspace=4100, workspace_bytes=need) == INVALID
        assert _bytes8(fa, paged, num_splits=1) == 0


@pytest.mark.parametrize("scale", SCALES, ids=["no_scale", "scale"])
@pytest.mark.parametrize("bad", host.BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_rejected_before_the_device(fa, bad, scale):
    for paged in (False, True):
        assert _call(fa, paged, scale, **bad) == INVALID
        assert _call(fa, paged, scale, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID
        assert _bytes8(fa, paged, **bad) == 0


@pytest.mark.parametrize("addr", [257, 258, 259, 6])
def test_a_misaligned_c_scale_is_refused(fa, addr):
    """with every other argument good, one split (no workspace needed): the scale's address alone refuses the call"""
    for paged in (False, True):
        assert _call(fa, paged, addr, num_splits=1) == INVALID
        assert _call(fa, paged, addr, workspace=4096, workspace_bytes=1 << 40) == INVALID
        assert _append(fa, paged, addr) == INVALID


def test_null_descriptor(fa):
    L = fa.lib()
    assert L.fa_mla_decode_fp8(None, None) == INVALID and L.fa_mla_decode_fp8_workspace_bytes(None) == 0
    assert L.fa_mla_append_fp8(None, None) == INVALID and L.fa_mla_decode_fp8(None, 256) == INVALID


@pytest.mark.parametrize("bad", [dict(Ncap=0), dict(Ncap=-5), dict(Ncap=(1 << 30) + 1)], ids=str)
def test_bad_capacity(fa, bad):
    assert _call(fa, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID and _bytes8(fa, **bad) == 0
    assert _append(fa, **bad) == INVALID


@pytest.mark.parametrize("bad", [dict(num_pages=0), dict(max_pages=0), dict(page_size=8), dict(page_size=24), dict(page_size=0),
                                 dict(max_pages=1 << 27), dict(block_table=18)], ids=str)
def test_bad_page_geometry(fa, bad):
    assert _call(fa, True, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID and _bytes8(fa, True, **bad) == 0
    assert _append(fa, True, **bad) == INVALID


def test_workspace_is_the_16_bit_entrys(fa):
    """the same function of the same descriptor: every shape of test_mla_host's sizing test, and the automatic choice"""
    shapes = [dict(num_splits=s) for s in (0, 1, 2, 3, 4)] + [dict(Hq=128), dict(max_q=8, total_q=16), dict(B=4), dict(in_dtype=1, out_dtype=1),
              dict(num_splits=0, Ncap=32768, B=1, Hq=16, max_q=1, total_q=1), dict(num_splits=0, Ncap=4096, B=8, Hq=128, max_q=1, total_q=8)]
    seen = set()
    for kw in shapes:
        for paged in (False, True):
            if paged and "Ncap" in kw:
                continue
            got = _bytes8(fa, paged, **kw)
            assert got == host._bytes(fa, paged, **kw), kw
            seen.add(got)
    assert 0 in seen and len(seen) >= 5
    assert fa.mla_decode_workspace_bytes(1, 16, 1, Ncap=32768) == _bytes8(fa, num_splits=0, Ncap=32768, B=1, Hq=16, max_q=1, total_q=1)


@pytest.mark.parametrize("scale", SCALES, ids=["no_scale", "scale"])
@pytest.mark.parametrize("bad", host.ABAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_append_rejected_before_the_device(fa, bad, scale):
    for paged in (False, True):
        assert _append(fa, paged, scale, **bad) == INVALID


def test_front_ends_judge_the_cache_first(fa):
    """a cache that is not float8_e4m3fn is refused with the fp8 tiers' message before anything else is looked at"""
    import torch
    for bad in (torch.zeros(1, 16, 576, dtype=torch.float16), torch.zeros(1, 16, 576, dtype=torch.float8_e5m2), None):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            fa.fa_mla_decode_fp8("not a tensor", bad, None, 1)
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            fa.fa_mla_append_fp8("not a tensor", bad, None)
    c8 = torch.zeros(1, 16, 576, dtype=torch.float8_e4m3fn)
    q = torch.zeros(1, 4, 576, dtype=torch.float16)
    cu = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(ValueError, match="c_scale"):
        fa.fa_mla_decode_fp8(q, c8, cu, 1, c_scale=torch.ones(2))
    with pytest.raises(ValueError, match="c_scale"):
        fa.fa_mla_append_fp8(q[:, 0], c8, cu, c_scale=torch.ones(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="fa_mla_decode_fp8"):   # the 16-bit entry points an fp8 cache to its own entry
        fa.fa_mla_decode(q, c8, cu, 1)
