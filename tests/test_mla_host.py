"""CPU tier of the MLA entries fa_mla_decode and fa_mla_append, through the C ABI: the symbols are exported and bound, the ctypes
structures mirror the header, every refusal the header lists holds before the device is touched, and the sizing function follows
(B, Hq, max_q, capacity, num_splits).  Only calls that must be rejected are issued, so the file is safe where a GPU is visible: a
descriptor that passes the checks shows it through fa_mla_decode_workspace_bytes, which is 0 for every descriptor the call refuses."""
import ctypes
import os
import subprocess

import pytest

import test_kvcache_ragged_host as ragged

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(fa, paged=False, **kw):
    """a descriptor with small made-up addresses that passes every check but the workspace's: two splits, no workspace given"""
    f = dict(Q=4096, O=8192, C=16, cu_seqlens_q=16, B=2, Hq=16, total_q=8, max_q=2, q_stride_t=16 * 576, q_stride_h=576,
             o_stride_t=16 * 512, o_stride_h=512, scale=0.04, causal=1, num_splits=2, in_dtype=0, out_dtype=0)
    if paged:
        f.update(block_table=16, num_pages=8, page_size=16, max_pages=16)
    else:
        f.update(Ncap=256)
    f.update(kw)
    return fa.capi.MlaDecodeDesc(**f)


def _call(fa, paged=False, **kw):
    return fa.lib().fa_mla_decode(ctypes.byref(_desc(fa, paged, **kw)))


def _bytes(fa, paged=False, **kw):
    return fa.lib().fa_mla_decode_workspace_bytes(ctypes.byref(_desc(fa, paged, **kw)))


def test_symbols_and_structs(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    for n in ("fa_mla_decode_workspace_bytes", "fa_mla_decode", "fa_mla_append"):
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
    D, A = fa.capi.MlaDecodeDesc, fa.capi.MlaAppendDesc
    assert L.fa_mla_decode.argtypes == [ctypes.POINTER(D)] and L.fa_mla_decode.restype is ctypes.c_int
    assert L.fa_mla_decode_workspace_bytes.argtypes == [ctypes.POINTER(D)] and L.fa_mla_decode_workspace_bytes.restype is ctypes.c_size_t
    assert L.fa_mla_append.argtypes == [ctypes.POINTER(A)] and L.fa_mla_append.restype is ctypes.c_int
    dec, app = ragged._header_fields("fa_mla_decode_desc"), ragged._header_fields("fa_mla_append_desc")
    assert dec == [f[0] for f in D._fields_] and dec[0] == "size" and dec[-1] == "stream"
    assert app == [f[0] for f in A._fields_] and app[0] == "size" and app[-1] == "stream"
    assert D().size == ctypes.sizeof(D) and fa.capi.new_desc(A).size == ctypes.sizeof(A)
    header = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    for text in ("#define FA_MLA_DC  512", "#define FA_MLA_DR  64", "#define FA_MLA_DQK 576"):
        assert text in header
    assert (fa.capi.MLA_DC, fa.capi.MLA_DR, fa.capi.MLA_DQK) == (512, 64, 576)
    for name in ("fa_mla_decode", "mla_decode_workspace_bytes", "fa_mla_append"):
        assert callable(getattr(fa, name)) and name in fa.__all__


def test_header_is_plain_c(tmp_path):
    """include/fa_mi355.h with the two new structures still compiles as C99 on its own, and both can be filled in from C"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "fa_mi355.h"\nint main(void) { fa_mla_decode_desc d = {0}; fa_mla_append_desc a = {0}; d.size = sizeof d; '
                   'a.size = sizeof a; d.q_stride_t = FA_MLA_DQK; d.o_stride_t = FA_MLA_DC; a.new_stride_t = FA_MLA_DC + FA_MLA_DR; '
                   'd.num_splits = 0; return d.C != 0 || a.Cnew != 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "hdr.o")])


def test_the_good_descriptor_is_only_short_of_a_workspace(fa):
    """the base descriptors pass every other check: they size a workspace, and the call stops at the missing one"""
    for paged in (False, True):
        need = _bytes(fa, paged)
        assert need > 0
        assert _call(fa, paged) == INVALID                                               # NULL workspace
        assert _call(fa, paged, workspace=4096, workspace_bytes=need - 1) == INVALID     # too small
        assert _call(fa, paged, workspace=4100, workspace_bytes=need) == INVALID         # misaligned
        assert _bytes(fa, paged, num_splits=1) == 0                                      # one pass: no workspace


BAD = [
    dict(size=8), dict(Q=None), dict(O=None), dict(C=None), dict(cu_seqlens_q=None),
    dict(B=0), dict(B=-1), dict(total_q=0), dict(max_q=0), dict(max_q=-2),
    dict(Hq=0), dict(Hq=129), dict(Hq=-4),
    dict(in_dtype=2), dict(in_dtype=-1), dict(out_dtype=2), dict(out_dtype=-1),
    dict(causal=2), dict(causal=-1),
    dict(num_splits=-1), dict(num_splits=5),                       # ceil(256 / 64) = 4 is the most
    dict(Q=4096 + 8), dict(O=8192 + 4), dict(C=24),                # 16-byte alignment
    dict(cu_seqlens_q=18), dict(seqlens_k=18), dict(lse=4098),     # 4-byte vectors
    dict(q_stride_t=575), dict(q_stride_t=16 * 576 + 4), dict(q_stride_h=580), dict(q_stride_h=-8),
    dict(o_stride_t=504), dict(o_stride_t=16 * 512 + 2), dict(o_stride_h=513), dict(o_stride_h=-8),
    dict(q_stride_t=1 << 31),                                      # two tokens of a sequence: beyond 32-bit byte offsets
    dict(o_stride_h=1 << 28, o_stride_t=1 << 33),                  # 16 heads of fp32
]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_rejected_before_the_device(fa, bad):
    for paged in (False, True):
        assert _call(fa, paged, **bad) == INVALID
        assert _call(fa, paged, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID   # not for want of a workspace
        assert _bytes(fa, paged, **bad) == 0


def test_null_descriptor(fa):
    L = fa.lib()
    assert L.fa_mla_decode(None) == INVALID and L.fa_mla_decode_workspace_bytes(None) == 0 and L.fa_mla_append(None) == INVALID


@pytest.mark.parametrize("bad", [dict(Ncap=0), dict(Ncap=-5), dict(Ncap=(1 << 30) + 1)], ids=str)
def test_bad_capacity(fa, bad):
    assert _call(fa, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID and _bytes(fa, **bad) == 0


@pytest.mark.parametrize("bad", [dict(num_pages=0), dict(max_pages=0), dict(page_size=8), dict(page_size=24), dict(page_size=0),
                                 dict(max_pages=1 << 27), dict(block_table=18)], ids=str)
def test_bad_page_geometry(fa, bad):
    assert _call(fa, True, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID and _bytes(fa, True, **bad) == 0


def test_workspace_follows_the_host_integers(fa):
    """monotone in num_splits, the same for a paged cache of the same capacity, independent of everything that lives on the device"""
    sizes = [_bytes(fa, num_splits=s) for s in (1, 2, 3, 4)]
    assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] == 2 * sizes[1] and 2 * sizes[2] == 3 * sizes[1]                   # proportional to the split count
    assert [_bytes(fa, True, num_splits=s) for s in (1, 2, 3, 4)] == sizes             # 16 pages of 16 = 256 keys
    assert _bytes(fa, seqlens_k=64, lse=4096, scale=0.0, causal=0, out_dtype=1, in_dtype=1) == sizes[1]
    # rows: max_q * Hq folded into row blocks -- more heads or more rows never need less
    assert _bytes(fa, Hq=128) >= _bytes(fa, Hq=16) and _bytes(fa, max_q=8, total_q=16) >= _bytes(fa, max_q=2)
    assert _bytes(fa, B=4) == 2 * sizes[1]
    # the automatic choice: a host rule on (B, Hq, max_q, capacity) -- one pass for a short cache, splits for a long one and few rows
    assert _bytes(fa, num_splits=0) == 0
    auto = _bytes(fa, num_splits=0, Ncap=32768, B=1, Hq=16, max_q=1, total_q=1)
    assert auto > 0 and auto % (_bytes(fa, num_splits=2, Ncap=32768, B=1, Hq=16, max_q=1, total_q=1) // 2) == 0


# ---- fa_mla_append ---------------------------------------------------------------------------------------------------------------------
def _adesc(fa, paged=False, **kw):
    f = dict(Cnew=4096, C=8192, cu_seqlens_new=16, seqlens_k=64, seqlens_out=64, B=2, total_new=4, new_stride_t=576, dtype=0)
    if paged:
        f.update(block_table=128, num_pages=8, page_size=16, max_pages=16)
    else:
        f.update(Ncap=256)
    f.update(kw)
    return fa.capi.MlaAppendDesc(**f)


ABAD = [
    dict(size=8), dict(Cnew=None), dict(C=None), dict(cu_seqlens_new=None), dict(B=0), dict(total_new=0), dict(total_new=(1 << 24) + 1),
    dict(dtype=2), dict(dtype=-1), dict(Cnew=4100), dict(C=8200), dict(new_stride_t=568), dict(new_stride_t=580),
    dict(cu_seqlens_new=18), dict(seqlens_k=66, seqlens_out=66),
    dict(seqlens_out=68),                    # a partial overlap with seqlens_k (B = 2: 8 bytes each)
    dict(seqlens_out=16), dict(seqlens_out=24),   # overlaps cu_seqlens_new (12 bytes)
]


@pytest.mark.parametrize("bad", ABAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_append_rejected_before_the_device(fa, bad):
    for paged in (False, True):
        assert fa.lib().fa_mla_append(ctypes.byref(_adesc(fa, paged, **bad))) == INVALID


def test_append_bad_geometry(fa):
    L = fa.lib()
    for bad in (dict(Ncap=0), dict(Ncap=(1 << 30) + 1)):
        assert L.fa_mla_append(ctypes.byref(_adesc(fa, **bad))) == INVALID
    for bad in (dict(num_pages=0), dict(max_pages=0), dict(page_size=8), dict(page_size=48), dict(max_pages=1 << 27)):
        assert L.fa_mla_append(ctypes.byref(_adesc(fa, True, **bad))) == INVALID
