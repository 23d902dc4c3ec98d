"""CPU tier of fa_kvcache_decode_d256_fp8 and fa_kvcache_append_varlen_d256, through the C ABI with a null stream: every refusal
holds before the device is touched, and the fp8 sizing function equals the 16-bit entry's on the twin descriptor.  Only calls that
must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue


def _decode(fa, **kw):
    """test_kv256_host's descriptor on an e4m3fn cache: it WOULD be launched"""
    f = dict(Q=4096, O=8192, K=16, V=16, cu_seqlens_q=16, B=2, Hkv=2, G=4, d=256, total_q=6, max_q=2, q_stride_t=2048, q_stride_h=256,
             o_stride_t=2048, o_stride_h=256, scale=0.0625, causal=1, in_dtype=0, out_dtype=0, kv_dtype=1, k_scale=64, v_scale=128)
    f.update(dict(block_table=16, num_pages=8, page_size=16, max_pages=64) if kw.pop("paged", False) else dict(Ncap=1024))
    f.update(kw)
    return fa.capi.KvDecodeVarlenDesc(**f)


def _append(fa, **kw):
    """a rotary fp8 append at d = 256 that WOULD be launched (paged: the pool form)"""
    f = dict(Knew=4096, Vnew=8192, K=16, V=16, cu_seqlens_new=16, B=1, Hkv=1, d=256, total_new=4, dtype=0, k_stride_t=256, k_stride_h=256,
             v_stride_t=256, v_stride_h=256, kv_dtype=1, k_scale=64, Q=1 << 20, Qout=1 << 20, rope_cos=16, rope_sin=16, G=1, rot_dim=256,
             max_pos=8, q_stride_t=256, q_stride_h=256, qo_stride_t=256, qo_stride_h=256)
    f.update(dict(block_table=16, num_pages=8, page_size=16, max_pages=12) if kw.pop("paged", False) else dict(Ncap=192))
    f.update(kw)
    return fa.capi.KvAppendVarlenDesc(**f)


BAD_DECODE = [dict(d=128), dict(d=512), dict(kv_dtype=0), dict(kv_dtype=2), dict(sinks=16), dict(k_scale=66), dict(v_scale=129),
              dict(size=8), dict(K=0), dict(Ncap=1 << 23), dict(window=-1), dict(softcap=float("nan")), dict(q_stride_t=2052),
              dict(paged=True, page_size=8), dict(paged=True, max_pages=1 << 20)]
BAD_APPEND = [dict(d=128), dict(d=64, rot_dim=64), dict(d=512), dict(kv_dtype=2), dict(kv_dtype=0), dict(size=8), dict(Knew=0),
              dict(cu_seqlens_new=0), dict(total_new=0), dict(Ncap=1 << 23), dict(Knew=4096 + 8), dict(k_stride_t=128), dict(v_stride_t=260),
              dict(k_stride_h=-256), dict(rot_dim=264), dict(rot_dim=8), dict(rot_dim=272), dict(max_pos=0), dict(interleaved=2), dict(G=0),
              dict(Qout=0), dict(Qout=(1 << 20) + 512), dict(qo_stride_t=512), dict(rope_cos=0), dict(rope_sin=0),
              dict(seqlens_out=16), dict(paged=True, page_size=8), dict(paged=True, num_pages=0), dict(paged=True, max_pages=1 << 20)]
ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())   # noqa: E731


@pytest.mark.parametrize("bad", BAD_DECODE, ids=ids)
def test_decode_refused_before_the_device(fa, bad):
    L = fa.lib()
    for S in (0, 1):
        assert L.fa_kvcache_decode_d256_fp8(ctypes.byref(_decode(fa, **bad)), S) == INVALID
    assert L.fa_kvcache_decode_d256_fp8_workspace_bytes(ctypes.byref(_decode(fa, **bad)), 4) == 0


@pytest.mark.parametrize("bad", BAD_APPEND, ids=ids)
def test_append_refused_before_the_device(fa, bad):
    opts = fa.capi.new_desc(fa.capi.KvAppendVarlenOpts)
    assert fa.lib().fa_kvcache_append_varlen_d256(ctypes.byref(_append(fa, **bad)), None) == INVALID
    assert fa.lib().fa_kvcache_append_varlen_d256(ctypes.byref(_append(fa, **bad)), ctypes.byref(opts)) == INVALID


def test_append_options_and_the_other_entries(fa):
    L = fa.lib()
    assert L.fa_kvcache_append_varlen_d256(None, None) == INVALID
    opts = fa.capi.KvAppendVarlenOpts(positions=16)
    opts.size = 8
    assert L.fa_kvcache_append_varlen_d256(ctypes.byref(_append(fa)), ctypes.byref(opts)) == INVALID   # a wrong size
    opts = fa.capi.new_desc(fa.capi.KvAppendVarlenOpts)
    opts.positions = 18
    assert L.fa_kvcache_append_varlen_d256(ctypes.byref(_append(fa)), ctypes.byref(opts)) == INVALID   # misaligned
    opts.positions = 16
    plain = _append(fa, Q=0, Qout=0, rope_cos=0, rope_sin=0, G=0, rot_dim=0, max_pos=0)
    assert L.fa_kvcache_append_varlen_d256(ctypes.byref(plain), ctypes.byref(opts)) == INVALID           # positions without rotary
    assert L.fa_kvcache_append_varlen_d256(ctypes.byref(_append(fa, kv_dtype=0)), None) == INVALID       # scales on a 16-bit cache
    # the d <= 128 entries keep refusing the descriptor, and the 16-bit decode an fp8 one
    assert L.fa_kvcache_append_varlen(ctypes.byref(plain)) == INVALID and L.fa_kvcache_append_varlen_ex(ctypes.byref(_append(fa)), None) == INVALID
    assert L.fa_kvcache_decode_d256(ctypes.byref(_decode(fa)), 1) == INVALID
    assert L.fa_kvcache_decode_varlen(ctypes.byref(_decode(fa))) == INVALID


def test_workspace_is_the_16_bit_entrys(fa):
    L = fa.lib()
    assert L.fa_kvcache_decode_d256_fp8(None, 0) == INVALID and L.fa_kvcache_decode_d256_fp8_workspace_bytes(None, 0) == 0
    twin = dict(kv_dtype=0, k_scale=0, v_scale=0)
    for kw in (dict(), dict(paged=True), dict(G=8, max_q=5), dict(Ncap=1 << 15), dict(Ncap=1 << 15, window=70, max_q=5), dict(k_scale=0)):
        for S in range(0, 18):
            got = L.fa_kvcache_decode_d256_fp8_workspace_bytes(ctypes.byref(_decode(fa, **kw)), S)
            assert got == L.fa_kvcache_decode_d256_workspace_bytes(ctypes.byref(_decode(fa, **{**kw, **twin})), S), (kw, S)
            tiles = kw.get("Ncap", 1024) // 64   # 0 for one split, above the tile count, and where the window's span is one split
            assert (got == 0) == (S == 1 or S > tiles or (S == 0 and "window" in kw)), (kw, S)
    for paged in (False, True):   # a split needs a workspace: missing, too small, misaligned
        need = L.fa_kvcache_decode_d256_fp8_workspace_bytes(ctypes.byref(_decode(fa, paged=paged)), 4)
        for ws in (dict(), dict(workspace=4096, workspace_bytes=need - 1), dict(workspace=4096 + 8, workspace_bytes=need)):
            assert need and L.fa_kvcache_decode_d256_fp8(ctypes.byref(_decode(fa, paged=paged, **ws)), 4) == INVALID
        assert L.fa_kvcache_decode_d256_fp8(ctypes.byref(_decode(fa, paged=paged)), 17) == INVALID
        assert L.fa_kvcache_decode_d256_fp8(ctypes.byref(_decode(fa, paged=paged)), -1) == INVALID
    assert fa.kvcache_decode_d256_fp8_workspace_bytes(2, 2, 4, 2, Ncap=1024, num_splits=4) == \
        fa.kvcache_decode_d256_workspace_bytes(2, 2, 4, 2, Ncap=1024, num_splits=4) > 0
