"""CPU tier of fa_kvcache_decode_d256, through the C ABI with a null stream: every refusal holds before the device is touched, the
sizing function is 0 for one split and for a refused descriptor and grows with the split count, and the entries for d in {64,128}
still refuse d = 256.  Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
ROW = 32 * (256 + 4) * 4   # one 32-row block of workspace rows: O^T, m, l and two floats of padding


def _desc(fa, paged=False, **kw):
    """a descriptor with small made-up addresses that WOULD be launched: two tokens per sequence, 1024 keys"""
    f = dict(Q=4096, O=8192, K=16, V=16, cu_seqlens_q=16, B=2, Hkv=2, G=4, d=256, total_q=6, max_q=2, q_stride_t=2048, q_stride_h=256,
             o_stride_t=2048, o_stride_h=256, scale=0.0625, causal=1, window=0, softcap=0.0, in_dtype=0, out_dtype=0)
    f.update(dict(block_table=16, num_pages=8, page_size=16, max_pages=64) if paged else dict(Ncap=1024))
    f.update(kw)
    return fa.capi.KvDecodeVarlenDesc(**f)


def _call(fa, S=0, **kw):
    return fa.lib().fa_kvcache_decode_d256(ctypes.byref(_desc(fa, **kw)), S)


def _bytes(fa, S=0, **kw):
    return fa.lib().fa_kvcache_decode_d256_workspace_bytes(ctypes.byref(_desc(fa, **kw)), S)


# one bad field (or pair) at a time; `paged` picks the form the field belongs to
BAD = [
    dict(size=8), dict(d=64), dict(d=128), dict(d=512), dict(kv_dtype=1), dict(kv_dtype=-1), dict(k_scale=16), dict(v_scale=16), dict(sinks=16),
    dict(Q=0), dict(O=0), dict(K=0), dict(V=0), dict(cu_seqlens_q=0), dict(B=0), dict(Hkv=0), dict(G=-1), dict(total_q=0), dict(max_q=0),
    dict(causal=2), dict(in_dtype=2), dict(out_dtype=3), dict(window=-1), dict(softcap=-1.0), dict(softcap=float("nan")),
    dict(softcap=float("inf")), dict(Ncap=0), dict(Ncap=1 << 23), dict(B=1 << 16, Hkv=1 << 16), dict(G=1 << 16, max_q=1 << 16),
    dict(Q=4096 + 8), dict(O=8192 + 2), dict(q_stride_t=128), dict(o_stride_t=255), dict(q_stride_t=2052), dict(q_stride_h=-256),
    dict(o_stride_h=260), dict(total_q=1 << 22), dict(q_stride_h=1 << 29), dict(o_stride_h=1 << 28),
    dict(paged=True, page_size=8), dict(paged=True, page_size=48), dict(paged=True, num_pages=0), dict(paged=True, max_pages=0),
    dict(paged=True, max_pages=1 << 28), dict(paged=True, max_pages=1 << 20),
]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_refused_before_the_device(fa, bad):
    assert _call(fa, **bad) == INVALID and _call(fa, 1, **bad) == INVALID
    assert _bytes(fa, 4, **bad) == 0


def test_splits_and_workspace(fa):
    L = fa.lib()
    assert L.fa_kvcache_decode_d256(None, 0) == INVALID and L.fa_kvcache_decode_d256_workspace_bytes(None, 0) == 0
    for paged in (False, True):   # 1024 keys = 16 tiles; B * Hkv = 4 heads of one 32-row block
        assert _bytes(fa, 1, paged=paged) == 0 and _bytes(fa, 0, paged=paged) == 4 * 4 * ROW   # 16 tiles, four per split
        sizes = [_bytes(fa, S, paged=paged) for S in range(1, 17)]
        assert sizes == [0] + [4 * S * ROW for S in range(2, 17)]   # monotone in S
        for S in (-1, 17, 1 << 20):
            assert _bytes(fa, S, paged=paged) == 0 and _call(fa, S, paged=paged) == INVALID
        # a split needs a workspace: missing, too small, misaligned
        need = _bytes(fa, 4, paged=paged)
        assert _call(fa, 4, paged=paged) == INVALID and _call(fa, 4, paged=paged, workspace=4096, workspace_bytes=need - 1) == INVALID
        assert _call(fa, 4, paged=paged, workspace=4096 + 8, workspace_bytes=need) == INVALID
    # G * max_q = 40 rows are two blocks; the choice follows the window's span (70 + 5 - 1 keys: three tiles, one split), not the capacity
    assert _bytes(fa, 3, G=8, max_q=5) == 4 * 2 * 3 * ROW
    assert _bytes(fa, 0, Ncap=1 << 15) > 0 and _bytes(fa, 0, Ncap=1 << 15, window=70, max_q=5) == 0
    assert fa.kvcache_decode_d256_workspace_bytes(2, 2, 4, 2, Ncap=1024, num_splits=4) == _bytes(fa, 4)
    assert fa.kvcache_decode_d256_workspace_bytes(2, 2, 4, 2, max_pages=64, page_size=16) == _bytes(fa, 0, paged=True)


def test_the_other_entries_still_refuse_256(fa):
    L = fa.lib()
    d = _desc(fa)
    assert L.fa_kvcache_decode_varlen(ctypes.byref(d)) == INVALID and L.fa_kvcache_decode_varlen_workspace_bytes(ctypes.byref(d)) == 0
    assert L.fa_kvcache_attend_varlen(ctypes.byref(d)) == INVALID
    assert L.fa_forward_kvcache_workspace_bytes(2, 2, 4, 2, 1 << 15, 256) == 0
    torch = pytest.importorskip("torch")
    q, k = torch.zeros(6, 8, 256, dtype=torch.float16), torch.zeros(2, 2, 64, 256, dtype=torch.float16)
    cu = torch.tensor([0, 2, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="64 or 128"):
        fa.fa_kvcache_decode_varlen(q, k, k, cu, 2)
    with pytest.raises(ValueError, match="must be 256"):
        fa.fa_kvcache_decode_d256(q[..., :128], k[..., :128], k[..., :128], cu, 2)
    with pytest.raises(ValueError, match="num_splits"):
        fa.fa_kvcache_decode_d256(q, k, k, cu, 2, num_splits=-1)
    with pytest.raises(ValueError, match="device tensor"):   # everything else in order: the HIP path has no CPU fallback
        fa.fa_kvcache_decode_d256(q, k, k, cu, 2)
    from flashattention_kernel_project_amd.torch_op import register
    register()
    m = lambda *s, dt=torch.bfloat16: torch.empty(*s, dtype=dt, device="meta")   # noqa: E731
    o, lse = torch.ops.fa_mi355.decode_d256(m(6, 8, 256), m(2, 2, 64, 256), m(2, 2, 64, 256), m(3, dt=torch.int32), 2, None, None, 0.0625,
                                            True, 0, 30.0, 0, False)
    assert o.shape == (6, 8, 256) and o.dtype == torch.bfloat16 and lse.shape == (8, 6)
