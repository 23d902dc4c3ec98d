"""CPU tier of fa_forward_varlen_d256 and fa_forward_varlen_kvcache_d256, through the C ABI with a null stream: every refusal holds
before the device is touched, and the d in {64,128} entries still refuse d = 256.  Only calls that must be rejected are issued, so the
file is safe where a GPU is visible."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
COMMON = dict(Q=4096, O=8192, K=16, V=16, cu_seqlens_q=16, B=2, Hkv=2, G=4, d=256, total_q=6, q_stride_t=2048, q_stride_h=256,
              o_stride_t=2048, o_stride_h=256, scale=0.0625, causal=1, in_dtype=0, out_dtype=0)


def _packed(fa, opts=None, **kw):
    """a packed call with small made-up addresses that WOULD be launched"""
    f = dict(COMMON, cu_seqlens_k=16, total_k=64, k_stride_t=512, k_stride_h=256, v_stride_t=512, v_stride_h=256)
    f.update(kw)
    o = None if opts is None else ctypes.byref(fa.capi.VarlenOpts(**opts))
    return fa.lib().fa_forward_varlen_d256(ctypes.byref(fa.capi.VarlenDesc(**f)), o)


def _cache_desc(fa, paged=False, **kw):
    f = dict(COMMON, seqlens_k=16, window=0, softcap=0.0)
    f.update(dict(block_table=16, num_pages=8, page_size=16, max_pages=64) if paged else dict(Ncap=1024))
    f.update(kw)
    return fa.capi.VarlenKvcacheDesc(**f)


def _cache(fa, **kw):
    return fa.lib().fa_forward_varlen_kvcache_d256(ctypes.byref(_cache_desc(fa, **kw)))


# one bad field (or pair) at a time: what both descriptors share
BAD_BOTH = [
    dict(size=8), dict(d=64), dict(d=128), dict(d=512), dict(Q=0), dict(O=0), dict(K=0), dict(V=0), dict(cu_seqlens_q=0), dict(B=0),
    dict(Hkv=0), dict(G=-1), dict(total_q=0), dict(in_dtype=2), dict(out_dtype=3), dict(B=1 << 16, Hkv=1 << 16), dict(Q=4096 + 8),
    dict(O=8192 + 2), dict(K=24), dict(V=8), dict(q_stride_t=128), dict(o_stride_t=255), dict(q_stride_t=2052), dict(q_stride_h=-256),
    dict(o_stride_h=260), dict(total_q=1 << 22), dict(q_stride_h=1 << 29),
]
BAD_PACKED = [
    dict(cu_seqlens_k=0), dict(total_k=0), dict(k_stride_t=128), dict(v_stride_t=516), dict(k_stride_h=-8), dict(total_k=1 << 23),
    dict(opts=dict(size=8)), dict(opts=dict(sinks=16)), dict(opts=dict(window=-1)), dict(opts=dict(softcap=-1.0)),
    dict(opts=dict(softcap=float("nan"))), dict(opts=dict(softcap=float("inf"))),
]
BAD_CACHE = [
    dict(seqlens_k=0), dict(sinks=16), dict(window=-1), dict(softcap=-1.0), dict(softcap=float("nan")), dict(softcap=float("inf")),
    dict(Ncap=0), dict(Ncap=(1 << 23) - 64), dict(Ncap=1 << 23), dict(paged=True, page_size=8), dict(paged=True, page_size=48),
    dict(paged=True, num_pages=0), dict(paged=True, max_pages=0), dict(paged=True, max_pages=1 << 28), dict(paged=True, max_pages=1 << 19),
]
ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())   # noqa: E731


@pytest.mark.parametrize("bad", BAD_BOTH + BAD_PACKED, ids=ids)
def test_packed_refused_before_the_device(fa, bad):
    assert _packed(fa, **bad) == INVALID


@pytest.mark.parametrize("bad", BAD_BOTH + BAD_CACHE, ids=ids)
def test_cache_refused_before_the_device(fa, bad):
    assert _cache(fa, **bad) == INVALID
    if "paged" not in bad and "Ncap" not in bad:
        assert _cache(fa, paged=True, **bad) == INVALID


def test_null_descriptors_and_the_capacity_bound(fa):
    L = fa.lib()
    assert L.fa_forward_varlen_d256(None, None) == INVALID and L.fa_forward_varlen_kvcache_d256(None) == INVALID
    # (cap + 64) * 512 < 2^32: the largest capacity the d = 256 decode takes is 2^23 - 65; the d <= 128 rule alone (cap * 512 <= 2^32)
    # would let 2^23 - 64 through
    assert _cache(fa, Ncap=(1 << 23) - 64) == INVALID and _cache(fa, paged=True, max_pages=1 << 19) == INVALID


def test_the_other_entries_still_refuse_256(fa):
    L = fa.lib()
    p = fa.capi.VarlenDesc(**dict(COMMON, cu_seqlens_k=16, total_k=64, k_stride_t=512, k_stride_h=256, v_stride_t=512, v_stride_h=256))
    assert L.fa_forward_varlen(ctypes.byref(p)) == INVALID
    assert L.fa_forward_varlen_ex(ctypes.byref(p), ctypes.byref(fa.capi.VarlenOpts(window=5))) == INVALID
    for paged in (False, True):
        c = _cache_desc(fa, paged=paged)
        assert L.fa_forward_varlen_kvcache(ctypes.byref(c)) == INVALID
        assert L.fa_forward_varlen_kvcache_fp8(ctypes.byref(c), None, None) == INVALID
    torch = pytest.importorskip("torch")
    q, k, c = (torch.zeros(*s, dtype=torch.float16) for s in ((6, 8, 256), (9, 2, 256), (2, 2, 64, 256)))
    cu, lens = torch.tensor([0, 2, 4], dtype=torch.int32), torch.tensor([9, 9], dtype=torch.int32)
    with pytest.raises(ValueError, match="64 or 128"):
        fa.fa_forward_varlen(q, k, k, cu)
    with pytest.raises(ValueError, match="64 or 128"):
        fa.fa_forward_varlen_kvcache(q, c, c, cu, lens)
    with pytest.raises(ValueError, match="must be 256"):
        fa.fa_forward_varlen_d256(q[..., :128], k[..., :128], k[..., :128], cu)
    with pytest.raises(ValueError, match="must be 256"):
        fa.fa_forward_varlen_kvcache_d256(q[..., :64], c[..., :64], c[..., :64], cu, lens)
    with pytest.raises(ValueError, match="device tensor"):   # everything else in order: the HIP path has no CPU fallback
        fa.fa_forward_varlen_d256(q, k, k, cu)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_varlen_kvcache_d256(q, c, c, cu, lens)
    from flashattention_kernel_project_amd.torch_op import register
    register()
    m = lambda *s, dt=torch.bfloat16: torch.empty(*s, dtype=dt, device="meta")   # noqa: E731
    o, lse = torch.ops.fa_mi355.forward_varlen_d256(m(6, 8, 256), m(9, 2, 256), m(9, 2, 256), m(3, dt=torch.int32), None, 0.0625, True, 17,
                                                    30.0, False)
    assert o.shape == (6, 8, 256) and o.dtype == torch.bfloat16 and lse.shape == (8, 6)
    o, lse = torch.ops.fa_mi355.forward_varlen_kvcache_d256(m(6, 8, 256), m(2, 2, 64, 256), m(2, 2, 64, 256), m(3, dt=torch.int32),
                                                            m(2, dt=torch.int32), None, 0.0625, True, 0, 0.0, True)
    assert o.shape == (6, 8, 256) and o.dtype == torch.float32 and lse.shape == (8, 6)
