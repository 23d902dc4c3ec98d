"""CPU tier of the fp8 KV-cache decode entries (fa_forward_kvcache_fp8, fa_forward_kvcache_paged_fp8): the symbols are exported and
bound, what the 16-bit entries reject is rejected here too before the device is touched, the Python front ends refuse what they
must, the custom ops register, and quantize_kv_fp8 keeps its promises.  Only calls that must be rejected are issued, so the file
is safe where a GPU is visible."""
import ctypes

import numpy as np
import pytest

import fp8_inputs as f8

INVALID = 1  # hipErrorInvalidValue
NAMES = ("fa_forward_kvcache_fp8", "fa_forward_kvcache_paged_fp8")


def test_fp8_symbols_exported(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    for n in NAMES:
        assert n in fa.capi.SYMBOLS, n
        assert hasattr(raw, n), n
        assert getattr(fa.lib(), n).restype is ctypes.c_int
        assert n in fa.__all__
    assert "quantize_kv_fp8" in fa.__all__
    # the workspace is the 16-bit entries': no size function of their own
    assert not hasattr(raw, "fa_forward_kvcache_fp8_workspace_bytes") and not hasattr(raw, "fa_forward_kvcache_paged_fp8_workspace_bytes")
    assert len(fa.lib().fa_forward_kvcache_fp8.argtypes) == len(fa.lib().fa_forward_kvcache.argtypes) + 2
    assert len(fa.lib().fa_forward_kvcache_paged_fp8.argtypes) == len(fa.lib().fa_forward_kvcache_paged.argtypes) + 2


def _contig(fa, q=16, k=16, v=16, o=16, lse=None, lens=None, ks=None, vs=None, B=1, Hkv=1, G=1, Nq=1, Ncap=200, d=64, scale=0.125,
            causal=0, in_dt=0, out_dt=0, ws=None, ws_bytes=0):
    """One call with small made-up addresses: every case below must be turned away before anything dereferences them."""
    vp = ctypes.c_void_p
    return fa.lib().fa_forward_kvcache_fp8(vp(q), vp(k), vp(v), vp(o), lse, lens, ks, vs, B, Hkv, G, Nq, Ncap, d, scale, causal,
                                           in_dt, out_dt, ws, ws_bytes, None)


def _paged(fa, q=16, k=16, v=16, o=16, lse=None, lens=None, table=16, ks=None, vs=None, B=1, Hkv=1, G=1, Nq=1, num_pages=8,
           page_size=16, max_pages=12, d=64, scale=0.125, causal=0, in_dt=0, out_dt=0, ws=None, ws_bytes=0):
    vp = ctypes.c_void_p
    return fa.lib().fa_forward_kvcache_paged_fp8(vp(q), vp(k), vp(v), vp(o), lse, lens, vp(table), ks, vs, B, Hkv, G, Nq, num_pages,
                                                 page_size, max_pages, d, scale, causal, in_dt, out_dt, ws, ws_bytes, None)


SCALES = dict(ks=ctypes.c_void_p(16), vs=ctypes.c_void_p(16))   # scale pointers present: still rejected first


# the cases of tests/test_kvcache_host.py
@pytest.mark.parametrize("bad", [
    dict(q=0), dict(k=0), dict(v=0), dict(o=0),                                     # null Q, K, V, O
    dict(q=0, **SCALES), dict(d=96, **SCALES),
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(G=0), dict(G=-2), dict(Nq=0), dict(Ncap=0), dict(Ncap=-5),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0),                                 # d in {64, 128}
    dict(causal=2), dict(causal=-1),
    dict(in_dt=2), dict(in_dt=-1), dict(out_dt=2), dict(out_dt=7),
    dict(Ncap=8192),                                                                # split: NULL workspace
    dict(Ncap=8192, ws=ctypes.c_void_p(16), ws_bytes=8),                            # split: short workspace
    dict(Ncap=8192, ws=None, ws_bytes=1 << 30),                                     # split: NULL workspace with a size
    dict(Ncap=1 << 25, d=128, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),            # the 16-bit entries' bound on the capacity
    dict(Ncap=1 << 26, d=64, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),
    dict(G=1 << 12, Nq=1 << 12, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),          # G*Nq rows of (d+2)*4 bytes: 32-bit offsets
    dict(G=1 << 16, Nq=1 << 16), dict(B=1 << 16, Hkv=1 << 16),                      # products beyond int
])
def test_fp8_rejects_without_device(fa, bad):
    assert _contig(fa, **bad) == INVALID, bad


# the cases of tests/test_kvcache_paged_host.py
@pytest.mark.parametrize("bad", [
    dict(page_size=0), dict(page_size=8), dict(page_size=24), dict(page_size=48), dict(page_size=-16),   # a power of two >= 16
    dict(page_size=8, **SCALES), dict(page_size=24, **SCALES),
    dict(k=0), dict(v=0), dict(table=0), dict(q=0), dict(o=0),                          # null pool, table, Q, O
    dict(num_pages=0), dict(num_pages=-3), dict(max_pages=0), dict(max_pages=-1),
    dict(max_pages=1 << 27, page_size=16), dict(max_pages=1 << 20, page_size=1 << 12),    # max_pages * page_size beyond int
    dict(max_pages=1 << 16, page_size=1 << 15),                                          # 2^31 exactly
    dict(max_pages=512, page_size=16),                                                   # split (8192 keys): NULL workspace
    dict(max_pages=512, page_size=16, ws=ctypes.c_void_p(16), ws_bytes=8),               # split: short workspace
    dict(max_pages=32, page_size=256, ws=None, ws_bytes=1 << 30),                        # split: NULL workspace with a size
    dict(max_pages=1 << 21, page_size=16, d=128, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),   # the 16-bit entries' bound
    dict(max_pages=1 << 18, page_size=256, d=64, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),
    dict(max_pages=1, page_size=1 << 26, d=64, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(G=0), dict(G=-2), dict(Nq=0),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0),                                      # d in {64, 128}
    dict(causal=2), dict(causal=-1),
    dict(in_dt=2), dict(in_dt=-1), dict(out_dt=2), dict(out_dt=7),
    dict(G=1 << 12, Nq=1 << 12, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),
    dict(G=1 << 16, Nq=1 << 16), dict(B=1 << 16, Hkv=1 << 16),
])
def test_paged_fp8_rejects_without_device(fa, bad):
    assert _paged(fa, **bad) == INVALID, bad


def test_fp8_ops_refuse_what_they_must(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    k8 = torch.zeros(2, 2, 200, 64, dtype=torch.float8_e4m3fn)
    pool8 = torch.zeros(10, 2, 16, 64, dtype=torch.float8_e4m3fn)
    table = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_kvcache_fp8(q, k8, k8)                                   # CPU tensors
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged_fp8(q, pool8, pool8, table)
    # the cache format is judged before anything that needs a device: other 8-bit formats and 16-bit caches name the one accepted
    for dt in (torch.float16, torch.bfloat16, torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
        with pytest.raises(ValueError, match="OCP e4m3fn"):
            fa.fa_forward_kvcache_fp8(q, k8.view(torch.uint8).to(dt), k8.view(torch.uint8).to(dt))
        with pytest.raises(ValueError, match="OCP e4m3fn"):
            fa.fa_forward_kvcache_fp8(q, k8, k8.view(torch.uint8).to(dt))
        with pytest.raises(ValueError, match="OCP e4m3fn"):
            fa.fa_forward_kvcache_paged_fp8(q, pool8.view(torch.uint8).to(dt), pool8.view(torch.uint8).to(dt), table)
    # scales: float32 [Hkv]
    for bad in (torch.ones(2, dtype=torch.float16), torch.ones(2, dtype=torch.float64), torch.ones(4), torch.ones(1),
                torch.ones(2, 1), torch.tensor(1.0), [1.0, 1.0], 1.0):
        for kw in (dict(k_scale=bad), dict(v_scale=bad)):
            with pytest.raises(ValueError, match="_scale"):
                fa.fa_forward_kvcache_fp8(q, k8, k8, **kw)
            with pytest.raises(ValueError, match="block_table|_scale"):
                fa.fa_forward_kvcache_paged_fp8(q, pool8, pool8, table, **kw)
    with pytest.raises(ValueError, match="k_scale"):
        fa.fa_forward_kvcache_fp8(q, k8, k8, k_scale=torch.ones(2))            # right type and shape, but not on the device
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_fp8(q, k8, k8[:, :1])                            # k_cache and v_cache differ in shape
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_fp8(torch.zeros(2, 3, 1, 64, dtype=torch.float16), k8, k8)   # Hq not a multiple of Hkv
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_fp8(q.float(), k8, k8)                           # q is fp16 or bf16
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_fp8(q, k8, k8, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block_table"):
        fa.fa_forward_kvcache_paged_fp8(q, pool8, pool8, torch.zeros(2, 5, dtype=torch.int64))
    # the 16-bit front ends still refuse an fp8 cache (their own tests assert the rest)
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache(q, k8, k8)
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged(q, pool8, pool8, table)


def test_decode_fp8_custom_ops_register(fa):
    """torch.ops.fa_mi355.decode_fp8 and .decode_paged_fp8 exist after register(), trace on meta tensors, and have no CPU kernel."""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    register()
    q = torch.empty(2, 8, 3, 128, dtype=torch.bfloat16, device="meta")
    k8 = torch.empty(2, 2, 500, 128, dtype=torch.float8_e4m3fn, device="meta")
    pool8 = torch.empty(40, 2, 32, 128, dtype=torch.float8_e4m3fn, device="meta")
    table = torch.empty(2, 16, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    sc = torch.empty(2, dtype=torch.float32, device="meta")
    o = torch.ops.fa_mi355.decode_fp8(q, k8, k8, sc, sc, lens, 0.125, True, True)
    assert o.shape == q.shape and o.dtype == torch.float32
    o = torch.ops.fa_mi355.decode_fp8(q, k8, k8, None, None, None, 0.125, False, False)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    o = torch.ops.fa_mi355.decode_paged_fp8(q, pool8, pool8, table, sc, sc, lens, 0.125, True, True)
    assert o.shape == q.shape and o.dtype == torch.float32
    o = torch.ops.fa_mi355.decode_paged_fp8(q, pool8, pool8, table, None, None, None, 0.125, False, False)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    c = torch.zeros(1, 1, 16, 64, dtype=torch.float16)
    c8 = torch.zeros(1, 1, 16, 64, dtype=torch.float8_e4m3fn)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        torch.ops.fa_mi355.decode_fp8(c, c8, c8, None, None, None, 0.125, False, True)
    with pytest.raises(Exception):
        torch.ops.fa_mi355.decode_paged_fp8(c, c8, c8, torch.zeros(1, 1, dtype=torch.int32), None, None, None, 0.125, False, True)


def test_quantize_kv_fp8(fa):
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, 50, 64, generator=g)
    x[:, 1] *= 37.0          # heads of different magnitude get scales of their own
    x[:, 2] = 0.0            # an all-zero head
    x[0, 3, 7, 5] = -9.0     # head 3's largest magnitude is negative
    for src in (x, x.half(), x.bfloat16()):
        x8, scale = fa.quantize_kv_fp8(src)
        assert x8.dtype == torch.float8_e4m3fn and x8.shape == x.shape
        assert scale.dtype == torch.float32 and scale.shape == (4,) and scale.is_contiguous()
        xf = src.float()
        amax = xf.abs().amax(dim=(0, 2, 3))
        want = torch.where(amax > 0, amax / 448.0, torch.ones(4))
        assert torch.equal(scale, want) and scale[2] == 1.0 and torch.isfinite(scale).all() and (scale > 0).all()
        codes = x8.view(torch.uint8).numpy()
        assert not np.isin(codes, f8.NAN_CODES).any()                          # no NaN, the zero head included
        deq = f8.decode(codes)                                                 # the table of the format, not torch's conversion
        assert (deq[:, 2] == 0.0).all()
        for h in range(4):
            if h != 2:                                                         # amax maps to +-448
                assert np.abs(deq[:, h]).max() == 448.0
        i = np.unravel_index(np.abs(xf[:, 3].numpy()).argmax(), (3, 50, 64))
        assert deq[:, 3][i] == -448.0
        # values that are normal in e4m3fn after scaling: half an ulp, 2^-4 relative, plus the rounding of the fp32 quotient
        sc = scale.view(1, 4, 1, 1).numpy()
        scaled = xf.numpy() / sc
        normal = np.abs(scaled) >= f8.MIN_NORMAL
        rel = np.abs(deq * sc - xf.numpy())[normal] / np.abs(xf.numpy())[normal]
        print(f"{src.dtype}: largest relative error of a normal value {rel.max():.4f} (bound {f8.REL_EPS})")
        assert normal.sum() > 0.7 * normal.size and rel.max() <= f8.REL_EPS * (1 + 2.0 ** -20)
        assert np.abs(deq * sc - xf.numpy())[~normal].max() <= f8.MIN_SUBNORMAL / 2 * sc.max()   # subnormals: half a step, absolute
        assert np.array_equal(codes, f8.encode(scaled))                        # and it is round-to-nearest-even throughout
    # a value that torch's own conversion would turn into NaN (it does not saturate) is clamped to 448
    big, s1 = fa.quantize_kv_fp8(torch.full((1, 1, 1, 64), 3.0), scale=torch.tensor([3.0 / 500.0]))
    assert (big.view(torch.uint8) == 0x7E).all() and s1.item() == pytest.approx(0.006)
    # given scales are used as they are; a pool layout [num_pages, Hkv, page, d] works the same way
    pool = torch.randn(7, 2, 16, 128, generator=g)
    given = torch.tensor([0.05, 0.3])
    p8, s = fa.quantize_kv_fp8(pool, scale=given)
    assert torch.equal(s, given) and np.array_equal(p8.view(torch.uint8).numpy(), f8.encode(pool.numpy() / given.view(1, 2, 1, 1).numpy()))
    with pytest.raises(ValueError):
        fa.quantize_kv_fp8(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError):
        fa.quantize_kv_fp8(pool, scale=torch.ones(3))
