"""CPU tier of the KV-cache decode entry (fa_forward_kvcache): the symbols are exported and bound, bad arguments are
rejected before the device is touched, the workspace size follows the capacity, and the Python front ends refuse what
they must.  Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
NAMES = ("fa_forward_kvcache_workspace_bytes", "fa_forward_kvcache")


def test_kvcache_symbols_exported(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    for n in NAMES:
        assert n in fa.capi.SYMBOLS, n
        assert hasattr(raw, n), n
    assert fa.lib().fa_forward_kvcache.restype is ctypes.c_int
    assert fa.lib().fa_forward_kvcache_workspace_bytes.restype is ctypes.c_size_t
    assert "fa_forward_kvcache" in fa.__all__ and "kvcache_workspace_bytes" in fa.__all__


def _call(fa, q=16, k=16, v=16, o=16, lse=None, lens=None, B=1, Hkv=1, G=1, Nq=1, Ncap=200, d=64, scale=0.125, causal=0,
          in_dt=0, out_dt=0, ws=None, ws_bytes=0):
    """One call with small made-up addresses: every case below must be turned away before anything dereferences them."""
    vp = ctypes.c_void_p
    return fa.lib().fa_forward_kvcache(vp(q), vp(k), vp(v), vp(o), lse, lens, B, Hkv, G, Nq, Ncap, d, scale, causal, in_dt,
                                       out_dt, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [
    dict(q=0), dict(k=0), dict(v=0), dict(o=0),                                     # null Q, K, V, O
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(G=0), dict(G=-2), dict(Nq=0), dict(Ncap=0), dict(Ncap=-5),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0),                                 # d in {64, 128}
    dict(causal=2), dict(causal=-1),
    dict(in_dt=2), dict(in_dt=-1), dict(out_dt=2), dict(out_dt=7),
    dict(Ncap=8192),                                                                # split: NULL workspace
    dict(Ncap=8192, ws=ctypes.c_void_p(16), ws_bytes=8),                            # split: short workspace
    dict(Ncap=8192, ws=None, ws_bytes=1 << 30),                                     # split: NULL workspace with a size
    dict(Ncap=1 << 25, d=128, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),            # K/V head of 2^33 bytes: 32-bit offsets
    dict(Ncap=1 << 26, d=64, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),
    dict(G=1 << 12, Nq=1 << 12, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),          # G*Nq rows of (d+2)*4 bytes: 32-bit offsets
    dict(G=1 << 16, Nq=1 << 16), dict(B=1 << 16, Hkv=1 << 16),                      # products beyond int
])
def test_kvcache_rejects_without_device(fa, bad):
    assert _call(fa, **bad) == INVALID, bad


def test_kvcache_workspace_bytes(fa):
    L = fa.lib()
    assert L.fa_forward_kvcache_workspace_bytes(1, 1, 1, 1, 8192, 64) > 0
    assert L.fa_forward_kvcache_workspace_bytes(8, 16, 1, 4096, 4096, 64) == 0   # enough workgroups already
    # the layout of fa_forward_splitkv's workspace, for G*Nq rows and Ncap keys
    assert L.fa_forward_kvcache_workspace_bytes(2, 2, 4, 1, 8229, 128) == L.fa_forward_splitkv_workspace_bytes(2, 2, 4, 8229, 128)
    assert fa.kvcache_workspace_bytes(2, 2, 4, 1, 8229, 128) == L.fa_forward_splitkv_workspace_bytes(2, 2, 4, 8229, 128)
    for bad in ((0, 1, 1, 1, 8192, 64), (1, 0, 1, 1, 8192, 64), (1, 1, 0, 1, 8192, 64), (1, 1, 1, 0, 8192, 64),
                (1, 1, 1, 1, 0, 64), (1, 1, 1, 1, 8192, 32)):
        assert L.fa_forward_kvcache_workspace_bytes(*bad) == 0, bad


def test_kvcache_op_refuses_cpu_tensors_and_bad_lengths(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache(q, k, k)
    # cache_seqlens is judged first, so these are refused for what is wrong with IT (q, k being CPU tensors is not reached)
    for bad in (torch.zeros(2, dtype=torch.int32),                                      # int32 [B], but not on the device
                torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.float32), torch.zeros(3, dtype=torch.int32),
                torch.zeros(2, 1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)[::2], [5, 7]):
        with pytest.raises(ValueError, match="cache_seqlens"):
            fa.fa_forward_kvcache(q, k, k, cache_seqlens=bad)
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache(q, k, k[:, :1])                                  # k_cache and v_cache differ in shape
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache(torch.zeros(2, 3, 1, 64, dtype=torch.float16), k, k)   # Hq not a multiple of Hkv
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache(q, k, k, out_dtype=torch.bfloat16)


def test_decode_custom_op_registers(fa):
    """torch.ops.fa_mi355.decode exists after register(), traces on meta tensors, and has no CPU kernel."""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    register()
    q = torch.empty(2, 8, 3, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(2, 2, 500, 128, dtype=torch.bfloat16, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    o = torch.ops.fa_mi355.decode(q, k, k, lens, 0.125, True, True)
    assert o.shape == q.shape and o.dtype == torch.float32
    o = torch.ops.fa_mi355.decode(q, k, k, None, 0.125, False, False)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        c = torch.zeros(1, 1, 1, 64, dtype=torch.float16)
        torch.ops.fa_mi355.decode(c, c, c, None, 0.125, False, True)
