"""CPU tier of the paged KV-cache decode entry (fa_forward_kvcache_paged): the symbols are exported and bound, bad arguments are
rejected before the device is touched, the workspace size is the contiguous entry's for the same capacity, and the Python front
ends refuse what they must.  Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
NAMES = ("fa_forward_kvcache_paged_workspace_bytes", "fa_forward_kvcache_paged")


def test_paged_symbols_exported(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    for n in NAMES:
        assert n in fa.capi.SYMBOLS, n
        assert hasattr(raw, n), n
    assert fa.capi.SYMBOLS[-2:] == NAMES   # appended: the slice of int-returning launchers at the head keeps its meaning
    assert fa.lib().fa_forward_kvcache_paged.restype is ctypes.c_int
    assert fa.lib().fa_forward_kvcache_paged_workspace_bytes.restype is ctypes.c_size_t
    assert "fa_forward_kvcache_paged" in fa.__all__ and "kvcache_paged_workspace_bytes" in fa.__all__


def _call(fa, q=16, k=16, v=16, o=16, lse=None, lens=None, table=16, B=1, Hkv=1, G=1, Nq=1, num_pages=8, page_size=16, max_pages=12,
          d=64, scale=0.125, causal=0, in_dt=0, out_dt=0, ws=None, ws_bytes=0):
    """One call with small made-up addresses: every case below must be turned away before anything dereferences them.
    The defaults (a capacity of 192 keys, one pass) are a call that would be launched."""
    vp = ctypes.c_void_p
    return fa.lib().fa_forward_kvcache_paged(vp(q), vp(k), vp(v), vp(o), lse, lens, vp(table), B, Hkv, G, Nq, num_pages, page_size,
                                             max_pages, d, scale, causal, in_dt, out_dt, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [
    dict(page_size=0), dict(page_size=8), dict(page_size=24), dict(page_size=48), dict(page_size=-16),   # a power of two >= 16
    dict(k=0), dict(v=0), dict(table=0), dict(q=0), dict(o=0),                          # null pool, table, Q, O
    dict(num_pages=0), dict(num_pages=-3), dict(max_pages=0), dict(max_pages=-1),
    dict(max_pages=1 << 27, page_size=16), dict(max_pages=1 << 20, page_size=1 << 12),    # max_pages * page_size beyond int
    dict(max_pages=1 << 16, page_size=1 << 15),                                          # 2^31 exactly
    dict(max_pages=512, page_size=16),                                                   # split (8192 keys): NULL workspace
    dict(max_pages=512, page_size=16, ws=ctypes.c_void_p(16), ws_bytes=8),               # split: short workspace
    dict(max_pages=32, page_size=256, ws=None, ws_bytes=1 << 30),                        # split: NULL workspace with a size
    dict(max_pages=1 << 21, page_size=16, d=128, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),   # 2^33 bytes of keys: 32-bit offsets
    dict(max_pages=1 << 18, page_size=256, d=64, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),
    dict(max_pages=1, page_size=1 << 26, d=64, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),     # one page-head block of 2^33 bytes
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(G=0), dict(G=-2), dict(Nq=0),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0),                                      # d in {64, 128}
    dict(causal=2), dict(causal=-1),
    dict(in_dt=2), dict(in_dt=-1), dict(out_dt=2), dict(out_dt=7),
    dict(G=1 << 12, Nq=1 << 12, ws=ctypes.c_void_p(16), ws_bytes=1 << 40),               # G*Nq rows of (d+2)*4 bytes: 32-bit offsets
    dict(G=1 << 16, Nq=1 << 16), dict(B=1 << 16, Hkv=1 << 16),                           # products beyond int
])
def test_paged_rejects_without_device(fa, bad):
    assert _call(fa, **bad) == INVALID, bad


def test_paged_workspace_is_the_contiguous_one(fa):
    L = fa.lib()
    for page_size, max_pages in ((16, 66), (16, 515), (32, 257), (64, 17), (64, 129), (128, 65), (256, 5), (256, 33), (1024, 9)):
        for (B, Hkv, G, Nq, d) in ((3, 2, 2, 1, 64), (1, 1, 1, 1, 128), (2, 2, 4, 5, 128), (8, 16, 1, 1, 64)):
            want = L.fa_forward_kvcache_workspace_bytes(B, Hkv, G, Nq, max_pages * page_size, d)
            assert L.fa_forward_kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d) == want
            assert fa.kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d) == want
    assert L.fa_forward_kvcache_paged_workspace_bytes(1, 1, 1, 1, 512, 16, 64) > 0
    assert L.fa_forward_kvcache_paged_workspace_bytes(3, 2, 2, 1, 12, 16, 64) == 0   # 192 keys: one pass
    for bad in ((0, 1, 1, 1, 512, 16, 64), (1, 0, 1, 1, 512, 16, 64), (1, 1, 0, 1, 512, 16, 64), (1, 1, 1, 0, 512, 16, 64),
                (1, 1, 1, 1, 0, 16, 64), (1, 1, 1, 1, 512, 0, 64), (1, 1, 1, 1, 512, 8, 64), (1, 1, 1, 1, 512, 24, 64),
                (1, 1, 1, 1, 512, 16, 32), (1, 1, 1, 1, 1 << 27, 16, 64)):
        assert L.fa_forward_kvcache_paged_workspace_bytes(*bad) == 0, bad


def test_paged_op_refuses_cpu_tensors_and_bad_tables(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)
    table = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged(q, pool, pool, table)                      # CPU tensors
    # block_table is judged first, so these are refused for what is wrong with IT (q and the pools being CPU tensors is not reached)
    for bad in (table,                                                                  # int32 [B, max_pages], but not on the device
                torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.float32),
                torch.zeros(10, dtype=torch.int32), torch.zeros(2, 5, 1, dtype=torch.int32),   # rank
                torch.zeros(3, 5, dtype=torch.int32),                                           # batch
                torch.zeros(2, 10, dtype=torch.int32)[:, ::2], torch.zeros(5, 2, dtype=torch.int32).t(),   # not contiguous
                [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]):
        with pytest.raises(ValueError, match="block_table"):
            fa.fa_forward_kvcache_paged(q, pool, pool, bad)
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged(q, pool, pool[:5], table)                  # k_pool and v_pool differ in shape
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged(q, pool[0], pool[0], table)                # pools are 4-D
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged(torch.zeros(2, 3, 1, 64, dtype=torch.float16), pool, pool, table)   # Hq not a multiple of Hkv
    with pytest.raises(ValueError):
        fa.fa_forward_kvcache_paged(q, pool, pool, table, out_dtype=torch.bfloat16)


def test_decode_paged_custom_op_registers(fa):
    """torch.ops.fa_mi355.decode_paged exists after register(), traces on meta tensors, and has no CPU kernel."""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    register()
    q = torch.empty(2, 8, 3, 128, dtype=torch.bfloat16, device="meta")
    pool = torch.empty(40, 2, 32, 128, dtype=torch.bfloat16, device="meta")
    table = torch.empty(2, 16, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    o = torch.ops.fa_mi355.decode_paged(q, pool, pool, table, lens, 0.125, True, True)
    assert o.shape == q.shape and o.dtype == torch.float32
    o = torch.ops.fa_mi355.decode_paged(q, pool, pool, table, None, 0.125, False, False)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        c = torch.zeros(1, 1, 16, 64, dtype=torch.float16)
        torch.ops.fa_mi355.decode_paged(c, c, c, torch.zeros(1, 1, dtype=torch.int32), None, 0.125, False, True)
