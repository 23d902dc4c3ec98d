"""CPU tier of the KV-cache append entries (fa_kvcache_append, _paged, _fp8, _paged_fp8): the symbols are exported and bound, bad
arguments are rejected before the device is touched, and the Python front ends refuse what they must.  Only calls that must be
rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os

import pytest

INVALID = 1  # hipErrorInvalidValue
NAMES = ("fa_kvcache_append", "fa_kvcache_append_paged", "fa_kvcache_append_fp8", "fa_kvcache_append_paged_fp8")


def test_append_symbols_exported(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    for n in NAMES:
        assert n in fa.capi.SYMBOLS, n
        assert n not in fa.capi.SYMBOLS[:9] and n not in fa.capi.SYMBOLS[-2:], n   # between the head slice and the pinned tail
        assert hasattr(raw, n), n
        assert getattr(fa.lib(), n).restype is ctypes.c_int, n
        assert n in fa.__all__ and callable(getattr(fa, n)), n
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fa_mi355.h")).read()
    for n in NAMES:
        assert f"int {n}(" in header, n


def _call(fa, entry, knew=16, vnew=16, k=16, v=16, lens=None, out=None, table=16, ks=None, vs=None, B=1, Hkv=1, Nnew=1, Ncap=192,
          num_pages=8, page_size=16, max_pages=12, d=64, dt=0):
    """One call with small made-up addresses: every case below must be turned away before anything dereferences them.
    The defaults (a capacity of 192 keys) are a call that would be launched."""
    vp = ctypes.c_void_p
    L = fa.lib()
    head = (vp(knew), vp(vnew), vp(k), vp(v), lens, out)
    if entry == "fa_kvcache_append":
        return L.fa_kvcache_append(*head, B, Hkv, Nnew, Ncap, d, dt, None)
    if entry == "fa_kvcache_append_paged":
        return L.fa_kvcache_append_paged(*head, vp(table), B, Hkv, Nnew, num_pages, page_size, max_pages, d, dt, None)
    if entry == "fa_kvcache_append_fp8":
        return L.fa_kvcache_append_fp8(*head, ks, vs, B, Hkv, Nnew, Ncap, d, dt, None)
    return L.fa_kvcache_append_paged_fp8(*head, vp(table), ks, vs, B, Hkv, Nnew, num_pages, page_size, max_pages, d, dt, None)


COMMON = [
    dict(knew=0), dict(vnew=0), dict(k=0), dict(v=0),                                    # null source, cache or pool
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(Hkv=-2), dict(Nnew=0), dict(Nnew=-1),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0),                                      # d in {64, 128}
    dict(dt=2), dict(dt=-1),
    dict(B=1 << 16, Hkv=1 << 16),                                                        # B * Hkv beyond int
    dict(B=1 << 10, Hkv=1 << 10, Nnew=1 << 8, d=64),                                     # 2^31 chunks: the kernel's index type
    dict(B=1 << 10, Hkv=1 << 10, Nnew=1 << 7, d=128),
    dict(Nnew=(1 << 31) - 1, B=2, d=64),
    # seqlens_out overlapping seqlens_k without being it (B = 4: 16 bytes each)
    dict(B=4, lens=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096 + 4)),
    dict(B=4, lens=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096 + 12)),
    dict(B=4, lens=ctypes.c_void_p(4096), out=ctypes.c_void_p(4096 - 12)),
]
CONTIG = [
    dict(Ncap=0), dict(Ncap=-128),
    dict(Ncap=1 << 25, d=128), dict(Ncap=1 << 26, d=64), dict(Ncap=(1 << 31) - 1),      # the decode entries' bound on Ncap
]
PAGED = [
    dict(table=0),
    dict(page_size=0), dict(page_size=8), dict(page_size=24), dict(page_size=48), dict(page_size=-16),   # a power of two >= 16
    dict(num_pages=0), dict(num_pages=-3), dict(max_pages=0), dict(max_pages=-1),
    dict(max_pages=1 << 27, page_size=16), dict(max_pages=1 << 20, page_size=1 << 12),   # max_pages * page_size beyond int
    dict(max_pages=1 << 16, page_size=1 << 15),                                          # 2^31 exactly
    dict(max_pages=1 << 21, page_size=16, d=128), dict(max_pages=1 << 18, page_size=256, d=64),   # the bound on the capacity
    dict(max_pages=1, page_size=1 << 26, d=64),
]
CASES = [(e, bad) for e in NAMES for bad in COMMON + (PAGED if "paged" in e else CONTIG)]


@pytest.mark.parametrize("entry,bad", CASES, ids=[f"{e[3:]}-{i}" for i, (e, _) in enumerate(CASES)])
def test_append_rejects_without_device(fa, entry, bad):
    assert _call(fa, entry, **bad) == INVALID, (entry, bad)


def _tensors(torch, dt=None, cache_dt=None, B=2, Hkv=2, Nnew=3, Ncap=32, d=64):
    dt = dt or torch.float16
    new = torch.zeros(B, Hkv, Nnew, d, dtype=dt)
    cache = torch.zeros(B, Hkv, Ncap, d, dtype=cache_dt or dt)
    return new, cache


def test_append_ops_refuse_bad_tensors(fa):
    torch = pytest.importorskip("torch")
    new, cache = _tensors(torch)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)
    table = torch.zeros(2, 2, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    c8, p8 = cache.to(torch.float8_e4m3fn), pool.to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_kvcache_append(new, new, cache, cache)                                   # CPU tensors
    with pytest.raises(ValueError, match="dtype of k_new"):
        fa.fa_kvcache_append(new, new, cache.bfloat16(), cache.bfloat16())             # k_new's dtype is not the cache's
    with pytest.raises(ValueError, match="dtype of k_new"):
        fa.fa_kvcache_append(new, new, c8, c8)                                         # an fp8 cache through the 16-bit entry
    with pytest.raises(ValueError):   # (the paged front ends judge block_table first, as the decode ones do: here it is a CPU tensor)
        fa.fa_kvcache_append_paged(new, new, pool.bfloat16(), pool.bfloat16(), table)
    with pytest.raises(ValueError, match="fp16 or both bf16"):
        fa.fa_kvcache_append(new.float(), new.float(), cache.float(), cache.float())
    with pytest.raises(ValueError, match="fp16 or both bf16"):
        fa.fa_kvcache_append(new, new.bfloat16(), cache, cache)
    for bad8 in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float16, torch.uint8):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            fa.fa_kvcache_append_fp8(new, new, cache.to(bad8), cache.to(bad8))
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            fa.fa_kvcache_append_paged_fp8(new, new, pool.to(bad8), pool.to(bad8), table)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        fa.fa_kvcache_append_fp8(new, new, c8, cache)                                  # only one of the two is fp8
    # shapes
    for fn, dst, extra in ((fa.fa_kvcache_append, cache, ()), (fa.fa_kvcache_append_fp8, c8, ()),
                           (fa.fa_kvcache_append_paged, pool, (table,)), (fa.fa_kvcache_append_paged_fp8, p8, (table,))):
        with pytest.raises(ValueError):
            fn(new[0], new[0], dst, dst, *extra)                                       # new rows are 4-D
        with pytest.raises(ValueError):
            fn(new, new[:, :, :2], dst, dst, *extra)                                   # k_new and v_new differ in shape
        with pytest.raises(ValueError):
            fn(new, new, dst, dst[:, :, :8], *extra)                                   # the two caches differ in shape
        with pytest.raises(ValueError):
            fn(new, new, dst[0], dst[0], *extra)                                       # caches are 4-D
        with pytest.raises(ValueError):
            fn(new[:, :1], new[:, :1], dst, dst, *extra)                               # Hkv
        with pytest.raises(ValueError):
            fn(new[..., :32], new[..., :32], dst, dst, *extra)                         # d
        for name in ("cache_seqlens", "seqlens_out"):
            for bad in (lens.long(), lens.float(), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), [0, 0],
                        lens):                                                         # the last: int32 [B], but not on the device
                with pytest.raises(ValueError, match=None if extra else name):   # (paged: the CPU block_table is refused first)
                    fn(new, new, dst, dst, *extra, **{name: bad})
    with pytest.raises(ValueError):
        fa.fa_kvcache_append(new[:1], new[:1], cache, cache)                           # batch
    for bad in (table, torch.zeros(2, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32),
                torch.zeros(2, 4, dtype=torch.int32)[:, ::2], [[0, 1], [2, 3]]):
        with pytest.raises(ValueError, match="block_table"):
            fa.fa_kvcache_append_paged(new, new, pool, pool, bad)
        with pytest.raises(ValueError, match="block_table"):
            fa.fa_kvcache_append_paged_fp8(new, new, p8, p8, bad)
    for name in ("k_scale", "v_scale"):
        for bad in (torch.ones(2), torch.ones(3), torch.ones(2, dtype=torch.float64), torch.ones(2, 1), 1.0):
            with pytest.raises(ValueError, match=name):
                fa.fa_kvcache_append_fp8(new, new, c8, c8, **{name: bad})


def test_append_custom_ops_register(fa):
    """torch.ops.fa_mi355.append* exist after register(), trace on meta tensors, return nothing and have no CPU kernel."""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    register()
    new = torch.empty(2, 2, 1, 128, dtype=torch.bfloat16, device="meta")

    def cache(dt=torch.bfloat16):
        return torch.empty(2, 2, 64, 128, dtype=dt, device="meta")

    def pool(dt=torch.bfloat16):
        return torch.empty(11, 2, 16, 128, dtype=dt, device="meta")

    table = torch.empty(2, 4, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    sc = torch.empty(2, dtype=torch.float32, device="meta")
    f8 = torch.float8_e4m3fn
    assert torch.ops.fa_mi355.append(new, new, cache(), cache(), lens, lens) is None
    assert torch.ops.fa_mi355.append(new, new, cache(), cache(), None, None) is None
    assert torch.ops.fa_mi355.append_paged(new, new, pool(), pool(), table, lens, None) is None
    assert torch.ops.fa_mi355.append_fp8(new, new, cache(f8), cache(f8), sc, None, lens, lens) is None
    assert torch.ops.fa_mi355.append_paged_fp8(new, new, pool(f8), pool(f8), table, sc, sc, None, lens) is None
    for name in ("append", "append_paged", "append_fp8", "append_paged_fp8"):
        schema = getattr(torch.ops.fa_mi355, name).default._schema
        mutated = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
        assert mutated == {"k_pool" if "paged" in name else "k_cache", "v_pool" if "paged" in name else "v_cache", "seqlens_out"}, name
        assert len(schema.returns) == 0, name
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        c = torch.zeros(1, 1, 16, 64, dtype=torch.float16)
        torch.ops.fa_mi355.append(c[:, :, :1], c[:, :, :1].clone(), c, c.clone(), None, None)
