"""CPU tier of the rotary append entries (fa_kvcache_append_rope, _paged_rope, _fp8_rope, _paged_fp8_rope): the symbols are exported
and bound, every rejection of the base entries still holds, the rotary arguments are judged before the device is touched, and the
Python front ends and custom ops refuse what they must.  Only calls that must be rejected are issued, so the file is safe where a
GPU is visible."""
import ctypes
import os

import pytest

import test_kvcache_append_host as base

INVALID = 1  # hipErrorInvalidValue
NAMES = tuple(n + "_rope" for n in base.NAMES)
VP = ctypes.c_void_p


def test_rope_symbols_exported(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    sym = fa.capi.SYMBOLS
    for n in NAMES:
        assert n in sym, n
        assert n not in sym[:9] and n not in sym[-2:], n   # between the head slice and the pinned tail
        assert hasattr(raw, n), n
        fn = getattr(fa.lib(), n)
        assert fn.restype is ctypes.c_int, n
        plain = getattr(fa.lib(), n[:-5]).argtypes
        assert len(fn.argtypes) == len(plain) + 8, n
        k = plain.index(ctypes.c_int)   # the insertion rule: four pointers before B, four ints after d
        assert list(fn.argtypes) == list(plain[:k]) + [VP] * 4 + list(plain[k:-2]) + [ctypes.c_int] * 4 + list(plain[-2:]), n
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fa_mi355.h")).read()
    for n in NAMES:
        assert f"int {n}(" in header, n
    assert "Rotary embedding, token-major" not in header and "a rot_dim that is not a multiple of 16" in header


def _call(fa, entry, knew=16, vnew=16, k=16, v=16, lens=None, out=None, table=16, ks=None, vs=None, q=4096, qout=4096, cos=16, sin=16,
          B=1, Hkv=1, Nnew=1, Ncap=192, num_pages=8, page_size=16, max_pages=12, d=64, G=1, rot_dim=64, max_pos=8, il=0, dt=0):
    """One call with small made-up addresses: every case below must be turned away before anything dereferences them.
    The defaults are a call that would be launched."""
    L = fa.lib()
    head = (VP(knew), VP(vnew), VP(k), VP(v), lens, out)
    rp = (VP(q) if q else None, VP(qout) if qout else None, VP(cos) if cos else None, VP(sin) if sin else None)
    ri = (G, rot_dim, max_pos, il)
    if entry == "fa_kvcache_append_rope":
        return L.fa_kvcache_append_rope(*head, *rp, B, Hkv, Nnew, Ncap, d, *ri, dt, None)
    if entry == "fa_kvcache_append_paged_rope":
        return L.fa_kvcache_append_paged_rope(*head, VP(table), *rp, B, Hkv, Nnew, num_pages, page_size, max_pages, d, *ri, dt, None)
    if entry == "fa_kvcache_append_fp8_rope":
        return L.fa_kvcache_append_fp8_rope(*head, ks, vs, *rp, B, Hkv, Nnew, Ncap, d, *ri, dt, None)
    return L.fa_kvcache_append_paged_fp8_rope(*head, VP(table), ks, vs, *rp, B, Hkv, Nnew, num_pages, page_size, max_pages, d, *ri, dt,
                                              None)


# every rejection of the base entries (tests/test_kvcache_append_host.py), with valid rotary arguments beside it
BASE_CASES = [(e, bad) for e in NAMES for bad in base.COMMON + (base.PAGED if "paged" in e else base.CONTIG)]
Q1 = 64 * 2   # bytes of Q at the defaults: one row of d = 64
ROPE = [
    dict(cos=0), dict(sin=0), dict(cos=0, sin=0, q=0, qout=0),                           # no table: not the plain append
    dict(rot_dim=0), dict(rot_dim=8), dict(rot_dim=24), dict(rot_dim=40), dict(rot_dim=-16), dict(rot_dim=63),
    dict(rot_dim=80), dict(rot_dim=128), dict(rot_dim=144, d=128), dict(rot_dim=1 << 30),   # a multiple of 16 in [16, d]
    dict(max_pos=0), dict(max_pos=-1), dict(G=0), dict(G=-4),
    dict(il=2), dict(il=-1),
    dict(B=1 << 12, Hkv=1 << 12, G=1 << 8), dict(B=1 << 15, Hkv=1 << 15, G=2),           # B * Hkv * G beyond int
    dict(B=1 << 10, Hkv=1 << 10, G=1 << 8),                                              # 2^31 chunks in Q (2^23 in K: accepted there)
    dict(B=1 << 8, Hkv=1 << 8, G=1 << 7, Nnew=1 << 4, d=128),
    dict(qout=0), dict(q=0),                                                             # exactly one of the two
    dict(q=4096, qout=4096 + 16), dict(q=4096, qout=4096 + Q1 - 2), dict(q=4096, qout=4096 - Q1 + 2),   # partial overlaps
    dict(B=4, G=2, q=1 << 20, qout=(1 << 20) + 4 * 2 * Q1 - 16),
]
ROPE_CASES = [(e, bad) for e in NAMES for bad in ROPE]


@pytest.mark.parametrize("entry,bad", BASE_CASES, ids=[f"{e[3:]}-{i}" for i, (e, _) in enumerate(BASE_CASES)])
def test_rope_entries_keep_the_base_rejections(fa, entry, bad):
    assert _call(fa, entry, **bad) == INVALID, (entry, bad)


@pytest.mark.parametrize("entry,bad", ROPE_CASES, ids=[f"{e[3:]}-{i}" for i, (e, _) in enumerate(ROPE_CASES)])
def test_rope_arguments_rejected_without_device(fa, entry, bad):
    assert _call(fa, entry, **bad) == INVALID, (entry, bad)


def test_rope_front_ends_refuse_bad_tensors(fa):
    torch = pytest.importorskip("torch")
    new, cache = base._tensors(torch)            # B 2, Hkv 2, Nnew 3, d 64; CPU tensors: a call that passes every check here still
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)   # ends in "must be a device tensor"
    table = torch.zeros(2, 2, dtype=torch.int32)
    c8, p8 = cache.to(torch.float8_e4m3fn), pool.to(torch.float8_e4m3fn)
    cos = torch.zeros(40, 32)
    q = torch.zeros(2, 6, 3, 64, dtype=torch.float16)
    fronts = ((fa.fa_kvcache_append, cache, ()), (fa.fa_kvcache_append_fp8, c8, ()))
    # (the paged front ends judge block_table first, as the decode ones do, and here it is a CPU tensor: they are covered through
    # the shared helper by the two contiguous ones, and by name below)
    for fn, dst, extra in fronts:
        def call(**kw):
            return fn(new, new, dst, dst, *extra, **kw)
        for kw in (dict(q=q), dict(q_out=q), dict(q=q, q_out=q), dict(rotary_sin=cos)):
            with pytest.raises(ValueError, match="need rotary_cos"):
                call(**kw)
        for bad in (cos.double(), cos.half(), cos[0], cos[None], [[1.0] * 32], cos.to(torch.int32)):
            with pytest.raises(ValueError, match="rotary_cos must be a float32"):
                call(rotary_cos=bad, rotary_sin=cos)
            with pytest.raises(ValueError, match="rotary_sin must be a float32"):
                call(rotary_cos=cos, rotary_sin=bad)
        with pytest.raises(ValueError, match="rotary_cos must be contiguous"):
            call(rotary_cos=torch.zeros(40, 64)[:, ::2], rotary_sin=cos)
        with pytest.raises(ValueError, match="rotary_sin must be contiguous"):
            call(rotary_cos=cos, rotary_sin=torch.zeros(32, 40).t())
        with pytest.raises(ValueError, match="one shape"):
            call(rotary_cos=cos, rotary_sin=cos[:39])
        with pytest.raises(ValueError, match="rotary_sin must be a float32"):
            call(rotary_cos=cos, rotary_sin=None)
        for width in (4, 12, 20, 36, 40, 64):   # rot_dim 8, 24, 40, 72, 80, 128 at d = 64
            w = torch.zeros(40, width)
            with pytest.raises(ValueError, match="multiple of 16"):
                call(rotary_cos=w, rotary_sin=w)
        with pytest.raises(ValueError, match="multiple of 16"):
            call(rotary_cos=torch.zeros(0, 32), rotary_sin=torch.zeros(0, 32))
        for bad in (q[0], q[:1], q[:, :5], q[:, :, :2], q[..., :32], q.bfloat16(), q.float(), torch.zeros(2, 0, 3, 64, dtype=torch.float16),
                    [1, 2]):
            with pytest.raises(ValueError, match=r"q must be \[B,Hq,Nnew,d\]"):
                call(q=bad, rotary_cos=cos, rotary_sin=cos)
        with pytest.raises(ValueError, match="q_out needs q"):
            call(q_out=q, rotary_cos=cos, rotary_sin=cos)
        for bad in (q[:, :2], q.bfloat16(), q[..., :32], 3):
            with pytest.raises(ValueError, match="q_out must have q's shape and dtype"):
                call(q=q, q_out=bad, rotary_cos=cos, rotary_sin=cos)
        # the existing refusals come first, in their order and wording
        with pytest.raises(ValueError, match="fp16 or both bf16"):
            fn(new, new.bfloat16(), dst, dst, *extra, rotary_cos=cos.double(), rotary_sin=cos)
        with pytest.raises(ValueError, match="device tensor"):   # all well: the first CPU tensor is named
            call(q=q, rotary_cos=cos, rotary_sin=cos, rotary_interleaved=True)
    for fn, dst in ((fa.fa_kvcache_append_paged, pool), (fa.fa_kvcache_append_paged_fp8, p8)):
        with pytest.raises(ValueError, match="block_table"):
            fn(new, new, dst, dst, table, q=q, rotary_cos=cos.double(), rotary_sin=cos)


def test_rope_custom_ops_register(fa):
    """torch.ops.fa_mi355.append*_rope exist after register(), trace on meta tensors, return nothing, mutate exactly the caches,
    seqlens_out and q, and have no CPU kernel."""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    register()
    new = torch.empty(2, 2, 1, 128, dtype=torch.bfloat16, device="meta")
    q = torch.empty(2, 8, 1, 128, dtype=torch.bfloat16, device="meta")
    cos = torch.empty(4096, 64, dtype=torch.float32, device="meta")

    def cache(dt=torch.bfloat16):
        return torch.empty(2, 2, 64, 128, dtype=dt, device="meta")

    def pool(dt=torch.bfloat16):
        return torch.empty(11, 2, 16, 128, dtype=dt, device="meta")

    table = torch.empty(2, 4, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    sc = torch.empty(2, dtype=torch.float32, device="meta")
    f8 = torch.float8_e4m3fn
    ops = torch.ops.fa_mi355
    assert ops.append_rope(new, new, cache(), cache(), lens, lens, q, cos, cos, False) is None
    assert ops.append_rope(new, new, cache(), cache(), None, None, None, cos, cos, True) is None
    assert ops.append_paged_rope(new, new, pool(), pool(), table, lens, None, q, cos, cos, False) is None
    assert ops.append_fp8_rope(new, new, cache(f8), cache(f8), sc, None, lens, lens, q, cos, cos, False) is None
    assert ops.append_paged_fp8_rope(new, new, pool(f8), pool(f8), table, sc, sc, None, lens, None, cos, cos, True) is None
    for name in ("append_rope", "append_paged_rope", "append_fp8_rope", "append_paged_fp8_rope"):
        schema = getattr(ops, name).default._schema
        mutated = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
        assert mutated == {"k_pool" if "paged" in name else "k_cache", "v_pool" if "paged" in name else "v_cache", "seqlens_out", "q"}, name
        assert len(schema.returns) == 0, name
        plain = getattr(ops, name[:-5]).default._schema
        assert [a.name for a in schema.arguments] == [a.name for a in plain.arguments] + ["q", "rotary_cos", "rotary_sin", "interleaved"]
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        c = torch.zeros(1, 1, 16, 64, dtype=torch.float16)
        t = torch.zeros(8, 32)
        ops.append_rope(c[:, :, :1], c[:, :, :1].clone(), c, c.clone(), None, None, None, t, t.clone(), False)
