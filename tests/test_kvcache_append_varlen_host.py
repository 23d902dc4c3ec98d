"""CPU tier of the packed append fa_kvcache_append_varlen: the symbol is exported and bound, the ctypes structure mirrors the header,
every rejection the header lists holds before the device is touched, the Python front ends check shapes and dtypes, and the two
torch ops register.  Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os
import re

import pytest

import test_kvcache_append_host as base

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fa_kvcache_append_varlen"
KINDS = ("", "paged_", "fp8_", "paged_fp8_", "rope", "paged_rope", "fp8_rope", "paged_fp8_rope")
FIELDS = ["size", "Knew", "Vnew", "K", "V", "cu_seqlens_new", "seqlens_k", "seqlens_out", "block_table", "k_scale", "v_scale", "Q", "Qout",
          "rope_cos", "rope_sin", "kv_dtype", "B", "Hkv", "d", "total_new", "Ncap", "num_pages", "page_size", "max_pages", "G", "rot_dim",
          "max_pos", "interleaved", "dtype", "k_stride_t", "k_stride_h", "v_stride_t", "v_stride_h", "q_stride_t", "q_stride_h",
          "qo_stride_t", "qo_stride_h", "stream"]


def _header():
    return open(os.path.join(ROOT, "include", "fa_mi355.h")).read()


def _header_fields(struct):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1), flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if decl.strip()]


def test_symbol_and_struct(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    sym = fa.capi.SYMBOLS
    assert NAME in sym and hasattr(raw, NAME)
    assert NAME not in sym[:9] and NAME not in sym[-2:]   # between the head slice and the pinned tail
    fn = getattr(fa.lib(), NAME)
    assert fn.argtypes == [ctypes.POINTER(fa.capi.KvAppendVarlenDesc)] and fn.restype is ctypes.c_int
    assert _header_fields("fa_kvappend_varlen_desc") == [f[0] for f in fa.capi.KvAppendVarlenDesc._fields_] == FIELDS
    types = dict(fa.capi.KvAppendVarlenDesc._fields_)
    assert all(types[n] is ctypes.c_longlong for n in FIELDS if "stride" in n) and types["total_new"] is ctypes.c_int
    assert fa.capi.KvAppendVarlenDesc().size == ctypes.sizeof(fa.capi.KvAppendVarlenDesc)
    header = _header()
    assert "int fa_kvcache_append_varlen(const fa_kvappend_varlen_desc* desc);" in header
    # the older entries no longer list packed sources as missing, and point here
    assert "not part of this entry: token-packed" not in header.lower() and header.count(NAME + ",") + header.count(NAME + "'s") >= 2
    # fa_kvappend_desc stays what it was
    assert [f[0] for f in fa.capi.KvAppendDesc._fields_] == _header_fields("fa_kvappend_desc")
    for name in ("fa_kvcache_append_varlen", "fa_kvcache_append_varlen_fp8"):
        assert name in fa.__all__ and callable(getattr(fa, name))


def _desc(fa, kind="", **kw):
    """a descriptor with small made-up addresses that WOULD be launched; test_kvcache_append_host's keyword names where they exist"""
    names = dict(knew="Knew", vnew="Vnew", k="K", v="V", lens="seqlens_k", out="seqlens_out", table="block_table", ks="k_scale",
                 vs="v_scale", q="Q", qout="Qout", cos="rope_cos", sin="rope_sin", il="interleaved", dt="dtype", cu="cu_seqlens_new",
                 total="total_new")
    f = dict(Knew=4096, Vnew=8192, K=16, V=16, cu_seqlens_new=16, B=1, Hkv=1, d=64, total_new=4, dtype=0, k_stride_t=64, k_stride_h=64,
             v_stride_t=64, v_stride_h=64)
    if "paged" in kind:
        f.update(block_table=16, num_pages=8, page_size=16, max_pages=12)
    else:
        f.update(Ncap=192)
    if "fp8" in kind:
        f.update(kv_dtype=fa.capi.KV_FP8_E4M3)
    if "rope" in kind:
        f.update(Q=1 << 20, Qout=1 << 20, rope_cos=16, rope_sin=16, G=1, rot_dim=64, max_pos=8, interleaved=0, q_stride_t=64,
                 q_stride_h=64, qo_stride_t=64, qo_stride_h=64)
    for k, v in kw.items():
        f[names.get(k, k)] = v.value if isinstance(v, ctypes.c_void_p) else v
    if "paged" in kind:
        f.pop("Ncap", None)
    return fa.capi.KvAppendVarlenDesc(**f)


def _call(fa, kind="", **kw):
    return getattr(fa.lib(), NAME)(ctypes.byref(_desc(fa, kind, **kw)))


# what the descriptor alone can get wrong, and the packed sources
COMMON = [
    dict(size=0), dict(size=8), dict(size=512), dict(kv_dtype=2), dict(kv_dtype=-1),
    dict(knew=0), dict(vnew=0), dict(k=0), dict(v=0), dict(cu=0),
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(Hkv=-2), dict(total=0), dict(total=-1),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0), dict(dt=2), dict(dt=-1),
    dict(B=1 << 16, Hkv=1 << 16),                                                        # B * Hkv beyond int
    dict(total=1 << 18, Hkv=1 << 10, d=64), dict(total=1 << 17, Hkv=1 << 10, d=128),     # 2^31 chunks: the kernel's index type
    dict(total=(1 << 31) - 1, Hkv=2, d=64),
    # fa_varlen_desc's rules for a packed tensor
    dict(k_stride_t=56), dict(v_stride_t=0), dict(k_stride_t=-64), dict(k_stride_h=-64), dict(v_stride_h=-8),
    dict(k_stride_t=68), dict(v_stride_t=100), dict(k_stride_h=4), dict(v_stride_h=36), dict(d=128, k_stride_t=64),
    dict(knew=4096 + 8), dict(vnew=8192 + 2), dict(knew=4096 + 4),
    # seqlens_out overlapping seqlens_k without being it (B = 4: 16 bytes each)
    dict(B=4, lens=1 << 16, out=(1 << 16) + 4), dict(B=4, lens=1 << 16, out=(1 << 16) + 12), dict(B=4, lens=1 << 16, out=(1 << 16) - 12),
    # cu_seqlens_new (B + 1 = 5 entries: 20 bytes) overlapping seqlens_out, identity included, with and without seqlens_k = seqlens_out
    dict(B=4, cu=1 << 16, out=1 << 16), dict(B=4, cu=1 << 16, out=(1 << 16) + 16), dict(B=4, cu=1 << 16, out=(1 << 16) - 12),
    dict(B=4, cu=1 << 16, out=(1 << 16) + 16, lens=(1 << 16) + 16), dict(B=4, cu=(1 << 16) + 12, out=1 << 16, lens=1 << 16),
]
Q1 = 4 * 64 * 2   # bytes of the default Q: 4 tokens, one head, d = 64
ROPE = [
    dict(sin=0), dict(rot_dim=0), dict(rot_dim=8), dict(rot_dim=24), dict(rot_dim=40), dict(rot_dim=-16), dict(rot_dim=80),
    dict(rot_dim=128), dict(rot_dim=144, d=128, k_stride_t=128, v_stride_t=128, q_stride_t=128, qo_stride_t=128),
    dict(max_pos=0), dict(max_pos=-1), dict(G=0), dict(G=-4), dict(il=2), dict(il=-1),
    dict(B=1 << 12, Hkv=1 << 12, G=1 << 8),                                              # B * Hkv * G beyond int
    dict(total=1 << 12, Hkv=1 << 10, G=1 << 6, q_stride_h=0, qo_stride_h=0),            # 2^31 chunks in Q (2^25 in K: accepted there)
    dict(qout=0), dict(q=0),                                                             # exactly one of the two
    dict(q_stride_t=56), dict(qo_stride_t=32), dict(q_stride_h=-64), dict(qo_stride_h=4), dict(q_stride_t=72, qo_stride_t=68),
    dict(q=(1 << 20) + 8), dict(qout=(1 << 20) + 4),
    # Qout neither Q with equal strides nor disjoint from Q's extent
    dict(qout=(1 << 20) + 16), dict(qout=(1 << 20) + Q1 - 16), dict(qout=(1 << 20) - Q1 + 16),
    dict(qo_stride_t=128), dict(G=2, qo_stride_h=128, qo_stride_t=256),                  # the same base through other strides
    dict(q_stride_t=128, qout=(1 << 20) + 128),                                          # interleaved with Q's padded rows
]


@pytest.mark.parametrize("kind", KINDS)
def test_rejections(fa, kind):
    L = fa.lib()
    assert getattr(L, NAME)(None) == INVALID
    assert _call(fa, kind, size=ctypes.sizeof(fa.capi.KvAppendVarlenDesc) - 8) == INVALID
    assert _call(fa, kind, size=ctypes.sizeof(fa.capi.KvAppendDesc)) == INVALID
    cases = COMMON + (base.PAGED if "paged" in kind else base.CONTIG) + (ROPE if "rope" in kind else [])
    for bad in cases:
        assert _call(fa, kind, **bad) == INVALID, (kind, bad)
    if "fp8" not in kind:   # a 16-bit cache has no scales
        assert _call(fa, kind, ks=16) == INVALID and _call(fa, kind, vs=16) == INVALID
    if "rope" not in kind:  # arguments of the rotary forms without a table
        for bad in (dict(q=4096, qout=4096), dict(q=4096), dict(qout=4096), dict(sin=16)):
            assert _call(fa, kind, **bad) == INVALID, (kind, bad)


def test_python_front_end_checks(fa):
    torch = pytest.importorskip("torch")
    f16, i32 = torch.float16, torch.int32
    fused = torch.zeros(12, 4 + 2 * 2, 64, dtype=f16)          # (total, Hq + 2 Hkv, d): views, as the projection leaves them
    q, k, v = fused[:, :4], fused[:, 4:6], fused[:, 6:]
    cache = torch.zeros(3, 2, 32, 64, dtype=f16)
    pool = torch.zeros(9, 2, 16, 64, dtype=f16)
    cache8, pool8 = cache.to(torch.float8_e4m3fn), pool.to(torch.float8_e4m3fn)
    cu = torch.tensor([0, 5, 5, 12], dtype=i32)
    lens = torch.zeros(3, dtype=i32)
    table = torch.zeros(3, 2, dtype=i32)
    cos = torch.zeros(8, 16)
    av, av8 = fa.fa_kvcache_append_varlen, fa.fa_kvcache_append_varlen_fp8
    bad = [
        (lambda: av(k[0], v[0], cache, cache, cu), "packed"),
        (lambda: av(k, v[:, :1], cache, cache, cu), "packed"),
        (lambda: av(k, v.float(), cache, cache, cu), "fp16 or both bf16"),
        (lambda: av(k.float(), v.float(), cache, cache, cu), "fp16 or both bf16"),
        (lambda: av(fused[:, :2, :32], fused[:, 2:4, :32], cache, cache, cu), "64 or 128"),
        (lambda: av(k, v, cache[:, :1], cache[:, :1], cu), "Hkv and d"),
        (lambda: av(k, v, cache, cache[:, :, :16], cu), "Hkv and d"),
        (lambda: av(k, v, cache.bfloat16(), cache.bfloat16(), cu), "dtype of k_new"),
        (lambda: av(k, v, cache8, cache8, cu), "dtype of k_new"),
        (lambda: av8(k, v, cache, cache, cu), "float8_e4m3fn"),
        (lambda: av8(k, v, cache8.view(torch.uint8).view(torch.float8_e5m2), cache8, cu), "float8_e4m3fn"),
        (lambda: av(k, v, cache, cache, cu.long()), "int32"),
        (lambda: av(k, v, cache, cache, cu[:1]), "B\\+1"),
        (lambda: av(k, v, cache, cache, torch.zeros(8, dtype=i32)[::2]), "B\\+1"),
        (lambda: av(k, v, cache, cache, cu[:3]), "holds 3 sequences"),
        (lambda: av(k, v, pool, pool, cu, block_table=table[:2]), "block_table"),
        (lambda: av(k, v, torch.zeros(9, 2, 24, 64, dtype=f16), torch.zeros(9, 2, 24, 64, dtype=f16), cu, block_table=table), "power of two"),
        (lambda: av(k, v, cache, cache, cu, cache_seqlens=lens[:2]), "cache_seqlens"),
        (lambda: av(k, v, cache, cache, cu, seqlens_out=lens.long()), "seqlens_out"),
        (lambda: av(torch.zeros(12, 2, 128, dtype=f16)[..., ::2], v, cache, cache, cu), "contiguous in its last dimension"),
        (lambda: av(k, v, cache, cache, cu, q=q), "need rotary_cos"),
        (lambda: av(k, v, cache, cache, cu, rotary_sin=cos), "need rotary_cos"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=cos, rotary_sin=cos[:4]), "one shape"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=torch.zeros(8, 12), rotary_sin=torch.zeros(8, 12)), "rot_dim"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=cos, rotary_sin=cos, q_out=q), "q_out needs q"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=cos, rotary_sin=cos, q=q[:8]), "total_new, Hq, d"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=cos, rotary_sin=cos, q=fused[:, :3]), "multiple of Hkv"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=cos, rotary_sin=cos, q=q.transpose(0, 1)), "total_new, Hq, d"),
        (lambda: av(k, v, cache, cache, cu, rotary_cos=cos, rotary_sin=cos, q=q, q_out=q.bfloat16()), "q's shape and dtype"),
        (lambda: av8(k, v, cache8, cache8, cu, k_scale=torch.ones(3)), "k_scale"),
    ]
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
    # a call that is right in shape and dtype still has no CPU path: the strided views are taken as they are, then refused as host memory
    for call in (lambda: av(k, v, cache, cache, cu, lens, lens), lambda: av(k, v, pool, pool, cu, lens, lens, table),
                 lambda: av(k, v, cache, cache, cu, q=q, rotary_cos=cos, rotary_sin=cos),
                 lambda: av8(k, v, cache8, cache8, cu, lens, None, None, torch.ones(2), torch.ones(2)),
                 lambda: av8(k, v, pool8, pool8, cu, block_table=table, q=q, q_out=torch.zeros(12, 4, 64, dtype=f16), rotary_cos=cos,
                             rotary_sin=cos, rotary_interleaved=True)):
        with pytest.raises(ValueError, match="must be a device tensor"):
            call()
    assert fused.count_nonzero() == 0


def test_custom_ops_register(fa):
    """the two ops exist after register(), trace on meta tensors, mutate what they say, return nothing and have no CPU kernel"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    meta = dict(device="meta")
    fused = torch.empty(40, 8 + 2 * 2, 128, dtype=torch.bfloat16, **meta)
    q, k, v = fused[:, :8], fused[:, 8:10], fused[:, 10:]
    cache = torch.empty(3, 2, 500, 128, dtype=torch.bfloat16, **meta)
    pool = torch.empty(40, 2, 32, 128, dtype=torch.bfloat16, **meta)
    cache8, pool8 = (torch.empty(x.shape, dtype=torch.float8_e4m3fn, **meta) for x in (cache, pool))
    cu, lens = torch.empty(4, dtype=torch.int32, **meta), torch.empty(3, dtype=torch.int32, **meta)
    table = torch.empty(3, 16, dtype=torch.int32, **meta)
    sc = torch.empty(2, dtype=torch.float32, **meta)
    cos = torch.empty(64, 64, dtype=torch.float32, **meta)
    qo = torch.empty(40, 8, 128, dtype=torch.bfloat16, **meta)
    for rot in ((q, None, cos, cos), (q, qo, cos, cos), (None, None, cos, cos), (None, None, None, None)):
        assert ops.append_varlen(k, v, cache, cache, cu, lens, lens, None, *rot, False) is None
        assert ops.append_varlen(k, v, pool, pool, cu, None, None, table, *rot, True) is None
        assert ops.append_varlen_fp8(k, v, cache8, cache8, cu, lens, None, None, sc, None, *rot, False) is None
        assert ops.append_varlen_fp8(k, v, pool8, pool8, cu, lens, lens, table, sc, sc, *rot, False) is None

    def args(name):
        return [(a.name, str(a.type)) for a in getattr(ops, name).default._schema.arguments]

    plain, fp8 = args("append_varlen"), args("append_varlen_fp8")
    assert [n for n, _ in plain] == ["k_new", "v_new", "k_cache", "v_cache", "cu_seqlens_new", "cache_seqlens", "seqlens_out", "block_table",
                                     "q", "q_out", "rotary_cos", "rotary_sin", "interleaved"]
    i = [n for n, _ in plain].index("block_table") + 1
    assert fp8 == plain[:i] + [("k_scale", "Optional[Tensor]"), ("v_scale", "Optional[Tensor]")] + plain[i:]
    for name in ("append_varlen", "append_varlen_fp8"):
        schema = getattr(ops, name).default._schema
        mutated = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
        assert mutated == {"k_cache", "v_cache", "seqlens_out", "q", "q_out"} and len(schema.returns) == 0
    c = torch.zeros(1, 1, 64, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.append_varlen(c[0], c[0].clone(), c, c.clone(), torch.zeros(2, dtype=torch.int32), None, None, None, None, None, None, None, False)
