"""CPU tier of fa_forward_varlen_kvcache (the varlen prefill against the KV cache, contiguous or paged): the symbol is exported,
declared and bound; capi.VarlenKvcacheDesc mirrors the header's structure (names, offsets and size, against the C compiler); every
rejection holds before the device is touched, contiguous and paged, with and without options; the front end is exported and refuses
what it must; the torch op traces on meta tensors.  Only calls that must be rejected are issued, with small made-up addresses, so the
file is safe where a GPU is visible."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from test_varlen_host import INVALID, ROOT, _header, _header_fields

FIELDS = ["size", "Q", "O", "lse", "K", "V", "cu_seqlens_q", "seqlens_k", "block_table", "B", "Hkv", "G", "d", "total_q", "Ncap",
          "num_pages", "page_size", "max_pages", "q_stride_t", "q_stride_h", "o_stride_t", "o_stride_h", "scale", "causal", "in_dtype",
          "out_dtype", "sinks", "window", "softcap", "stream"]


def test_symbol_and_struct(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    assert "fa_forward_varlen_kvcache" in fa.capi.SYMBOLS and hasattr(raw, "fa_forward_varlen_kvcache")
    assert L.fa_forward_varlen_kvcache.argtypes == [ctypes.POINTER(fa.capi.VarlenKvcacheDesc)]
    assert L.fa_forward_varlen_kvcache.restype is ctypes.c_int
    assert "fa_forward_varlen_kvcache" in fa.__all__ and callable(fa.fa_forward_varlen_kvcache)
    header = _header()
    assert "int fa_forward_varlen_kvcache(const fa_varlen_kvcache_desc* desc);" in header
    assert _header_fields("fa_varlen_kvcache_desc") == [f[0] for f in fa.capi.VarlenKvcacheDesc._fields_] == FIELDS
    assert fa.capi.VarlenKvcacheDesc().size == ctypes.sizeof(fa.capi.VarlenKvcacheDesc)
    low = re.sub(r"\s+", " ", header.lower())
    for words in ("nothing on the host reads device data", "table entries at or past ceil(lk_b / page_size) are never read",
                  "the chunk's own tokens included", "not part of this entry: fp8 caches; split-kv for a short chunk",
                  "is fa_forward_varlen_kvcache's, further below", "are fa_forward_varlen_kvcache's, below"):
        assert words in low, words


def test_descriptor_layout_matches_the_c_compiler(fa, tmp_path):
    src = tmp_path / "layout.c"
    prints = " ".join('printf("%%zu\\n", offsetof(fa_varlen_kvcache_desc, %s));' % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fa_mi355.h"\nint main(void) { fa_varlen_kvcache_desc v = {0}; '
                   'v.size = sizeof v; v.page_size = 16; v.softcap = 50.0f; printf("%zu\\n", sizeof(fa_varlen_kvcache_desc)); ' + prints +
                   ' return v.block_table != 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = fa.capi.VarlenKvcacheDesc
    assert got[0] == ctypes.sizeof(D)
    assert got[1:] == [getattr(D, f).offset for f in FIELDS]
    assert ctypes.sizeof(fa.capi.VarlenDesc) == 176 and ctypes.sizeof(fa.capi.VarlenOpts) == 24     # the others did not change


def _desc(fa, paged, **kw):
    """a descriptor with small made-up addresses that WOULD be launched: (300, 4, 64) queries on a cache of 2 sequences, 2 K/V heads
    and 640 keys, contiguous or as 40 + 3 pages of 32"""
    f = dict(Q=4096, O=16384, lse=20480, K=8192, V=12288, cu_seqlens_q=32, seqlens_k=64, B=2, Hkv=2, G=2, d=64, total_q=300,
             q_stride_t=256, q_stride_h=64, o_stride_t=256, o_stride_h=64, scale=0.125, causal=1, in_dtype=0, out_dtype=0)
    f.update(dict(block_table=128, num_pages=43, page_size=32, max_pages=20) if paged else dict(Ncap=640))
    f.update(kw)
    return fa.capi.VarlenKvcacheDesc(**f)


def _call(fa, paged, **kw):
    return fa.lib().fa_forward_varlen_kvcache(ctypes.byref(_desc(fa, paged, **kw)))


OPTS = {"off": {}, "window": dict(window=17), "softcap": dict(softcap=30.0), "sinks": dict(sinks=256),
        "all": dict(window=1, softcap=0.5, sinks=256)}


@pytest.mark.parametrize("opts", sorted(OPTS))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_rejections_without_device(fa, paged, opts):
    """everything fa_forward_varlen_ex refuses for Q, O, lse, B, Hkv, G, d, the dtypes, window and softcap, and the cache's own"""
    o = OPTS[opts]

    def call(**kw):
        return _call(fa, paged, **dict(o, **kw))

    assert fa.lib().fa_forward_varlen_kvcache(None) == INVALID
    size = ctypes.sizeof(fa.capi.VarlenKvcacheDesc)
    for bad in (0, 8, size - 8, size + 8, 1 << 20):
        assert call(size=bad) == INVALID, bad
    for name in ("Q", "K", "V", "O", "cu_seqlens_q", "seqlens_k"):
        assert call(**{name: 0}) == INVALID, name
    for name in ("B", "Hkv", "G", "total_q"):
        for v in (0, -1, -(1 << 31)):
            assert call(**{name: v}) == INVALID, (name, v)
    for d in (0, 32, 96, 256, -64):
        assert call(d=d, q_stride_t=1024, o_stride_t=1024) == INVALID, d
    for name in ("in_dtype", "out_dtype"):
        for v in (-1, 2, 99):
            assert call(**{name: v}) == INVALID, (name, v)
    for t in "qo":
        assert call(**{t + "_stride_t": 56}) == INVALID, t            # below d
        assert call(**{t + "_stride_t": 0}) == INVALID, t
        assert call(**{t + "_stride_t": -256}) == INVALID, t
        assert call(**{t + "_stride_h": -64}) == INVALID, t           # negative
        for s in ("_stride_t", "_stride_h"):                           # not a multiple of 8 elements
            for v in (260, 132, 68, 257):
                assert call(**{t + s: v}) == INVALID, (t, s, v)
    for name in ("Q", "K", "V", "O"):                                  # 16-byte loads and stores
        for off in (2, 4, 8):
            assert call(**{name: 4096 + off}) == INVALID, (name, off)
    assert call(total_q=1 << 23, out_dtype=1) == INVALID              # Q's last byte at 2^32
    assert call(total_q=1 << 22) == INVALID                           # O alone, in fp32
    assert call(q_stride_h=1 << 30) == INVALID and call(q_stride_t=1 << 62) == INVALID and call(o_stride_h=(1 << 63) - 8) == INVALID
    for shape in (dict(B=1 << 16, Hkv=1 << 8, G=1 << 8), dict(B=1, Hkv=1 << 16, G=1 << 15), dict(B=(1 << 31) - 1, Hkv=2, G=1)):
        assert call(q_stride_h=0, o_stride_h=0, **shape) == INVALID, shape
    flat = dict(q_stride_t=64, q_stride_h=0, o_stride_t=64, o_stride_h=0, out_dtype=1)
    assert call(B=1 << 15, Hkv=1 << 15, G=1, total_q=1 << 22, **flat) == INVALID      # the block slots
    # the options
    for w in (-1, -64, -(1 << 31)):
        assert call(window=w) == INVALID, w
    for cap in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert call(softcap=cap) == INVALID, cap
    # the capacity: its rows of one (sequence, head), Ncap * d * 2 bytes, must fit 32 bits
    if paged:
        for ps in (0, -16, 8, 15, 24, 48, 100, (1 << 31) - 1):
            assert call(page_size=ps) == INVALID, ps
        for name in ("num_pages", "max_pages"):
            for v in (0, -1, -(1 << 31)):
                assert call(**{name: v}) == INVALID, (name, v)
        assert call(max_pages=1 << 27, page_size=16) == INVALID       # 2^31 keys: the capacity is an int
        assert call(max_pages=1 << 21, page_size=16) == INVALID       # 2^25 keys of 128 bytes: 2^32 bytes exactly
        assert call(max_pages=1 << 20, page_size=16, d=128, q_stride_t=512, q_stride_h=128, o_stride_t=512, o_stride_h=128) == INVALID
    else:
        for n in (0, -1, -(1 << 31)):
            assert call(Ncap=n) == INVALID, n
        assert call(Ncap=1 << 25) == INVALID                          # 2^25 keys of 128 bytes: 2^32 bytes exactly
        assert call(Ncap=1 << 24, d=128, q_stride_t=512, q_stride_h=128, o_stride_t=512, o_stride_h=128) == INVALID


def test_front_end_refusals(fa):
    torch = pytest.importorskip("torch")
    f16 = torch.float16
    q = torch.zeros(10, 4, 64, dtype=f16)
    kc = torch.zeros(2, 2, 64, 64, dtype=f16)
    pool = torch.zeros(9, 2, 16, 64, dtype=f16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    lens = torch.tensor([4, 40], dtype=torch.int32)
    table = torch.zeros(2, 4, dtype=torch.int32)
    f = fa.fa_forward_varlen_kvcache
    # with good arguments the call gets as far as the device checks, contiguous and paged
    with pytest.raises(ValueError, match="device tensor"):
        f(q, kc, kc, cu, lens)
    with pytest.raises(ValueError, match="device tensor"):
        f(q, pool, pool, cu, lens, block_table=table, causal=True, return_lse=True, window=4, softcap=30.0)
    with pytest.raises(ValueError, match="multiple of the number of K/V heads"):
        f(q, torch.zeros(2, 3, 64, 64, dtype=f16), torch.zeros(2, 3, 64, 64, dtype=f16), cu, lens)
    with pytest.raises(ValueError, match="contiguous in its last dimension"):
        f(torch.zeros(10, 4, 128, dtype=f16)[:, :, ::2], kc, kc, cu, lens)
    with pytest.raises(ValueError, match="int32"):
        f(q, kc, kc, cu.long(), lens)
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kc, kc, cu, lens.long())
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kc, kc, cu, lens[:1])
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kc, kc, cu, None)
    with pytest.raises(ValueError, match=r"B\+1 entries"):
        f(q, kc, kc, cu[:1], lens)
    with pytest.raises(ValueError, match="block_table"):
        f(q, pool, pool, cu, lens, block_table=table[:1])
    with pytest.raises(ValueError, match="block_table"):
        f(q, pool, pool, cu, lens, block_table=table.reshape(-1))
    with pytest.raises(ValueError, match="page_size"):
        f(q, torch.zeros(9, 2, 24, 64, dtype=f16), torch.zeros(9, 2, 24, 64, dtype=f16), cu, lens, block_table=table)
    with pytest.raises(ValueError, match="sequences"):
        f(q, torch.zeros(3, 2, 64, 64, dtype=f16), torch.zeros(3, 2, 64, 64, dtype=f16), cu, lens)
    for bad in (lambda: f(q[0], kc, kc, cu, lens),                                   # not (total, H, d)
                lambda: f(q, kc[0], kc[0], cu, lens),                                # not [B,Hkv,Ncap,d]
                lambda: f(q, kc.bfloat16(), kc, cu, lens),                           # mixed element types
                lambda: f(q.float(), kc.float(), kc.float(), cu, lens),
                lambda: f(q, kc, kc[:, :, :32], cu, lens),                           # K and V differ
                lambda: f(q[:, :, :32], kc[..., :32], kc[..., :32], cu, lens),       # d
                lambda: f(q, kc, kc, cu, lens, out_dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            bad()
    for w in (-1, 1.5, True, "4"):
        with pytest.raises(ValueError, match="window"):
            f(q, kc, kc, cu, lens, window=w)
    for cap in (-1.0, math.inf, math.nan, "1", None):
        with pytest.raises(ValueError, match="softcap"):
            f(q, kc, kc, cu, lens, softcap=cap)
    for bad, words in ((torch.zeros(4, dtype=f16), "float32"), (torch.zeros(3), "one value per query head"),
                       (torch.zeros(8)[::2], "contiguous"), ([0.0] * 4, "float32")):
        with pytest.raises(ValueError, match=words):
            f(q, kc, kc, cu, lens, sinks=bad)


def test_custom_op_registers(fa):
    """forward_varlen_kvcache exists after register(), traces on meta tensors, and the packed ops keep their schemas"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    op = torch.ops.fa_mi355.forward_varlen_kvcache
    q = torch.empty(515, 8, 128, dtype=torch.bfloat16, device="meta")
    pool = torch.empty(33, 2, 64, 128, dtype=torch.bfloat16, device="meta")
    cu = torch.empty(7, dtype=torch.int32, device="meta")
    lens = torch.empty(6, dtype=torch.int32, device="meta")
    table = torch.empty(6, 5, dtype=torch.int32, device="meta")
    sinks = torch.empty(8, dtype=torch.float32, device="meta")
    for f32, tbl, s in ((True, table, sinks), (False, None, None)):
        o, lse = op(q, pool, pool, cu, lens, tbl, 0.125, True, 4096, s, 50.0, f32)
        assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and o.device.type == "meta"
        assert lse.shape == (8, 515) and lse.dtype == torch.float32 and lse.device.type == "meta"
    assert [a.name for a in op.default._schema.arguments] == ["q", "k_cache", "v_cache", "cu_seqlens_q", "cache_seqlens", "block_table",
                                                              "scale", "causal", "window", "sinks", "softcap", "out_f32"]
    assert [a.name for a in torch.ops.fa_mi355.forward_varlen_ex.default._schema.arguments] == [
        "q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "scale", "causal", "window", "sinks", "softcap", "out_f32"]
    c = torch.zeros(4, 1, 64, dtype=torch.float16)
    kc = torch.zeros(1, 1, 16, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        op(c, kc, kc, torch.tensor([0, 4], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), None, 0.125, False, 2, None, 0.0, True)


def test_header_is_plain_c(tmp_path):
    """include/fa_mi355.h with the new structure still compiles as C99 on its own, and a descriptor can be filled in from C"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "fa_mi355.h"\nint main(void) { fa_varlen_kvcache_desc v = {0}; v.size = sizeof v; v.q_stride_t = 1; '
                   'v.causal = 1; v.out_dtype = FA_OUT_SAME; v.window = 128; return v.seqlens_k != 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "hdr.o")])
