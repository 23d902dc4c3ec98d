"""CPU tier of fa_forward_varlen_kvcache_fp8 (the varlen prefill against an fp8 KV cache): the symbol is exported, declared and bound;
the rejection list of tests/test_varlen_cache_host.py holds for the new entry before the device is touched, with null and non-null
scales; the front end is exported and refuses what it must -- a cache that is not e4m3fn first -- while fa_forward_varlen_kvcache keeps
refusing an fp8 cache; the torch op traces on meta tensors and the older ops keep their argument names.  Only calls that must be
rejected are issued, with small made-up addresses, so the file is safe where a GPU is visible."""
import ctypes
import math
import os
import re
import subprocess

import pytest

import test_varlen_cache_host as th
from test_varlen_host import INVALID, ROOT, _header

NAME = "fa_forward_varlen_kvcache_fp8"
SCALES = {"null": (None, None), "both": (512, 768), "k": (512, None), "v": (None, 768)}


def test_symbol_signature_and_declaration(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    assert NAME in fa.capi.SYMBOLS and hasattr(raw, NAME)
    assert NAME not in fa.capi.SYMBOLS[:9] and NAME not in fa.capi.SYMBOLS[-2:]
    fn = getattr(L, NAME)
    assert fn.argtypes == [ctypes.POINTER(fa.capi.VarlenKvcacheDesc), ctypes.c_void_p, ctypes.c_void_p] and fn.restype is ctypes.c_int
    assert NAME in fa.__all__ and callable(getattr(fa, NAME))
    header = _header()
    assert "int fa_forward_varlen_kvcache_fp8(const fa_varlen_kvcache_desc* desc, const float* k_scale, const float* v_scale);" in header
    # the descriptor did not move, and the 16-bit entry's comment points at the new entry
    assert th._header_fields("fa_varlen_kvcache_desc") == th.FIELDS
    low = re.sub(r"\s+", " ", header.lower())
    for words in ("not part of this entry: fp8 caches; split-kv for a short chunk", "fa_forward_varlen_kvcache_fp8, below",
                  "one ocp e4m3fn byte per element", "clamped to +-flt_min after the product with k_scale", "the sinks take neither scale",
                  "raw bytes are zeroed", "the capacity bound stays ncap*d*2 bytes in 32 bits", "the window clamp",
                  "per-token or per-page scales; an fp8 q or fp8 mfmas; rotary"):
        assert words in low, words


@pytest.mark.parametrize("scales", sorted(SCALES))
@pytest.mark.parametrize("opts", sorted(th.OPTS))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_rejections_without_device(fa, monkeypatch, paged, opts, scales):
    """tests/test_varlen_cache_host.py's list, as it is, with its one call pointed at the new entry"""
    ks, vs = SCALES[scales]
    fn = getattr(fa.lib(), NAME)
    assert fn(None, ks, vs) == INVALID
    calls = []

    def call(fa_, paged_, **kw):
        calls.append(kw)
        return fn(ctypes.byref(th._desc(fa_, paged_, **kw)), ks, vs)

    monkeypatch.setattr(th, "_call", call)
    th.test_rejections_without_device(fa, paged, opts)
    assert len(calls) > 50                      # the list did go through `call`


def test_front_end_refusals(fa):
    torch = pytest.importorskip("torch")
    f16, e4 = torch.float16, torch.float8_e4m3fn
    q = torch.zeros(10, 4, 64, dtype=f16)
    kc = torch.zeros(2, 2, 64, 64, dtype=f16).to(e4)
    pool = torch.zeros(9, 2, 16, 64, dtype=f16).to(e4)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    lens = torch.tensor([4, 40], dtype=torch.int32)
    table = torch.zeros(2, 4, dtype=torch.int32)
    ones = torch.ones(2)
    f = getattr(fa, NAME)
    # with good arguments the call gets as far as the device checks, contiguous and paged, with and without scales
    with pytest.raises(ValueError, match="device tensor"):
        f(q, kc, kc, cu, lens)
    with pytest.raises(ValueError, match="device tensor"):
        f(q, pool, pool, cu, lens, block_table=table, k_scale=ones, v_scale=ones, causal=True, return_lse=True, window=4, softcap=30.0)
    # the cache format is judged first: before q, the table, the scales and anything that needs a device
    for bad in (torch.float16, torch.bfloat16, torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float32, torch.uint8):
        other = torch.zeros(2, 2, 64, 64, dtype=f16).to(bad)
        for k, v in ((other, kc), (kc, other), (other, other)):
            with pytest.raises(ValueError, match="an fp8 cache must be torch.float8_e4m3fn"):
                f(q.float(), k, v, cu.long(), None, block_table="no table", k_scale="no scale")
    with pytest.raises(ValueError, match="fp16 or bf16"):
        f(q.float(), kc, kc, cu, lens)
    # the scales go through the decode front end's check
    for name in ("k_scale", "v_scale"):
        for bad in (torch.ones(2, dtype=f16), torch.ones(2, dtype=torch.float64), torch.ones(3), torch.ones(1), torch.ones(2, 1), [1.0, 1.0], 1.0):
            with pytest.raises(ValueError, match=name + " must be a float32 device tensor"):
                f(q, kc, kc, cu, lens, **{name: bad})
        with pytest.raises(ValueError, match=name + " must be a device tensor"):   # a host tensor
            f(q, kc, kc, cu, lens, **{name: ones})
    # everything the 16-bit front end refuses
    z = lambda *shape: torch.zeros(*shape, dtype=f16).to(e4)   # noqa: E731
    with pytest.raises(ValueError, match="multiple of the number of K/V heads"):
        f(q, z(2, 3, 64, 64), z(2, 3, 64, 64), cu, lens)
    with pytest.raises(ValueError, match="contiguous in its last dimension"):
        f(torch.zeros(10, 4, 128, dtype=f16)[:, :, ::2], kc, kc, cu, lens)
    with pytest.raises(ValueError, match="int32"):
        f(q, kc, kc, cu.long(), lens)
    for bad in (lens.long(), lens[:1], None):
        with pytest.raises(ValueError, match="cache_seqlens"):
            f(q, kc, kc, cu, bad)
    with pytest.raises(ValueError, match=r"B\+1 entries"):
        f(q, kc, kc, cu[:1], lens)
    for bad in (table[:1], table.reshape(-1)):
        with pytest.raises(ValueError, match="block_table"):
            f(q, pool, pool, cu, lens, block_table=bad)
    with pytest.raises(ValueError, match="page_size"):
        f(q, z(9, 2, 24, 64), z(9, 2, 24, 64), cu, lens, block_table=table)
    with pytest.raises(ValueError, match="sequences"):
        f(q, z(3, 2, 64, 64), z(3, 2, 64, 64), cu, lens)
    for bad in (lambda: f(q[0], kc, kc, cu, lens),                                   # not (total, H, d)
                lambda: f(q, kc[0], kc[0], cu, lens),                                # not [B,Hkv,Ncap,d]
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


def test_the_16_bit_front_end_still_refuses_an_fp8_cache(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(10, 4, 64, dtype=torch.float16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    lens = torch.tensor([4, 40], dtype=torch.int32)
    for dt in (torch.float8_e4m3fn, torch.float8_e5m2):
        kc = torch.zeros(2, 2, 64, 64, dtype=torch.float16).to(dt)
        with pytest.raises(ValueError, match="must all be fp16 or all bf16"):
            fa.fa_forward_varlen_kvcache(q, kc, kc, cu, lens)
    assert "k_scale" not in fa.fa_forward_varlen_kvcache.__code__.co_varnames


def test_custom_op_registers(fa):
    """forward_varlen_kvcache_fp8 exists after register(), traces on meta tensors, and the older ops keep their argument names"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    op = torch.ops.fa_mi355.forward_varlen_kvcache_fp8
    q = torch.empty(515, 8, 128, dtype=torch.bfloat16, device="meta")
    pool = torch.empty(33, 2, 64, 128, dtype=torch.float8_e4m3fn, device="meta")
    cu = torch.empty(7, dtype=torch.int32, device="meta")
    lens = torch.empty(6, dtype=torch.int32, device="meta")
    table = torch.empty(6, 5, dtype=torch.int32, device="meta")
    sinks = torch.empty(8, dtype=torch.float32, device="meta")
    sc = torch.empty(2, dtype=torch.float32, device="meta")
    for f32, tbl, s, k_s, v_s in ((True, table, sinks, sc, sc), (False, None, None, None, None), (False, table, None, sc, None)):
        o, lse = op(q, pool, pool, cu, lens, tbl, k_s, v_s, 0.125, True, 4096, s, 50.0, f32)
        assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and o.device.type == "meta"
        assert lse.shape == (8, 515) and lse.dtype == torch.float32 and lse.device.type == "meta"
    names = lambda o: [a.name for a in o.default._schema.arguments]   # noqa: E731
    tail = ["scale", "causal", "window", "sinks", "softcap", "out_f32"]
    lead = ["q", "k_cache", "v_cache", "cu_seqlens_q", "cache_seqlens", "block_table"]
    assert names(op) == lead + ["k_scale", "v_scale"] + tail
    assert [str(a.type) for a in op.default._schema.arguments][5:8] == ["Optional[Tensor]"] * 3
    assert names(torch.ops.fa_mi355.forward_varlen_kvcache) == lead + tail
    assert names(torch.ops.fa_mi355.forward_varlen_ex) == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k"] + tail
    assert names(torch.ops.fa_mi355.forward_varlen) == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "scale", "causal", "out_f32"]
    assert names(torch.ops.fa_mi355.decode_paged_fp8_ex) == ["q", "k_pool", "v_pool", "block_table", "k_scale", "v_scale", "cache_seqlens",
                                                            "scale", "causal", "window", "sinks", "softcap", "out_fp32"]
    c = torch.zeros(4, 1, 64, dtype=torch.float16)
    kc = torch.zeros(1, 1, 16, 64, dtype=torch.float16).to(torch.float8_e4m3fn)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        op(c, kc, kc, torch.tensor([0, 4], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), None, None, None, 0.125, False, 2, None,
           0.0, True)


def test_header_is_plain_c(tmp_path):
    """include/fa_mi355.h with the new declaration still compiles as C99 on its own, and the entry can be named from C"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "fa_mi355.h"\nint main(void) { fa_varlen_kvcache_desc v = {0}; '
                   'int (*f)(const fa_varlen_kvcache_desc*, const float*, const float*) = fa_forward_varlen_kvcache_fp8; '
                   'v.size = sizeof v; return f == 0 && v.seqlens_k != 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "hdr.o")])
