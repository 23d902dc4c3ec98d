"""CPU tier of fa_forward_varlen: the symbol is exported, declared and bound; the ctypes structure mirrors the header's (names, size and
offsets, against the C compiler); every rejection holds before the device is touched; the front end is exported and refuses what it
must; the torch op traces on meta tensors.  Only calls that must be rejected are issued, with small made-up addresses, so the file is
safe where a GPU is visible."""
import ctypes
import os
import re
import subprocess

import pytest

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["size", "Q", "K", "V", "O", "lse", "cu_seqlens_q", "cu_seqlens_k", "B", "Hkv", "G", "d", "total_q", "total_k", "q_stride_t",
          "q_stride_h", "k_stride_t", "k_stride_h", "v_stride_t", "v_stride_h", "o_stride_t", "o_stride_h", "scale", "causal", "in_dtype",
          "out_dtype", "stream"]


def _header():
    return open(os.path.join(ROOT, "include", "fa_mi355.h")).read()


def _header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]


def test_symbol_and_struct(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    sym = fa.capi.SYMBOLS
    assert "fa_forward_varlen" in sym and hasattr(raw, "fa_forward_varlen")
    assert "fa_forward_varlen" not in sym[:9] and "fa_forward_varlen" not in sym[-2:]   # between the head slice and the pinned tail
    assert L.fa_forward_varlen.argtypes == [ctypes.POINTER(fa.capi.VarlenDesc)] and L.fa_forward_varlen.restype is ctypes.c_int
    assert "fa_forward_varlen" in fa.__all__ and callable(fa.fa_forward_varlen)
    header = _header()
    assert "int fa_forward_varlen(const fa_varlen_desc* desc);" in header
    assert _header_fields("fa_varlen_desc") == [f[0] for f in fa.capi.VarlenDesc._fields_] == FIELDS
    assert fa.capi.VarlenDesc().size == ctypes.sizeof(fa.capi.VarlenDesc)
    low = re.sub(r"\s+", " ", header.lower())
    for words in ("not part of this entry: a window, sinks, a soft-cap, fp8, a paged k/v, rotary, max_seqlen hints, dropout",
                  "nothing on the host reads cu_seqlens_*", "never an address outside [0, total) rows"):
        assert words in low, words


def test_descriptor_layout_matches_the_c_compiler(fa, tmp_path):
    src = tmp_path / "layout.c"
    prints = " ".join('printf("%%zu\\n", offsetof(fa_varlen_desc, %s));' % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fa_mi355.h"\nint main(void) { printf("%zu\\n", '
                   'sizeof(fa_varlen_desc)); ' + prints + ' return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = fa.capi.VarlenDesc
    assert got[0] == ctypes.sizeof(D) == 176
    assert got[1:] == [getattr(D, f).offset for f in FIELDS]
    assert (D.B.offset, D.q_stride_t.offset, D.scale.offset, D.stream.offset) == (64, 88, 152, 176 - 8)


def _desc(fa, **kw):
    """a descriptor with small made-up addresses that WOULD be launched: (300, 4, 64) queries on (300, 2, 64) keys"""
    f = dict(Q=4096, K=8192, V=12288, O=16384, lse=20480, cu_seqlens_q=32, cu_seqlens_k=64, B=2, Hkv=2, G=2, d=64, total_q=300,
             total_k=300, q_stride_t=256, q_stride_h=64, k_stride_t=128, k_stride_h=64, v_stride_t=128, v_stride_h=64, o_stride_t=256,
             o_stride_h=64, scale=0.125, causal=1, in_dtype=0, out_dtype=0)
    f.update(kw)
    return fa.capi.VarlenDesc(**f)


def _call(fa, **kw):
    return fa.lib().fa_forward_varlen(ctypes.byref(_desc(fa, **kw)))


def test_rejections_without_device(fa):
    L = fa.lib()
    assert L.fa_forward_varlen(None) == INVALID
    size = ctypes.sizeof(fa.capi.VarlenDesc)
    for bad in (0, 8, size - 8, size + 8, 1 << 20):
        assert _call(fa, size=bad) == INVALID, bad
    for name in ("Q", "K", "V", "O", "cu_seqlens_q", "cu_seqlens_k"):
        assert _call(fa, **{name: 0}) == INVALID, name
    for name in ("B", "Hkv", "G", "total_q", "total_k"):
        for v in (0, -1, -(1 << 31)):
            assert _call(fa, **{name: v}) == INVALID, (name, v)
    for d in (0, 32, 96, 256, -64):
        assert _call(fa, d=d, q_stride_t=1024, k_stride_t=1024, v_stride_t=1024, o_stride_t=1024) == INVALID, d
    for name in ("in_dtype", "out_dtype"):
        for v in (-1, 2, 99):
            assert _call(fa, **{name: v}) == INVALID, (name, v)
    for t in "qkvo":
        assert _call(fa, **{t + "_stride_t": 56}) == INVALID, t            # below d
        assert _call(fa, **{t + "_stride_t": 0}) == INVALID, t
        assert _call(fa, **{t + "_stride_t": -256}) == INVALID, t
        assert _call(fa, **{t + "_stride_h": -64}) == INVALID, t           # negative
        for s in ("_stride_t", "_stride_h"):                                # not a multiple of 8 elements
            for v in (260, 132, 68, 257):
                assert _call(fa, **{t + s: v}) == INVALID, (t, s, v)
    for name in ("Q", "K", "V", "O"):                                       # 16-byte loads and stores
        for off in (2, 4, 8):
            assert _call(fa, **{name: 4096 + off}) == INVALID, (name, off)
    # the last addressable byte, ((total-1)*stride_t + (H-1)*stride_h + d) * element bytes, must fit 32 bits
    assert _call(fa, total_k=1 << 25, Hkv=1, G=4, k_stride_t=64, k_stride_h=0) == INVALID                # 2^32 exactly
    assert _call(fa, total_k=1 << 25, Hkv=1, G=4, v_stride_t=64, v_stride_h=0) == INVALID
    assert _call(fa, total_q=1 << 23, out_dtype=1) == INVALID        # Q: (2^23 - 1) * 256 + 3 * 64 + 64 elements of 2 bytes = 2^32
    assert _call(fa, total_q=1 << 22) == INVALID                     # O alone, in fp32; the same shape in 16 bit fits
    assert _call(fa, total_q=1 << 24, Hkv=1, G=1, q_stride_t=64, q_stride_h=0, o_stride_t=64, o_stride_h=0) == INVALID   # O in fp32
    assert _call(fa, q_stride_h=1 << 30) == INVALID and _call(fa, k_stride_h=1 << 31) == INVALID         # the head term alone
    assert _call(fa, q_stride_t=1 << 62) == INVALID and _call(fa, o_stride_h=(1 << 63) - 8) == INVALID   # no overflow on the way
    # B * Hkv * G beyond the grid's range, however the product is spread
    for shape in (dict(B=1 << 16, Hkv=1 << 8, G=1 << 8), dict(B=1, Hkv=1 << 16, G=1 << 15), dict(B=(1 << 31) - 1, Hkv=2, G=1),
                  dict(B=(1 << 31) - 1, Hkv=(1 << 31) - 1, G=(1 << 31) - 1)):
        assert _call(fa, q_stride_h=0, k_stride_h=0, v_stride_h=0, o_stride_h=0, **shape) == INVALID, shape
    # ... and the block slots, floor(total_q / 128) + B per query head: (2^15 + 2^15) * 2^15 = 2^31
    flat = dict(q_stride_t=64, q_stride_h=0, k_stride_h=0, v_stride_h=0, o_stride_t=64, o_stride_h=0, out_dtype=1)
    assert _call(fa, B=1 << 15, Hkv=1 << 15, G=1, total_q=1 << 22, **flat) == INVALID


def test_front_end_refusals(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(10, 4, 64, dtype=torch.float16)
    k = torch.zeros(10, 2, 64, dtype=torch.float16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_varlen(q, k, k, cu)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_varlen(q, k, k, cu, cu, causal=True, return_lse=True)
    with pytest.raises(ValueError, match="multiple of the number of K/V heads"):
        fa.fa_forward_varlen(q, torch.zeros(10, 3, 64, dtype=torch.float16), torch.zeros(10, 3, 64, dtype=torch.float16), cu)
    wide = torch.zeros(10, 4, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="contiguous in its last dimension"):
        fa.fa_forward_varlen(wide[:, :, ::2], k, k, cu)
    with pytest.raises(ValueError, match="contiguous in its last dimension"):
        fa.fa_forward_varlen(q, k, torch.zeros(10, 64, 2, dtype=torch.float16).transpose(1, 2), cu)
    with pytest.raises(ValueError, match="int32"):
        fa.fa_forward_varlen(q, k, k, cu.long())
    with pytest.raises(ValueError, match="int32"):
        fa.fa_forward_varlen(q, k, k, cu, cu.long())
    with pytest.raises(ValueError, match=r"B\+1 entries"):
        fa.fa_forward_varlen(q, k, k, cu, cu[:2])
    with pytest.raises(ValueError, match=r"B\+1 entries"):
        fa.fa_forward_varlen(q, k, k, cu[:1])
    for bad in (lambda: fa.fa_forward_varlen(q[0], k, k, cu),                                  # not (total, H, d)
                lambda: fa.fa_forward_varlen(q, k.bfloat16(), k, cu),                         # mixed element types
                lambda: fa.fa_forward_varlen(q.float(), k.float(), k.float(), cu),
                lambda: fa.fa_forward_varlen(q, k, k[:9], cu),
                lambda: fa.fa_forward_varlen(q[:, :, :32], k[:, :, :32], k[:, :, :32], cu),   # d
                lambda: fa.fa_forward_varlen(q, k, k, cu, out_dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            bad()
    # a (H, total, d) tensor passed through .transpose(0, 1) is taken as it lies: it gets as far as the device check
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_varlen(torch.zeros(4, 10, 64, dtype=torch.float16).transpose(0, 1), k, k, cu)


def test_custom_op_registers(fa):
    """forward_varlen exists after register(), traces on meta tensors with the right shapes and dtypes, and has no CPU kernel"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    op = torch.ops.fa_mi355.forward_varlen
    q = torch.empty(515, 8, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(641, 2, 128, dtype=torch.bfloat16, device="meta")
    cu = torch.empty(7, dtype=torch.int32, device="meta")
    for f32, cuk in ((True, cu), (False, None)):
        o, lse = op(q, k, k, cu, cuk, 0.125, True, f32)
        assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and o.device.type == "meta"
        assert lse.shape == (8, 515) and lse.dtype == torch.float32 and lse.device.type == "meta"
    assert [a.name for a in op.default._schema.arguments] == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "scale", "causal", "out_f32"]
    c = torch.zeros(4, 1, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        op(c, c, c, torch.tensor([0, 4], dtype=torch.int32), None, 0.125, False, True)


def test_header_is_plain_c(tmp_path):
    """include/fa_mi355.h with the new structure still compiles as C99 on its own, and a descriptor can be filled in from C"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "fa_mi355.h"\nint main(void) { fa_varlen_desc v = {0}; v.size = sizeof v; v.q_stride_t = 1; v.causal = 1; '
                   'v.out_dtype = FA_OUT_SAME; return v.cu_seqlens_k != 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "hdr.o")])
