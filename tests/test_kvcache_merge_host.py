"""CPU tier of fa_merge_states and fa_forward_kvcache_shared_prefix: the symbol is exported, declared and bound; the two ctypes
structures mirror the header; every rejection holds before the device is touched; the front ends are exported and refuse CPU
tensors; both torch ops trace on meta tensors; the header is still C99.  Only calls that must be rejected are issued, with small
made-up addresses, so the file is safe where a GPU is visible."""
import ctypes
import os
import re
import subprocess

import pytest

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fa_mi355.h")).read()


def _header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*", "", n.strip().lstrip("*").strip().split(" ")[-1].lstrip("*")) for n in decl.split(",")]
    return names


def test_symbol_and_structs(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    assert "fa_merge_states" in fa.capi.SYMBOLS and hasattr(raw, "fa_merge_states")
    assert "fa_merge_states" not in fa.capi.SYMBOLS[:9] and "fa_merge_states" not in fa.capi.SYMBOLS[-2:]
    assert L.fa_merge_states.argtypes == [ctypes.POINTER(fa.capi.MergeDesc)] and L.fa_merge_states.restype is ctypes.c_int
    header = _header()
    assert "int fa_merge_states(const fa_merge_desc* desc);" in header
    for line in ("#define FA_MERGE_MAX_PARTS 16", "#define FA_STATE_F16  0", "#define FA_STATE_BF16 1", "#define FA_STATE_F32  2"):
        assert line in header, line
    assert (fa.capi.MERGE_MAX_PARTS, fa.capi.STATE_F16, fa.capi.STATE_BF16, fa.capi.STATE_F32) == (16, 0, 1, 2)
    part, desc = _header_fields("fa_state_part"), _header_fields("fa_merge_desc")
    assert part == [f[0] for f in fa.capi.StatePart._fields_] == ["O", "lse", "stride_b", "stride_h"]
    assert desc == [f[0] for f in fa.capi.MergeDesc._fields_] == ["size", "parts", "R", "B", "H", "rows", "d", "part_dtype", "O", "lse",
                                                                   "out_dtype", "stream"]
    # the parts are the kernel's 512 bytes of arguments; the descriptor's layout is the C compiler's
    assert ctypes.sizeof(fa.capi.StatePart) == 32 and ctypes.sizeof(fa.capi.StatePart) * fa.capi.MERGE_MAX_PARTS == 512
    assert fa.capi.MergeDesc.parts.offset == 8 and fa.capi.MergeDesc.R.offset == 520 and fa.capi.MergeDesc.O.offset == 544
    assert fa.capi.MergeDesc().size == ctypes.sizeof(fa.capi.MergeDesc) == fa.capi.MergeDesc.stream.offset + 8 == 576
    d = fa.capi.MergeDesc(parts=[(16, 32, 5, 7), fa.capi.StatePart(48, 64, 1, 2)], R=2)
    assert (d.parts[0].O, d.parts[0].lse, d.parts[0].stride_b, d.parts[0].stride_h) == (16, 32, 5, 7)
    assert (d.parts[1].O, d.parts[1].stride_h, d.parts[2].O) == (48, 2, None)
    low = header.lower()
    assert "not part of this entry: parts of different element types" in low and "a window or seqlens_q cannot be composed" in low


def test_descriptor_size_matches_the_c_compiler(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fa_mi355.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(fa_state_part), sizeof(fa_merge_desc), offsetof(fa_merge_desc, O), offsetof(fa_merge_desc, stream)); '
                   'return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "576", "544", "568"]


def _desc(fa, R=2, parts=None, **kw):
    """a descriptor with small made-up addresses that WOULD be launched"""
    f = dict(B=2, H=2, rows=6, d=64, part_dtype=fa.capi.STATE_F32, O=4096, lse=8192, out_dtype=fa.capi.STATE_F32)
    f.update(kw)
    if parts is None:
        parts = [(65536 * (i + 1), 65536 * (i + 1) + 32768, 12, 6) for i in range(max(min(R, 16), 0))]
    return fa.capi.MergeDesc(parts=parts, R=R, **f)


def _call(fa, **kw):
    return fa.lib().fa_merge_states(ctypes.byref(_desc(fa, **kw)))


def test_rejections_without_device(fa):
    L = fa.lib()
    assert L.fa_merge_states(None) == INVALID
    size = ctypes.sizeof(fa.capi.MergeDesc)
    for bad in (0, 8, 512, size - 8, size + 8):
        assert _call(fa, size=bad) == INVALID, bad
    for R in (0, -1, 17, 1 << 20):
        assert _call(fa, R=R) == INVALID, R
    assert _call(fa, O=0) == INVALID
    good = [(65536, 98304, 12, 6), (131072, 163840, 12, 6), (196608, 229376, 12, 6)]
    for i in range(3):                                  # a null O or lse in any of the first R parts
        for field in (0, 1):
            parts = [tuple(0 if (j == i and k == field) else v for k, v in enumerate(p)) for j, p in enumerate(good)]
            assert _call(fa, R=3, parts=parts) == INVALID, (i, field)
    for i in range(3):                                  # a negative stride
        for field in (2, 3):
            parts = [tuple(-1 if (j == i and k == field) else v for k, v in enumerate(p)) for j, p in enumerate(good)]
            assert _call(fa, R=3, parts=parts) == INVALID, (i, field)
    for name in ("B", "H", "rows"):
        for v in (0, -1):
            assert _call(fa, **{name: v}) == INVALID, (name, v)
    for d in (0, 32, 96, 256, -64):
        assert _call(fa, d=d) == INVALID, d
    for name in ("part_dtype", "out_dtype"):
        for v in (-1, 3, 99):
            assert _call(fa, **{name: v}) == INVALID, (name, v)
    # B * H * rows beyond the grid's range (one wave per row), however the product is spread
    for shape in (dict(B=1 << 26, H=1, rows=1), dict(B=1 << 13, H=1 << 13, rows=1), dict(B=1 << 10, H=1 << 10, rows=1 << 10),
                  dict(B=(1 << 31) - 1, H=(1 << 31) - 1, rows=(1 << 31) - 1)):
        assert _call(fa, **shape) == INVALID, shape
    # rows of four elements are loaded and stored whole: the alignment they need
    assert _call(fa, O=4096 + 8) == INVALID and _call(fa, O=4096 + 4, out_dtype=fa.capi.STATE_F16) == INVALID
    assert _call(fa, R=1, parts=[(65536 + 8, 98304, 12, 6)]) == INVALID
    assert _call(fa, R=1, parts=[(65536 + 4, 98304, 12, 6)], part_dtype=fa.capi.STATE_BF16) == INVALID


def test_exported_and_refuse_cpu_tensors(fa):
    torch = pytest.importorskip("torch")
    for n in ("fa_merge_states", "fa_forward_kvcache_shared_prefix"):
        assert n in fa.__all__ and callable(getattr(fa, n)), n
    o = torch.zeros(2, 4, 3, 64)
    l = torch.zeros(2, 4, 3)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_merge_states([o, o], [l, l])
    for outs, lses, kw in (([], [], {}), ([o] * 17, [l] * 17, {}), ([o, o], [l], {}), ([o, o.half()], [l, l], {}),
                           ([o, o[:1]], [l, l], {}), ([o], [l[:1]], {}), ([o], [l], dict(out_dtype=torch.float64)),
                           ([o.double()], [l], {}), ([o[0]], [l[0]], {})):
        with pytest.raises(ValueError):
            fa.fa_merge_states(outs, lses, **kw)
    q = torch.zeros(3, 8, 1, 64, dtype=torch.float16)
    kp = torch.zeros(1, 2, 200, 64, dtype=torch.float16)
    kc = torch.zeros(3, 2, 192, 64, dtype=torch.float16)
    pool = torch.zeros(40, 2, 16, 64, dtype=torch.float16)
    table = torch.zeros(3, 12, dtype=torch.int32)
    n1 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_kvcache_shared_prefix(q, kp, kp, kc, kc)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_kvcache_shared_prefix(q, kp, kp, pool, pool, prefix_len=n1, block_table=table, causal=True, softcap=1.0)
    f8 = torch.float8_e4m3fn
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_kvcache_shared_prefix(q, kp.to(f8), kp.to(f8), kc.to(f8), kc.to(f8), k_scale=torch.ones(2), v_scale=torch.ones(2))
    for bad in (lambda: fa.fa_forward_kvcache_shared_prefix(q, kc, kc, kc, kc),                    # a prefix per sequence
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp[:, :1], kp[:, :1], kc, kc),     # other K/V heads
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp.bfloat16(), kp.bfloat16(), kc, kc),
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp.to(f8), kp.to(f8), kc, kc),      # another element type than the suffix
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp, kp, kc, kc, k_scale=torch.ones(2)),
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp, kp, kc, kc, prefix_len=torch.zeros(3, dtype=torch.int32)),
                lambda: fa.fa_forward_kvcache_shared_prefix(q[:, :7], kp, kp, kc, kc),
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp, kp, kc, kc, out_dtype=torch.bfloat16),
                lambda: fa.fa_forward_kvcache_shared_prefix(q, kp, kp, kc, kc, stream=0)):
        with pytest.raises(ValueError):
            bad()
    for kw in (dict(window=5), dict(seqlens_q=n1)):      # not keywords of this function
        with pytest.raises(TypeError):
            fa.fa_forward_kvcache_shared_prefix(q, kp, kp, kc, kc, **kw)
    doc = fa.fa_forward_kvcache_shared_prefix.__doc__
    assert "`window` and `seqlens_q` are NOT keywords" in doc


def test_custom_ops_register(fa):
    """merge_states and decode_shared_prefix exist after register(), trace on meta tensors and have no CPU kernel"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    outs = torch.empty(3, 2, 8, 3, 128, dtype=torch.bfloat16, device="meta")
    lses = torch.empty(3, 2, 8, 3, dtype=torch.float32, device="meta")
    for f32 in (True, False):
        o, lse = ops.merge_states(outs, lses, f32)
        assert o.shape == outs.shape[1:] and o.dtype == (torch.float32 if f32 else torch.bfloat16) and o.device.type == "meta"
        assert lse.shape == lses.shape[1:] and lse.dtype == torch.float32
    q = torch.empty(2, 8, 3, 128, dtype=torch.bfloat16, device="meta")
    kp = torch.empty(1, 2, 700, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(2, 2, 500, 128, dtype=torch.bfloat16, device="meta")
    one = torch.empty(1, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    sinks = torch.empty(8, dtype=torch.float32, device="meta")
    for pl, cl, s, f32 in ((one, lens, sinks, True), (None, None, None, False)):
        o = ops.decode_shared_prefix(q, kp, kp, k, k, pl, cl, 0.125, True, s, 1.0, f32)
        assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and o.device.type == "meta"
    args = [(a.name, str(a.type)) for a in ops.decode_shared_prefix.default._schema.arguments]
    assert [n for n, _ in args] == ["q", "k_prefix", "v_prefix", "k_cache", "v_cache", "prefix_len", "cache_seqlens", "scale", "causal",
                                    "sinks", "softcap", "out_fp32"]
    assert str(ops.merge_states.default._schema).endswith("(Tensor outs, Tensor lses, bool out_f32) -> (Tensor, Tensor)")
    c = torch.zeros(1, 1, 1, 1, 64)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.merge_states(c, c[..., 0], True)
    h = torch.zeros(1, 1, 64, 64, dtype=torch.float16)
    with pytest.raises(Exception):
        ops.decode_shared_prefix(h, h, h, h, h, None, None, 0.125, False, None, 0.0, True)


def test_header_is_plain_c(tmp_path):
    """include/fa_mi355.h with the two new structures still compiles as C99 on its own, and a descriptor can be filled in from C"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "fa_mi355.h"\nint main(void) { fa_merge_desc m = {0}; m.size = sizeof m; m.R = FA_MERGE_MAX_PARTS; '
                   'm.parts[15].stride_b = 1; m.part_dtype = FA_STATE_F32; return m.parts[0].O != 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "hdr.o")])
