"""CPU tier of fa_forward_varlen_ex (the packed prefill with a window, a soft-cap and sinks): the symbol is exported, declared and
bound; capi.VarlenOpts mirrors the header's structure (names, offsets and size, against the C compiler); every rejection holds before
the device is touched, with and without options; the front end refuses what it must; the torch op traces on meta tensors.  Only calls
that must be rejected are issued, with small made-up addresses, so the file is safe where a GPU is visible."""
import ctypes
import math
import os
import subprocess

import pytest

from test_varlen_host import INVALID, ROOT, _desc, _header, _header_fields

FIELDS = ["size", "sinks", "window", "softcap"]


def test_symbol_and_struct(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    assert "fa_forward_varlen_ex" in fa.capi.SYMBOLS and hasattr(raw, "fa_forward_varlen_ex")
    assert L.fa_forward_varlen_ex.argtypes == [ctypes.POINTER(fa.capi.VarlenDesc), ctypes.POINTER(fa.capi.VarlenOpts)]
    assert L.fa_forward_varlen_ex.restype is ctypes.c_int
    header = _header()
    assert "int fa_forward_varlen_ex(const fa_varlen_desc* desc, const fa_varlen_opts* opts);" in header
    assert _header_fields("fa_varlen_opts") == [f[0] for f in fa.capi.VarlenOpts._fields_] == FIELDS
    assert fa.capi.VarlenOpts().size == ctypes.sizeof(fa.capi.VarlenOpts)
    o = fa.capi.VarlenOpts(window=5)
    assert (o.sinks, o.window, o.softcap) == (None, 5, 0.0)


def test_opts_layout_matches_the_c_compiler(fa, tmp_path):
    src = tmp_path / "layout.c"
    prints = " ".join('printf("%%zu\\n", offsetof(fa_varlen_opts, %s));' % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fa_mi355.h"\nint main(void) { fa_varlen_opts o = {0}; o.size = '
                   'sizeof o; o.window = 4096; o.softcap = 50.0f; printf("%zu\\n", sizeof(fa_varlen_opts)); ' + prints +
                   ' return o.sinks != 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = fa.capi.VarlenOpts
    assert got[0] == ctypes.sizeof(D) == 24
    assert got[1:] == [getattr(D, f).offset for f in FIELDS] == [0, 8, 16, 20]
    assert ctypes.sizeof(fa.capi.VarlenDesc) == 176          # the descriptor did not grow


def _call(fa, opts, **kw):
    return fa.lib().fa_forward_varlen_ex(ctypes.byref(_desc(fa, **kw)), None if opts is None else ctypes.byref(opts))


def test_option_rejections_without_device(fa):
    O = fa.capi.VarlenOpts
    size = ctypes.sizeof(O)
    for bad in (0, 8, size - 8, size + 8, 1 << 20):
        assert _call(fa, O(size=bad, window=4)) == INVALID, bad
        assert _call(fa, O(size=bad)) == INVALID, bad          # ... also with every option off
    for w in (-1, -64, -(1 << 31)):
        assert _call(fa, O(window=w)) == INVALID, w
        assert _call(fa, O(window=w, softcap=1.0, sinks=256)) == INVALID, w
    for cap in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), -float("inf")):
        assert _call(fa, O(softcap=cap)) == INVALID, cap
        assert _call(fa, O(softcap=cap, window=4)) == INVALID, cap


@pytest.mark.parametrize("opts", ("null", "off", "window", "softcap", "sinks", "all"))
def test_base_rejections_hold_under_every_opts(fa, opts):
    """a null opts and an all-off opts reach fa_forward_varlen's checks, and so does a call with options: everything that entry
    refuses is refused here, before the device is touched"""
    O = fa.capi.VarlenOpts
    o = {"null": None, "off": O(), "window": O(window=17), "softcap": O(softcap=30.0), "sinks": O(sinks=256),
         "all": O(window=1, softcap=0.5, sinks=256)}[opts]
    L = fa.lib()
    assert L.fa_forward_varlen_ex(None, None if o is None else ctypes.byref(o)) == INVALID
    size = ctypes.sizeof(fa.capi.VarlenDesc)
    for bad in (0, size - 8, size + 8):
        assert _call(fa, o, size=bad) == INVALID, bad
    for name in ("Q", "K", "V", "O", "cu_seqlens_q", "cu_seqlens_k"):
        assert _call(fa, o, **{name: 0}) == INVALID, name
    for name in ("B", "Hkv", "G", "total_q", "total_k"):
        for v in (0, -1):
            assert _call(fa, o, **{name: v}) == INVALID, (name, v)
    for d in (0, 32, 96, 256):
        assert _call(fa, o, d=d, q_stride_t=1024, k_stride_t=1024, v_stride_t=1024, o_stride_t=1024) == INVALID, d
    for name in ("in_dtype", "out_dtype"):
        assert _call(fa, o, **{name: 2}) == INVALID, name
    for t in "qkvo":
        assert _call(fa, o, **{t + "_stride_t": 56}) == INVALID, t
        assert _call(fa, o, **{t + "_stride_h": -64}) == INVALID, t
        assert _call(fa, o, **{t + "_stride_t": 260}) == INVALID, t
    for name in ("Q", "K", "V", "O"):
        assert _call(fa, o, **{name: 4096 + 8}) == INVALID, name
    assert _call(fa, o, total_k=1 << 25, Hkv=1, G=4, k_stride_t=64, k_stride_h=0) == INVALID      # the last byte at 2^32
    assert _call(fa, o, total_q=1 << 22) == INVALID                                               # O alone, in fp32
    assert _call(fa, o, B=(1 << 31) - 1, Hkv=2, G=1, q_stride_h=0, k_stride_h=0, v_stride_h=0, o_stride_h=0) == INVALID
    flat = dict(q_stride_t=64, q_stride_h=0, k_stride_h=0, v_stride_h=0, o_stride_t=64, o_stride_h=0, out_dtype=1)
    assert _call(fa, o, B=1 << 15, Hkv=1 << 15, G=1, total_q=1 << 22, **flat) == INVALID          # the block slots


def test_front_end_refusals(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(10, 4, 64, dtype=torch.float16)
    k = torch.zeros(10, 2, 64, dtype=torch.float16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    for w in (-1, 1.5, True, "4"):
        with pytest.raises(ValueError, match="window"):
            fa.fa_forward_varlen(q, k, k, cu, window=w)
    for cap in (-1.0, math.inf, math.nan, "1", None):
        with pytest.raises(ValueError, match="softcap"):
            fa.fa_forward_varlen(q, k, k, cu, softcap=cap)
    for bad, words in ((torch.zeros(4, dtype=torch.float16), "float32"), (torch.zeros(3), "one value per query head"),
                       (torch.zeros(8)[::2], "contiguous"), ([0.0] * 4, "float32")):
        with pytest.raises(ValueError, match=words):
            fa.fa_forward_varlen(q, k, k, cu, sinks=bad)
    # with good options the call gets as far as the device checks: the base refusals come first
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_forward_varlen(q, k, k, cu, window=4, softcap=30.0)
    with pytest.raises(ValueError, match="int32"):
        fa.fa_forward_varlen(q, k, k, cu.long(), window=4)


def test_custom_op_registers(fa):
    """forward_varlen_ex exists after register(), traces on meta tensors, and forward_varlen keeps its schema"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    op = torch.ops.fa_mi355.forward_varlen_ex
    q = torch.empty(515, 8, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(641, 2, 128, dtype=torch.bfloat16, device="meta")
    cu = torch.empty(7, dtype=torch.int32, device="meta")
    sinks = torch.empty(8, dtype=torch.float32, device="meta")
    for f32, cuk, s in ((True, cu, sinks), (False, None, None)):
        o, lse = op(q, k, k, cu, cuk, 0.125, True, 4096, s, 50.0, f32)
        assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and o.device.type == "meta"
        assert lse.shape == (8, 515) and lse.dtype == torch.float32 and lse.device.type == "meta"
    assert [a.name for a in op.default._schema.arguments] == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "scale", "causal", "window",
                                                              "sinks", "softcap", "out_f32"]
    assert [a.name for a in torch.ops.fa_mi355.forward_varlen.default._schema.arguments] == [
        "q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "scale", "causal", "out_f32"]
    c = torch.zeros(4, 1, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        op(c, c, c, torch.tensor([0, 4], dtype=torch.int32), None, 0.125, False, 2, None, 0.0, True)
