"""CPU tier of the tree step's two entries, through the C ABI: fa_kvcache_decode_varlen_ex (a tree mask on the packed decode) and
fa_kvcache_append_varlen_ex (rotary positions on the packed append).  The symbols are exported, declared and bound, both option
structures mirror the header under the C compiler, every refusal holds before the device is touched, and null options fall through
to exactly what the plain entries refuse.  Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os
import subprocess

import pytest

import test_kvcache_append_varlen_host as appendv
import test_kvcache_decode_varlen_host as decodev
import test_kvcache_logits_host as logits

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fa_kvcache_decode_varlen_ex", "fa_kvcache_append_varlen_ex")
MASK, POS = 1 << 12, 1 << 13   # made-up device addresses with the alignment the entries ask for


def _tree(fa, kind="", mask=MASK, opts_size=None, **kw):
    """the packed decode's good descriptor, causal, with a mask; `mask` None: options without a mask"""
    o = fa.capi.KvDecodeTreeOpts(tree_mask=mask)
    if opts_size is not None:
        o.size = opts_size
    return fa.lib().fa_kvcache_decode_varlen_ex(ctypes.byref(decodev._desc(fa, kind, **dict(dict(causal=1), **kw))), ctypes.byref(o))


def _pos(fa, kind="rope", pos=POS, opts_size=None, **kw):
    o = fa.capi.KvAppendVarlenOpts(positions=pos)
    if opts_size is not None:
        o.size = opts_size
    return fa.lib().fa_kvcache_append_varlen_ex(ctypes.byref(appendv._desc(fa, kind, **kw)), ctypes.byref(o))


def test_symbols_structs_and_declarations(fa):
    raw, L = ctypes.CDLL(fa.capi.LIB_PATH), fa.lib()
    for n in NAMES:
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
        assert n not in fa.capi.SYMBOLS[:9] and n not in fa.capi.SYMBOLS[-2:], n
    T, P = fa.capi.KvDecodeTreeOpts, fa.capi.KvAppendVarlenOpts
    assert L.fa_kvcache_decode_varlen_ex.argtypes == [ctypes.POINTER(fa.capi.KvDecodeVarlenDesc), ctypes.POINTER(T)]
    assert L.fa_kvcache_append_varlen_ex.argtypes == [ctypes.POINTER(fa.capi.KvAppendVarlenDesc), ctypes.POINTER(P)]
    assert L.fa_kvcache_decode_varlen_ex.restype is ctypes.c_int and L.fa_kvcache_append_varlen_ex.restype is ctypes.c_int
    assert appendv._header_fields("fa_kvdecode_tree_opts") == [f[0] for f in T._fields_] == ["size", "tree_mask"]
    assert appendv._header_fields("fa_kvappend_varlen_opts") == [f[0] for f in P._fields_] == ["size", "positions"]
    for S in (T, P):
        assert S().size == ctypes.sizeof(S) == fa.capi.new_desc(S).size
    header = appendv._header()
    for decl in ("int fa_kvcache_decode_varlen_ex(const fa_kvdecode_varlen_desc* desc, const fa_kvdecode_tree_opts* opts);",
                 "int fa_kvcache_append_varlen_ex(const fa_kvappend_varlen_desc* desc, const fa_kvappend_varlen_opts* opts);"):
        assert decl in header
    assert header.count("Not part of this entry") >= 2 and "per-head masks" in header and "per-sequence position offset" in header
    assert callable(fa.tree_from_parents) and "tree_from_parents" in fa.__all__


def test_option_layouts_match_the_c_compiler(fa, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fa_mi355.h"\nint main(void) { '
                   'printf("%zu %zu %zu\\n", sizeof(fa_kvdecode_tree_opts), offsetof(fa_kvdecode_tree_opts, size), '
                   'offsetof(fa_kvdecode_tree_opts, tree_mask)); '
                   'printf("%zu %zu %zu\\n", sizeof(fa_kvappend_varlen_opts), offsetof(fa_kvappend_varlen_opts, size), '
                   'offsetof(fa_kvappend_varlen_opts, positions)); '
                   'printf("%zu %zu\\n", sizeof(fa_kvdecode_varlen_desc), sizeof(fa_kvappend_varlen_desc)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    T, P = fa.capi.KvDecodeTreeOpts, fa.capi.KvAppendVarlenOpts
    assert got[:3] == [ctypes.sizeof(T), T.size.offset, T.tree_mask.offset] == [16, 0, 8]
    assert got[3:6] == [ctypes.sizeof(P), P.size.offset, P.positions.offset] == [16, 0, 8]
    assert got[6:] == [ctypes.sizeof(fa.capi.KvDecodeVarlenDesc), ctypes.sizeof(fa.capi.KvAppendVarlenDesc)]   # the descriptors' one size


@pytest.mark.parametrize("kind", logits.KINDS)
def test_tree_refusals(fa, kind):
    L = fa.lib()
    for bad in (0, 8, 15, 24, 32):
        assert _tree(fa, kind, opts_size=bad) == INVALID, bad
        assert _tree(fa, kind, mask=None, opts_size=bad) == INVALID, bad        # a wrong size is refused with or without a mask
    # the mask's own rules: the triangle's place, one bit per token, 8-byte words
    assert _tree(fa, kind, causal=0) == INVALID
    assert _tree(fa, kind, max_q=65, total_q=80) == INVALID and _tree(fa, kind, max_q=1000, total_q=1000) == INVALID
    for off in (1, 2, 4, 7):
        assert _tree(fa, kind, mask=MASK + off) == INVALID, off
    # everything the plain entry refuses, with the mask and through null options and a null mask
    bads = list(logits.PAGED if "paged" in kind else logits.CONTIG) + [dict(cu_seqlens_q=0), dict(total_q=0), dict(max_q=0), dict(Q=4096 + 8),
                                                                      dict(q_stride_t=32), dict(o_stride_h=65), dict(size=8)]
    for bad in bads:
        if bad.get("causal", 1) != 1:
            continue
        assert _tree(fa, kind, **bad) == INVALID, (kind, bad)
    for bad in bads:
        d = decodev._desc(fa, kind, **bad)
        assert L.fa_kvcache_decode_varlen_ex(ctypes.byref(d), None) == INVALID == L.fa_kvcache_decode_varlen(ctypes.byref(d)), bad
        assert _tree(fa, kind, mask=None, **dict(dict(causal=0), **bad)) == INVALID, bad
    assert L.fa_kvcache_decode_varlen_ex(None, None) == INVALID
    # a split needs the workspace the plain sizing function gives
    big = dict(max_pages=512, page_size=16) if "paged" in kind else dict(Ncap=8192)
    assert decodev._bytes(fa, kind, **big) > 0 and _tree(fa, kind, **big) == INVALID


@pytest.mark.parametrize("kind", appendv.KINDS)
def test_position_refusals(fa, kind):
    L = fa.lib()
    rope = "rope" in kind
    for bad in (0, 8, 15, 24):
        assert _pos(fa, kind, opts_size=bad) == INVALID and _pos(fa, kind, pos=None, opts_size=bad) == INVALID, bad
    if not rope:
        assert _pos(fa, kind) == INVALID, "positions without rope_cos"
    else:
        for off in (1, 2, 3):
            assert _pos(fa, kind, pos=POS + off) == INVALID, off
    for bad in appendv.COMMON:
        assert _pos(fa, kind, **bad) == INVALID, (kind, bad)
        d = appendv._desc(fa, kind, **bad)
        assert L.fa_kvcache_append_varlen_ex(ctypes.byref(d), None) == INVALID == L.fa_kvcache_append_varlen(ctypes.byref(d)), bad
        assert _pos(fa, kind, pos=None, **bad) == INVALID, bad
    assert L.fa_kvcache_append_varlen_ex(None, None) == INVALID


def test_python_checks(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(6, 4, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    mask = torch.zeros(6, dtype=torch.int64)
    dec = fa.fa_kvcache_decode_varlen
    for bad, what in ((mask.int(), "int64"), (mask[:5], "total_q"), (mask[None], "total_q"), (torch.zeros(12, dtype=torch.int64)[::2], "total_q"),
                      (torch.zeros(6, dtype=torch.int64, device="meta"), "device"), ([0] * 6, "int64")):
        with pytest.raises(ValueError, match=what):
            dec(q, k, k, cu, 3, lens, causal=True, tree_mask=bad)
    with pytest.raises(ValueError, match="causal"):
        dec(q, k, k, cu, 3, lens, causal=False, tree_mask=mask)
    with pytest.raises(ValueError, match="<= 64"):
        dec(q, k, k, cu, 65, lens, causal=True, tree_mask=mask)
    k8 = k.to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="causal"):
        fa.fa_kvcache_decode_varlen_fp8(q, k8, k8, cu, 3, lens, tree_mask=mask)
    for call in (lambda: dec(q, k, k, cu, 3, lens, causal=True, tree_mask=mask),
                 lambda: fa.fa_kvcache_decode_varlen_fp8(q, k8, k8, cu, 3, lens, causal=True, tree_mask=mask)):
        with pytest.raises(ValueError, match="device tensor"):   # everything else in order: the HIP path has no CPU fallback
            call()
    # the append
    kn = torch.zeros(6, 2, 64, dtype=torch.float16)
    pos = torch.zeros(6, dtype=torch.int32)
    cos = torch.zeros(16, 16, dtype=torch.float32)
    app = fa.fa_kvcache_append_varlen
    with pytest.raises(ValueError, match="rotary_cos"):
        app(kn, kn, k, k, cu, lens, positions=pos)
    for bad, what in ((pos.long(), "int32"), (pos[:4], "total_new"), (torch.zeros(12, dtype=torch.int32)[::2], "total_new"),
                      (torch.zeros(6, dtype=torch.int32, device="meta"), "device")):
        with pytest.raises(ValueError, match=what):
            app(kn, kn, k, k, cu, lens, rotary_cos=cos, rotary_sin=cos, positions=bad)
    for call in (lambda: app(kn, kn, k, k, cu, lens, rotary_cos=cos, rotary_sin=cos, positions=pos),
                 lambda: fa.fa_kvcache_append_varlen_fp8(kn, kn, k8, k8, cu, lens, rotary_cos=cos, rotary_sin=cos, positions=pos)):
        with pytest.raises(ValueError, match="device tensor"):
            call()


def test_custom_ops_register(fa):
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    meta = dict(device="meta")
    q = torch.empty(9, 8, 128, dtype=torch.bfloat16, **meta)
    k = torch.empty(2, 2, 500, 128, dtype=torch.bfloat16, **meta)
    k8 = torch.empty(2, 2, 500, 128, dtype=torch.float8_e4m3fn, **meta)
    cu, lens = torch.empty(3, dtype=torch.int32, **meta), torch.empty(2, dtype=torch.int32, **meta)
    sc = torch.empty(2, dtype=torch.float32, **meta)
    mask = torch.empty(9, dtype=torch.int64, **meta)
    for o, lse in (ops.decode_varlen_tree(q, k, k, cu, 4, lens, None, mask, 0.125, True, 0, None, 0.0, True),
                   ops.decode_varlen_tree_fp8(q, k8, k8, cu, 4, lens, None, mask, sc, None, 0.125, True, 64, None, 1.0, True)):
        assert o.shape == q.shape and o.dtype == torch.float32 and lse.shape == (8, 9)
    names = [a.name for a in ops.decode_varlen_tree_fp8.default._schema.arguments]
    assert names == ["q", "k_cache", "v_cache", "cu_seqlens_q", "max_seqlen_q", "cache_seqlens", "block_table", "tree_mask", "k_scale",
                     "v_scale", "scale", "causal", "window", "sinks", "softcap", "out_f32"]
    names = [a.name for a in ops.append_varlen_pos_fp8.default._schema.arguments]
    assert names == ["k_new", "v_new", "k_cache", "v_cache", "cu_seqlens_new", "cache_seqlens", "seqlens_out", "block_table", "k_scale",
                     "v_scale", "positions", "q", "q_out", "rotary_cos", "rotary_sin", "interleaved"]
    assert [a.name for a in ops.append_varlen_pos.default._schema.arguments][8] == "positions"
    # the existing ops keep their schemas
    assert "tree_mask" not in [a.name for a in ops.decode_varlen.default._schema.arguments]
    assert "positions" not in [a.name for a in ops.append_varlen.default._schema.arguments]
