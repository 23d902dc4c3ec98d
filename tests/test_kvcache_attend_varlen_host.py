"""CPU tier of the mixed prefill + decode step fa_kvcache_attend_varlen[_part], through the C ABI: the symbols are exported and bound,
the header declares them, and every refusal holds before the device is touched -- what fa_kvcache_decode_varlen refuses for the
descriptor, what fa_forward_varlen_kvcache refuses for the same fields, causal != 1, a null seqlens_k and parts outside {1, 2, 3}.
Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os

import pytest

import test_kvcache_decode_varlen_host as dvh
import test_kvcache_logits_host as logits

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fa_kvcache_attend_varlen", "fa_kvcache_attend_varlen_part")
PARTS = (1, 2, 3)


def _desc(fa, kind="", **kw):
    """the packed decode tier's good descriptor (max_q: the threshold, here 1) made a mixed step's: causal, with lengths"""
    return dvh._desc(fa, kind, **dict(dict(causal=1, seqlens_k=16), **kw))


def _calls(fa, kind="", **kw):
    """the return codes of the plain entry and of every part"""
    L, desc = fa.lib(), _desc(fa, kind, **kw)
    return [L.fa_kvcache_attend_varlen(ctypes.byref(desc))] + [L.fa_kvcache_attend_varlen_part(ctypes.byref(desc), p) for p in PARTS]


def _refused(fa, kind="", **kw):
    return _calls(fa, kind, **kw) == [INVALID] * (1 + len(PARTS))


def test_symbols_header_and_front_ends(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    D = fa.capi.KvDecodeVarlenDesc
    for n in NAMES:
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
        assert n not in fa.capi.SYMBOLS[:9] and n not in fa.capi.SYMBOLS[-2:], n   # between the head slice and the pinned tail
        assert getattr(L, n).restype is ctypes.c_int
    assert L.fa_kvcache_attend_varlen.argtypes == [ctypes.POINTER(D)]
    assert L.fa_kvcache_attend_varlen_part.argtypes == [ctypes.POINTER(D), ctypes.c_int]
    assert (fa.capi.ATTEND_SHORT, fa.capi.ATTEND_LONG) == (1, 2)
    header = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    for decl in ("#define FA_ATTEND_SHORT 1", "#define FA_ATTEND_LONG  2",
                 "int fa_kvcache_attend_varlen(const fa_kvdecode_varlen_desc* desc);",
                 "int fa_kvcache_attend_varlen_part(const fa_kvdecode_varlen_desc* desc, int parts);"):
        assert decl in header, decl
    # the descriptor is the packed decode entry's, unchanged; its sizing function sizes this entry's workspace, and the header says so
    assert dvh.ragged._header_fields("fa_kvdecode_varlen_desc") == [f[0] for f in D._fields_]
    assert "fa_kvcache_decode_varlen_workspace_bytes(desc) sizes the workspace of this entry" in " ".join(header.split()).replace(" * ", " ")
    assert "total_q <= T" in header
    for name in ("fa_kvcache_attend_varlen", "fa_kvcache_attend_varlen_fp8"):
        assert callable(getattr(fa, name)) and name in fa.__all__


def test_the_good_descriptor_is_only_short_of_a_device(fa):
    """the base descriptor passes every check of both entries it is judged by: fa_kvcache_decode_varlen's sizing function accepts it (one
    pass, no workspace), and what stops a call is listed below, one field at a time.  (No call is issued on it: it would be launched.)"""
    for kind in logits.KINDS:
        d = _desc(fa, kind)
        assert fa.lib().fa_kvcache_decode_varlen_workspace_bytes(ctypes.byref(d)) == 0
        assert d.causal == 1 and d.seqlens_k and d.size == ctypes.sizeof(fa.capi.KvDecodeVarlenDesc)
        assert d.total_q > d.max_q                         # the LONG half would be launched too


@pytest.mark.parametrize("kind", logits.KINDS)
def test_refuses_what_the_packed_decode_entry_refuses(fa, kind):
    """every case of the padded descriptor's CPU tier with Nq = max_q, for the plain entry and every part"""
    for bad in (logits.PAGED if "paged" in kind else logits.CONTIG):
        assert _refused(fa, kind, **bad), (kind, bad)
    if "fp8" not in kind:   # a 16-bit cache has no scales
        assert _refused(fa, kind, k_scale=16) and _refused(fa, kind, v_scale=16)
    L = fa.lib()
    assert L.fa_kvcache_attend_varlen(None) == INVALID and L.fa_kvcache_attend_varlen_part(None, 3) == INVALID
    size = ctypes.sizeof(fa.capi.KvDecodeVarlenDesc)
    for bad in (0, 8, size - 8, size + 8, ctypes.sizeof(fa.capi.KvDecodeDesc), ctypes.sizeof(fa.capi.VarlenKvcacheDesc)):
        assert _refused(fa, kind, size=bad), bad
    for bad in (dict(cu_seqlens_q=0), dict(total_q=0), dict(total_q=-4), dict(max_q=0), dict(max_q=-1),
                dict(Q=4096 + 8), dict(O=8192 + 2), dict(Q=0), dict(O=0), dict(q_stride_t=32), dict(o_stride_t=63), dict(q_stride_t=68),
                dict(q_stride_h=-64), dict(o_stride_h=-8), dict(q_stride_h=4), dict(o_stride_h=65),
                dict(Hkv=8, G=4, total_q=2, q_stride_h=1 << 26, max_q=2), dict(Hkv=8, G=4, total_q=2, o_stride_h=1 << 25, max_q=2)):
        assert _refused(fa, kind, **bad), (kind, bad)
    # the SHORT half's workspace is checked whichever parts are asked for: many keys for one row per sequence need a split
    big = dict(max_pages=512, page_size=16) if "paged" in kind else dict(Ncap=8192)
    assert fa.lib().fa_kvcache_decode_varlen_workspace_bytes(ctypes.byref(_desc(fa, kind, **big))) > 0
    assert _refused(fa, kind, **big) and _refused(fa, kind, workspace=16, workspace_bytes=8, **big)


@pytest.mark.parametrize("kind", logits.KINDS)
def test_refusals_of_its_own(fa, kind):
    L = fa.lib()
    # a mixed step is causal, and the tiled half needs the lengths
    assert _refused(fa, kind, causal=0) and _refused(fa, kind, causal=2) and _refused(fa, kind, seqlens_k=0)
    desc = _desc(fa, kind)
    for parts in (0, 4, -1, 7, 1 << 8 | 3):
        assert L.fa_kvcache_attend_varlen_part(ctypes.byref(desc), parts) == INVALID, parts
    # fa_forward_varlen_kvcache's bounds cover ALL total_q rows of Q and O, not T of them; K and V must be 16-byte aligned for the
    # tiled kernel's loads
    assert _refused(fa, kind, total_q=1 << 25, q_stride_t=64) and _refused(fa, kind, total_q=1 << 24, out_dtype=0, o_stride_t=64)
    assert _refused(fa, kind, K=24) and _refused(fa, kind, V=8)
    # a capacity whose rows of one (sequence, head) do not fit 32 bits of bytes (the workspace is ample: it is the capacity that stops it)
    cap = dict(max_pages=1 << 21, page_size=16) if "paged" in kind else dict(Ncap=1 << 25)
    assert _refused(fa, kind, d=128, workspace=16, workspace_bytes=1 << 40, **cap)


def test_python_checks(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(6, 4, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)
    table = torch.zeros(2, 5, dtype=torch.int32)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="split_rows"):
            fa.fa_kvcache_attend_varlen(q, k, k, cu, lens, split_rows=bad)
    for bad in (0, 4, -1, True, None, 1.0):
        with pytest.raises(ValueError, match="parts"):
            fa.fa_kvcache_attend_varlen(q, k, k, cu, lens, parts=bad)
    with pytest.raises(ValueError, match="cache_seqlens"):
        fa.fa_kvcache_attend_varlen(q, k, k, cu, None)
    with pytest.raises(ValueError, match="int32"):
        fa.fa_kvcache_attend_varlen(q, k, k, cu.long(), lens)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        fa.fa_kvcache_attend_varlen_fp8(q, k, k, cu, lens)
    for call in (lambda: fa.fa_kvcache_attend_varlen(q, k, k, cu, lens), lambda: fa.fa_kvcache_attend_varlen(q, pool, pool, cu, lens, table),
                 lambda: fa.fa_kvcache_attend_varlen_fp8(q, k.to(torch.float8_e4m3fn), k.to(torch.float8_e4m3fn), cu, lens, parts=2)):
        with pytest.raises(ValueError, match="device tensor"):   # everything else in order: the HIP path has no CPU fallback
            call()


def test_custom_ops_register(fa):
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    q = torch.empty(9, 8, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(2, 2, 500, 128, dtype=torch.bfloat16, device="meta")
    pool8 = torch.empty(40, 2, 32, 128, dtype=torch.float8_e4m3fn, device="meta")
    table = torch.empty(2, 16, dtype=torch.int32, device="meta")
    cu = torch.empty(3, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    sc = torch.empty(2, dtype=torch.float32, device="meta")
    sinks = torch.empty(8, dtype=torch.float32, device="meta")
    for f32 in (True, False):
        for o, lse in (ops.attend_varlen(q, k, k, cu, lens, None, 128, 0.125, 0, sinks, 0.0, 3, f32),
                       ops.attend_varlen_fp8(q, pool8, pool8, cu, lens, table, sc, None, 4, 0.125, 64, None, 1.0, 1, f32)):
            assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and lse.shape == (8, 9)
    names = [a.name for a in ops.attend_varlen_fp8.default._schema.arguments]
    assert names == ["q", "k_cache", "v_cache", "cu_seqlens_q", "cache_seqlens", "block_table", "k_scale", "v_scale", "split_rows", "scale",
                     "window", "sinks", "softcap", "parts", "out_f32"]
    c = torch.zeros(1, 1, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.attend_varlen(c, c[None], c[None], torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), None, 4, 0.125, 0, None,
                          0.0, 3, True)
