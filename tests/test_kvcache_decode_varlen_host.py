"""CPU tier of the token-packed decode entry fa_kvcache_decode_varlen, through the C ABI: the symbols are exported and bound, the ctypes
structure mirrors the header, every refusal holds before the device is touched, and the sizing function is the padded entry's with
Nq = max_q.  Only calls that must be rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os

import pytest

import test_kvcache_logits_host as logits
import test_kvcache_ragged_host as ragged

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fa_kvcache_decode_varlen_workspace_bytes", "fa_kvcache_decode_varlen")


def _desc(fa, kind="", **kw):
    """a descriptor with small made-up addresses that WOULD be launched (one token per sequence, about 200 keys, one pass); the padded
    entry's keyword Nq names max_q here, so that its lists of refusals apply as they are"""
    f = dict(Q=4096, O=8192, K=16, V=16, cu_seqlens_q=16, B=1, Hkv=1, G=1, d=64, total_q=4, max_q=1, q_stride_t=64, q_stride_h=64,
             o_stride_t=64, o_stride_h=64, scale=0.125, causal=0, window=0, softcap=0.0, in_dtype=0, out_dtype=0)
    if "paged" in kind:
        f.update(block_table=16, num_pages=8, page_size=16, max_pages=12)
    else:
        f.update(Ncap=200)
    if "fp8" in kind:
        f.update(kv_dtype=fa.capi.KV_FP8_E4M3)
    for k, v in kw.items():
        f["max_q" if k == "Nq" else k] = v
    return fa.capi.KvDecodeVarlenDesc(**f)


def _call(fa, kind="", **kw):
    return fa.lib().fa_kvcache_decode_varlen(ctypes.byref(_desc(fa, kind, **kw)))


def _bytes(fa, kind="", **kw):
    return fa.lib().fa_kvcache_decode_varlen_workspace_bytes(ctypes.byref(_desc(fa, kind, **kw)))


def test_symbols_and_struct(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    for n in NAMES:
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
        assert n not in fa.capi.SYMBOLS[:9] and n not in fa.capi.SYMBOLS[-2:], n   # between the head slice and the pinned tail
    D = fa.capi.KvDecodeVarlenDesc
    assert L.fa_kvcache_decode_varlen.argtypes == [ctypes.POINTER(D)] and L.fa_kvcache_decode_varlen.restype is ctypes.c_int
    assert L.fa_kvcache_decode_varlen_workspace_bytes.restype is ctypes.c_size_t
    fields = ragged._header_fields("fa_kvdecode_varlen_desc")
    assert fields == [f[0] for f in D._fields_] and fields[0] == "size" and fields[-1] == "stream"
    # everything the padded descriptor carries about the cache and the options; the packed fields of the varlen prefill; max_q
    padded = [f[0] for f in fa.capi.KvDecodeDesc._fields_]
    assert set(padded) - set(fields) == {"Nq", "seqlens_q"}
    assert set(fields) - set(padded) == {"cu_seqlens_q", "total_q", "max_q", "q_stride_t", "q_stride_h", "o_stride_t", "o_stride_h"}
    assert D().size == ctypes.sizeof(D) and fa.capi.new_desc(D).size == ctypes.sizeof(D)
    header = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    for decl in ("size_t fa_kvcache_decode_varlen_workspace_bytes(const fa_kvdecode_varlen_desc* desc);",
                 "int fa_kvcache_decode_varlen(const fa_kvdecode_varlen_desc* desc);"):
        assert decl in header
    for name in ("fa_kvcache_decode_varlen", "fa_kvcache_decode_varlen_fp8", "kvcache_decode_varlen_workspace_bytes"):
        assert callable(getattr(fa, name)) and name in fa.__all__


def test_the_good_descriptor_is_only_short_of_a_device(fa):
    """the base descriptor passes every check: what stops it is listed below, one field at a time"""
    D = fa.capi.KvDecodeVarlenDesc
    for kind in logits.KINDS:
        assert _bytes(fa, kind) == 0                          # one pass: no workspace
        assert _bytes(fa, kind, size=ctypes.sizeof(D)) == 0


@pytest.mark.parametrize("kind", logits.KINDS)
def test_refuses_what_the_padded_entry_refuses(fa, kind):
    """every case of the padded descriptor's CPU tier with Nq = max_q"""
    for bad in (logits.PAGED if "paged" in kind else logits.CONTIG):
        assert _call(fa, kind, **bad) == INVALID, (kind, bad)
        if "fp8" in kind:
            assert _call(fa, kind, k_scale=16, v_scale=16, **bad) == INVALID, (kind, bad)
    if "fp8" not in kind:   # a 16-bit cache has no scales
        assert _call(fa, kind, k_scale=16) == INVALID and _call(fa, kind, v_scale=16) == INVALID


@pytest.mark.parametrize("kind", logits.KINDS)
def test_refusals_of_the_packed_fields(fa, kind):
    L = fa.lib()
    size = ctypes.sizeof(fa.capi.KvDecodeVarlenDesc)
    assert L.fa_kvcache_decode_varlen(None) == INVALID and L.fa_kvcache_decode_varlen_workspace_bytes(None) == 0
    # any wrong size, the padded descriptor's two among them
    for bad in (0, 8, size - 8, size + 8, size - 4, ctypes.sizeof(fa.capi.KvDecodeDesc), fa.capi.KvDecodeDesc.seqlens_q.offset,
                ctypes.sizeof(fa.capi.VarlenKvcacheDesc)):
        assert _call(fa, kind, size=bad) == INVALID and _bytes(fa, kind, size=bad) == 0, bad
    cases = [
        dict(cu_seqlens_q=0), dict(total_q=0), dict(total_q=-4), dict(max_q=0), dict(max_q=-1),
        # fa_forward_varlen's checks on packed Q and O: alignment, strides, 32-bit byte offsets
        dict(Q=4096 + 8), dict(O=8192 + 2), dict(Q=0), dict(O=0),
        dict(q_stride_t=32), dict(o_stride_t=63), dict(q_stride_t=68), dict(o_stride_t=72 + 4), dict(q_stride_h=-64), dict(o_stride_h=-8),
        dict(q_stride_h=4), dict(o_stride_h=65),
        dict(total_q=1 << 25, q_stride_t=64), dict(total_q=1 << 24, out_dtype=0, o_stride_t=64), dict(Hkv=2, G=2, q_stride_h=1 << 30),
        dict(Hkv=2, G=2, o_stride_h=1 << 29),
        # one (sequence, K/V head) view: (min(max_q, total_q) - 1) * stride_t + Hq * stride_h + d elements inside 32 bits of bytes
        # (these two pass fa_forward_varlen's bound, which counts Hq - 1 head strides)
        dict(Hkv=8, G=4, total_q=2, q_stride_h=1 << 26, max_q=2),
        dict(Hkv=8, G=4, total_q=2, o_stride_h=1 << 25, max_q=2),
    ]
    assert _call(fa, kind, Hkv=8, G=4, total_q=2, q_stride_h=1 << 25, o_stride_h=1 << 24, max_q=2, B=0) == INVALID   # (B alone is wrong)
    for bad in cases:
        assert _call(fa, kind, **bad) == INVALID, (kind, bad)
    # a split needs a workspace here too: many keys for one token per sequence
    big = dict(max_pages=512, page_size=16) if "paged" in kind else dict(Ncap=8192)
    assert _bytes(fa, kind, **big) > 0
    assert _call(fa, kind, **big) == INVALID and _call(fa, kind, workspace=16, workspace_bytes=8, **big) == INVALID


def test_workspace_is_the_padded_entrys(fa):
    """all four forms and a window: the sizing function of the padded descriptor with Nq = max_q; total_q, the strides and the vector
    do not enter"""
    L = fa.lib()
    some = 0
    for kind in logits.KINDS:
        for kw in (dict(Ncap=8192), dict(Ncap=32768, window=1024, B=3, G=2, Nq=5, d=128), dict(Ncap=200), dict(Ncap=32768, B=8, Hkv=8, G=4, Nq=16, d=128),
                   dict(Ncap=4096, B=256, Hkv=8, G=4, Nq=1, d=64)):
            if "paged" in kind:
                kw = dict({k: v for k, v in kw.items() if k != "Ncap"}, max_pages=kw["Ncap"] // 16, page_size=16)
            want = L.fa_kvcache_decode_workspace_bytes(ctypes.byref(logits._desc(fa, kind, **kw)))
            assert _bytes(fa, kind, **kw) == want, (kind, kw)
            assert _bytes(fa, kind, total_q=12345, q_stride_t=1 << 20, cu_seqlens_q=0, Q=0, **kw) == want
            some += want > 0
    assert some >= 12
    for bad in (dict(kv_dtype=2), dict(kv_dtype=-1), dict(k_scale=16), dict(size=8)):
        assert _bytes(fa, Ncap=8192, **bad) == 0, bad
    assert fa.kvcache_decode_varlen_workspace_bytes(1, 1, 1, 1, 64, Ncap=8192) == _bytes(fa, Ncap=8192) > 0
    assert fa.kvcache_decode_varlen_workspace_bytes(3, 1, 2, 5, 128, max_pages=2048, page_size=16, window=1024) == \
        _bytes(fa, "paged_", max_pages=2048, page_size=16, window=1024, B=3, G=2, Nq=5, d=128)


def test_python_checks(fa):
    torch = pytest.importorskip("torch")
    q = torch.zeros(6, 4, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)
    table = torch.zeros(2, 5, dtype=torch.int32)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    for bad_max in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_seqlen_q"):
            fa.fa_kvcache_decode_varlen(q, k, k, cu, bad_max, lens)
    with pytest.raises(ValueError, match="int32"):
        fa.fa_kvcache_decode_varlen(q, k, k, cu.long(), 3, lens)
    with pytest.raises(ValueError, match="packed"):
        fa.fa_kvcache_decode_varlen(q[None], k, k, cu, 3, lens)
    with pytest.raises(ValueError, match="holds 2 sequences"):
        fa.fa_kvcache_decode_varlen(q, k, k, torch.tensor([0, 6], dtype=torch.int32), 3, None)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        fa.fa_kvcache_decode_varlen_fp8(q, k, k, cu, 3, lens)
    with pytest.raises(ValueError, match="last dimension"):
        fa.fa_kvcache_decode_varlen(q.transpose(1, 2).contiguous().transpose(1, 2), k, k, cu, 3, lens)
    for call in (lambda: fa.fa_kvcache_decode_varlen(q, k, k, cu, 3, lens), lambda: fa.fa_kvcache_decode_varlen(q, pool, pool, cu, 3, lens, table),
                 lambda: fa.fa_kvcache_decode_varlen_fp8(q, k.to(torch.float8_e4m3fn), k.to(torch.float8_e4m3fn), cu, 3, lens)):
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
        for o, lse in (ops.decode_varlen(q, k, k, cu, 4, lens, None, 0.125, True, 0, sinks, 0.0, f32),
                       ops.decode_varlen_fp8(q, pool8, pool8, cu, 1, None, table, sc, None, 0.125, True, 64, None, 1.0, f32)):
            assert o.shape == q.shape and o.dtype == (torch.float32 if f32 else torch.bfloat16) and lse.shape == (8, 9)
    names = [a.name for a in ops.decode_varlen_fp8.default._schema.arguments]
    assert names == ["q", "k_cache", "v_cache", "cu_seqlens_q", "max_seqlen_q", "cache_seqlens", "block_table", "k_scale", "v_scale", "scale",
                     "causal", "window", "sinks", "softcap", "out_f32"]
    c = torch.zeros(1, 1, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.decode_varlen(c, c[None], c[None], torch.zeros(2, dtype=torch.int32), 1, None, None, 0.125, False, 0, None, 0.0, True)
