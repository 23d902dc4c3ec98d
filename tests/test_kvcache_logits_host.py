"""CPU tier of the descriptor decode entry (fa_kvcache_decode, fa_kvcache_decode_workspace_bytes) and of the `sinks` / `softcap`
keywords: the symbols are exported and bound, the descriptor mirrors the header's struct, a bad descriptor, a bad soft-cap and
everything the flat entries reject is rejected before the device is touched, the sizing function equals the existing ones for all
eight forms, the Python front ends refuse what they must, and the four _ex ops register.  Only calls that must be rejected are
issued, so the file is safe where a GPU is visible."""
import ctypes
import os
import re

import pytest

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_struct(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    for n in ("fa_kvcache_decode", "fa_kvcache_decode_workspace_bytes"):
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
        assert getattr(L, n).argtypes == [ctypes.POINTER(fa.capi.KvDecodeDesc)]
    assert L.fa_kvcache_decode.restype is ctypes.c_int and L.fa_kvcache_decode_workspace_bytes.restype is ctypes.c_size_t
    # the ctypes structure names the header's fields in the header's order, and `size` is filled in
    text = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct fa_kvdecode_desc \{(.*?)\} fa_kvdecode_desc;", text, re.S).group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if decl.strip()]
    assert names == [f[0] for f in fa.capi.KvDecodeDesc._fields_], names
    assert names[0] == "size" and fa.capi.KvDecodeDesc().size == ctypes.sizeof(fa.capi.KvDecodeDesc)
    assert (fa.capi.KV_16BIT, fa.capi.KV_FP8_E4M3) == (0, 1)


def _desc(fa, kind="", **kw):
    """a descriptor with small made-up addresses that WOULD be launched (about 200 keys, one pass): every case below must be turned
    away before anything dereferences them"""
    f = dict(Q=16, K=16, V=16, O=16, B=1, Hkv=1, G=1, Nq=1, d=64, scale=0.125, causal=0, window=0, softcap=0.0, in_dtype=0, out_dtype=0)
    if "paged" in kind:
        f.update(block_table=16, num_pages=8, page_size=16, max_pages=12)
    else:
        f.update(Ncap=200)
    if "fp8" in kind:
        f.update(kv_dtype=fa.capi.KV_FP8_E4M3)
    f.update(kw)
    return fa.capi.KvDecodeDesc(**f)


def _call(fa, kind="", **kw):
    return fa.lib().fa_kvcache_decode(ctypes.byref(_desc(fa, kind, **kw)))


KINDS = ("", "paged_", "fp8_", "paged_fp8_")
WS = dict(workspace=16, workspace_bytes=1 << 40)
COMMON = [
    dict(size=0), dict(size=8), dict(size=ctypes.sizeof(ctypes.c_void_p) * 64), dict(kv_dtype=2), dict(kv_dtype=-1),
    dict(softcap=-1.0), dict(softcap=-0.5, sinks=16), dict(softcap=float("nan")), dict(softcap=float("inf")), dict(softcap=float("-inf")),
    dict(window=-1), dict(window=-1, softcap=1.0), dict(window=-2 ** 31, sinks=16),
    dict(Q=0), dict(K=0), dict(V=0), dict(O=0), dict(Q=0, sinks=16, softcap=2.0),
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(G=0), dict(G=-2), dict(Nq=0), dict(Nq=0, softcap=1.0),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0), dict(d=96, sinks=16),
    dict(causal=2), dict(causal=-1), dict(in_dtype=2), dict(in_dtype=-1), dict(out_dtype=2), dict(out_dtype=7),
    dict(G=1 << 12, Nq=1 << 12, **WS), dict(G=1 << 16, Nq=1 << 16), dict(B=1 << 16, Hkv=1 << 16),
]
CONTIG = COMMON + [
    dict(Ncap=0), dict(Ncap=-5), dict(Ncap=-5, softcap=1.0),
    # a split needs a workspace: without a window, under one, and on the sink / soft-cap path (window 0 and windowed)
    dict(Ncap=8192), dict(Ncap=8192, window=4096), dict(Ncap=8192, sinks=16), dict(Ncap=8192, softcap=30.0, window=4096),
    dict(Ncap=8192, sinks=16, workspace=16, workspace_bytes=8), dict(Ncap=8192, softcap=1.0, workspace=None, workspace_bytes=1 << 30),
    dict(Ncap=1 << 25, d=128, **WS), dict(Ncap=1 << 26, d=64, sinks=16, **WS),
]
PAGED = COMMON + [
    dict(page_size=0), dict(page_size=8), dict(page_size=24), dict(page_size=-16), dict(page_size=24, sinks=16),
    dict(num_pages=0), dict(num_pages=-3), dict(max_pages=0), dict(max_pages=-1), dict(max_pages=-1, softcap=1.0),
    dict(max_pages=1 << 27, page_size=16), dict(max_pages=1 << 16, page_size=1 << 15),
    dict(max_pages=512, page_size=16), dict(max_pages=512, page_size=16, sinks=16), dict(max_pages=512, page_size=16, window=4096, softcap=1.0),
    dict(max_pages=1 << 21, page_size=16, d=128, **WS),
]


@pytest.mark.parametrize("kind", KINDS)
def test_rejects_without_device(fa, kind):
    for bad in (PAGED if "paged" in kind else CONTIG):
        assert _call(fa, kind, **bad) == INVALID, (kind, bad)
        if "fp8" in kind:
            assert _call(fa, kind, k_scale=16, v_scale=16, **bad) == INVALID, (kind, bad)
    if "fp8" not in kind:   # a 16-bit cache has no scales
        assert _call(fa, kind, k_scale=16) == INVALID and _call(fa, kind, v_scale=16) == INVALID


def test_null_descriptor(fa):
    L = fa.lib()
    assert L.fa_kvcache_decode(None) == INVALID
    assert L.fa_kvcache_decode_workspace_bytes(None) == 0
    for bad in (dict(size=0), dict(size=8), dict(kv_dtype=5)):
        assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(_desc(fa, Ncap=8192, **bad))) == 0


def test_workspace_bytes_equal_the_existing_functions(fa):
    """for all eight forms (contiguous / paged x 16 bit / fp8 x window / none), with and without the two options: the split count
    and the workspace depend on the shape and the window alone"""
    L = fa.lib()
    some = 0
    for (B, Hkv, G, Nq, d) in ((3, 2, 2, 1, 64), (1, 1, 1, 1, 128), (2, 2, 4, 5, 128), (8, 16, 1, 1, 64)):
        for Ncap in (192, 1024, 4096, 32768):
            for W in (0, 1, 100, 1024, Ncap, 2 ** 31 - 1):
                want = L.fa_forward_kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W)
                if W == 0:
                    assert want == L.fa_forward_kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d)
                some += want > 0
                for fp8 in ("", "fp8_"):
                    for opt in (dict(), dict(sinks=16), dict(softcap=1.0), dict(sinks=16, softcap=30.0)):
                        kw = dict(B=B, Hkv=Hkv, G=G, Nq=Nq, d=d, window=W, **opt)
                        assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(_desc(fa, fp8, Ncap=Ncap, **kw))) == want
                        for ps in (16, 256):
                            pw = L.fa_forward_kvcache_paged_window_workspace_bytes(B, Hkv, G, Nq, Ncap // ps, ps, d, W)
                            got = L.fa_kvcache_decode_workspace_bytes(
                                ctypes.byref(_desc(fa, "paged_" + fp8, max_pages=Ncap // ps, page_size=ps, num_pages=7, **kw)))
                            assert got == pw
                            if W == 0:
                                assert pw == L.fa_forward_kvcache_paged_workspace_bytes(B, Hkv, G, Nq, Ncap // ps, ps, d)
    assert some > 20
    for bad in (dict(window=-1), dict(B=0), dict(d=96), dict(Ncap=0)):
        assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(_desc(fa, **{"Ncap": 8192, **bad}))) == 0
    assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(_desc(fa, "paged_", page_size=24, max_pages=512))) == 0


def test_python_checks_on_sinks_and_softcap(fa):
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd import ops
    cpu = torch.device("cpu")
    good = torch.zeros(8, dtype=torch.float32)
    assert ops._sinks_ptr(None, 8, cpu) is None
    with pytest.raises(ValueError, match="float32"):
        ops._sinks_ptr(good.double(), 8, cpu)
    with pytest.raises(ValueError, match="float32"):
        ops._sinks_ptr(good.half(), 8, cpu)
    with pytest.raises(ValueError, match="float32"):
        ops._sinks_ptr([0.0] * 8, 8, cpu)
    with pytest.raises(ValueError, match="per query head"):
        ops._sinks_ptr(good, 4, cpu)          # Hkv values where Hkv * G are needed
    with pytest.raises(ValueError, match="per query head"):
        ops._sinks_ptr(good[:7], 8, cpu)
    with pytest.raises(ValueError, match="contiguous"):
        ops._sinks_ptr(torch.zeros(16, dtype=torch.float32)[::2], 8, cpu)
    with pytest.raises(ValueError, match="is on"):
        ops._sinks_ptr(good, 8, torch.device("meta"))
    with pytest.raises(ValueError, match="device tensor"):
        ops._sinks_ptr(good, 8, cpu)          # everything else in order: the HIP path has no CPU fallback
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="softcap"):
            ops._softcap(bad)
    assert ops._softcap(0) == 0.0 and ops._softcap(30) == 30.0 and ops._softcap(1.5) == 1.5
    # the four front ends take the keywords and still refuse CPU tensors
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)
    k8, pool8 = k.to(torch.float8_e4m3fn), pool.to(torch.float8_e4m3fn)
    table = torch.zeros(2, 5, dtype=torch.int32)
    calls = (lambda **kw: fa.fa_forward_kvcache(q, k, k, **kw), lambda **kw: fa.fa_forward_kvcache_paged(q, pool, pool, table, **kw),
             lambda **kw: fa.fa_forward_kvcache_fp8(q, k8, k8, **kw), lambda **kw: fa.fa_forward_kvcache_paged_fp8(q, pool8, pool8, table, **kw))
    for call in calls:
        for kw in (dict(sinks=torch.zeros(4)), dict(softcap=1.0), dict(sinks=torch.zeros(4), softcap=30.0, window=5)):
            with pytest.raises(ValueError):
                call(**kw)


def test_decode_ex_custom_ops_register(fa):
    """the four _ex ops exist after register(), trace on meta tensors, have no CPU kernel, and leave the other ops' schemas alone"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    q = torch.empty(2, 8, 3, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(2, 2, 500, 128, dtype=torch.bfloat16, device="meta")
    pool = torch.empty(40, 2, 32, 128, dtype=torch.bfloat16, device="meta")
    k8, pool8 = (torch.empty(x.shape, dtype=torch.float8_e4m3fn, device="meta") for x in (k, pool))
    table = torch.empty(2, 16, dtype=torch.int32, device="meta")
    lens = torch.empty(2, dtype=torch.int32, device="meta")
    sc = torch.empty(2, dtype=torch.float32, device="meta")
    sinks = torch.empty(8, dtype=torch.float32, device="meta")
    for s, cap, f32 in ((sinks, 0.0, True), (None, 30.0, False), (sinks, 1.0, False)):
        want = torch.float32 if f32 else torch.bfloat16
        for o in (ops.decode_ex(q, k, k, lens, 0.125, True, 100, s, cap, f32),
                  ops.decode_paged_ex(q, pool, pool, table, None, 0.125, False, 0, s, cap, f32),
                  ops.decode_fp8_ex(q, k8, k8, sc, None, lens, 0.125, True, 64, s, cap, f32),
                  ops.decode_paged_fp8_ex(q, pool8, pool8, table, sc, sc, lens, 0.125, True, 0, s, cap, f32)):
            assert o.shape == q.shape and o.dtype == want and o.device.type == "meta"
    for name, base in (("decode_ex", "decode_window"), ("decode_paged_ex", "decode_paged_window"), ("decode_fp8_ex", "decode_fp8_window"),
                       ("decode_paged_fp8_ex", "decode_paged_fp8_window")):
        ex = [(a.name, str(a.type)) for a in getattr(ops, name).default._schema.arguments]
        win = [(a.name, str(a.type)) for a in getattr(ops, base).default._schema.arguments]
        i = [n for n, _ in win].index("window") + 1
        assert ex == win[:i] + [("sinks", "Optional[Tensor]"), ("softcap", "float")] + win[i:], name
    c = torch.zeros(1, 1, 64, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.decode_ex(c, c, c, None, 0.125, False, 0, None, 1.0, True)
