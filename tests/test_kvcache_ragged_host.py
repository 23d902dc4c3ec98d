"""CPU tier of the per-sequence counts of the KV-cache step: `seqlens_q` of fa_kvcache_decode and the descriptor append entry
fa_kvcache_append_ex with `seqlens_new`.  The symbols are exported and bound, both ctypes structures mirror the header, the old
decode descriptor size is still taken, every rejection of the append descriptor and of the flat entries behind it holds before the
device is touched, the Python front ends check the two vectors, and the eight _ragged ops register.  Only calls that must be
rejected are issued, so the file is safe where a GPU is visible."""
import ctypes
import os
import re

import pytest

import test_kvcache_append_host as base
import test_kvcache_append_rope_host as rope
import test_kvcache_logits_host as logits

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p


def _header_fields(struct):
    text = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1), flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if decl.strip()]


def test_symbols_and_structs(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    L = fa.lib()
    for n in ("fa_kvcache_decode", "fa_kvcache_append_ex"):
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
    assert "fa_kvcache_append_ex" not in fa.capi.SYMBOLS[:9] and "fa_kvcache_append_ex" not in fa.capi.SYMBOLS[-2:]
    assert L.fa_kvcache_append_ex.argtypes == [ctypes.POINTER(fa.capi.KvAppendDesc)] and L.fa_kvcache_append_ex.restype is ctypes.c_int
    # both ctypes structures name the header's fields in the header's order; seqlens_q is the decode descriptor's LAST field
    dec, app = _header_fields("fa_kvdecode_desc"), _header_fields("fa_kvappend_desc")
    assert dec == [f[0] for f in fa.capi.KvDecodeDesc._fields_] and dec[-1] == "seqlens_q" and dec[-2] == "stream"
    assert app == [f[0] for f in fa.capi.KvAppendDesc._fields_]
    assert app == ["size", "Knew", "Vnew", "K", "V", "seqlens_k", "seqlens_out", "seqlens_new", "block_table", "k_scale", "v_scale", "Q",
                   "Qout", "rope_cos", "rope_sin", "kv_dtype", "B", "Hkv", "Nnew", "d", "Ncap", "num_pages", "page_size", "max_pages", "G",
                   "rot_dim", "max_pos", "interleaved", "dtype", "stream"]
    assert fa.capi.KvAppendDesc().size == ctypes.sizeof(fa.capi.KvAppendDesc)
    assert fa.capi.KvDecodeDesc().size == ctypes.sizeof(fa.capi.KvDecodeDesc) == fa.capi.KvDecodeDesc.seqlens_q.offset + 8
    header = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    assert "int fa_kvcache_append_ex(const fa_kvappend_desc* desc);" in header and "not part of this entry" in header.lower()


# ---- decode: the descriptor's size and the new field ------------------------------------------------------------------------------
def test_old_descriptor_size_is_still_taken(fa):
    L = fa.lib()
    old = fa.capi.KvDecodeDesc.seqlens_q.offset          # offsetof(fa_kvdecode_desc, seqlens_q): the structure before the field
    new = ctypes.sizeof(fa.capi.KvDecodeDesc)
    assert old == new - ctypes.sizeof(ctypes.c_void_p)
    some = 0
    for kind in logits.KINDS:
        for kw in (dict(Ncap=8192), dict(Ncap=32768, window=1024, B=3, G=2, Nq=5, d=128), dict(Ncap=200)):
            if "paged" in kind:
                kw = dict({k: v for k, v in kw.items() if k != "Ncap"}, max_pages=kw["Ncap"] // 16, page_size=16)
            want = L.fa_kvcache_decode_workspace_bytes(ctypes.byref(logits._desc(fa, kind, **kw)))
            assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(logits._desc(fa, kind, size=old, **kw))) == want
            # the field is ignored by the sizing function
            assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(logits._desc(fa, kind, seqlens_q=16, **kw))) == want
            some += want > 0
    assert some >= 4
    for bad in (0, 8, 512, old - 8, old + 4, new + 8):
        d = logits._desc(fa, Ncap=8192, size=bad)
        assert L.fa_kvcache_decode_workspace_bytes(ctypes.byref(d)) == 0 and L.fa_kvcache_decode(ctypes.byref(d)) == INVALID, bad
    # a split without a workspace is turned away whichever size names the structure, with and without the field
    for kw in (dict(size=old), dict(size=new), dict(seqlens_q=16), dict(size=old, seqlens_q=16)):
        assert logits._call(fa, Ncap=8192, **kw) == INVALID, kw


@pytest.mark.parametrize("kind", logits.KINDS)
def test_decode_rejections_hold_with_seqlens_q(fa, kind):
    for bad in (logits.PAGED if "paged" in kind else logits.CONTIG):
        assert logits._call(fa, kind, seqlens_q=16, **bad) == INVALID, (kind, bad)
    if "fp8" not in kind:
        assert logits._call(fa, kind, seqlens_q=16, k_scale=16) == INVALID


# ---- append: the descriptor ---------------------------------------------------------------------------------------------------------
def _adesc(fa, kind="", **kw):
    """a descriptor with small made-up addresses that WOULD be launched; base._call's keyword names"""
    names = dict(knew="Knew", vnew="Vnew", k="K", v="V", lens="seqlens_k", out="seqlens_out", table="block_table", ks="k_scale",
                 vs="v_scale", q="Q", qout="Qout", cos="rope_cos", sin="rope_sin", il="interleaved", dt="dtype", new="seqlens_new")
    f = dict(Knew=16, Vnew=16, K=16, V=16, B=1, Hkv=1, Nnew=1, d=64, dtype=0)
    if "paged" in kind:
        f.update(block_table=16, num_pages=8, page_size=16, max_pages=12)
    else:
        f.update(Ncap=192)
    if "fp8" in kind:
        f.update(kv_dtype=fa.capi.KV_FP8_E4M3)
    if "rope" in kind:
        f.update(Q=4096, Qout=4096, rope_cos=16, rope_sin=16, G=1, rot_dim=64, max_pos=8, interleaved=0)
    for k, v in kw.items():
        v = v.value if isinstance(v, ctypes.c_void_p) else v
        f[names.get(k, k)] = v
    if "paged" in kind:
        f.pop("Ncap", None)
    return fa.capi.KvAppendDesc(**f)


def _acall(fa, kind="", **kw):
    return fa.lib().fa_kvcache_append_ex(ctypes.byref(_adesc(fa, kind, **kw)))


KINDS = ("", "paged_", "fp8_", "paged_fp8_", "rope", "paged_rope", "fp8_rope", "paged_fp8_rope")


def test_append_descriptor_rejections(fa):
    L = fa.lib()
    assert L.fa_kvcache_append_ex(None) == INVALID
    for kind in KINDS:
        for new in (None, 8192):
            for bad in (dict(size=0), dict(size=8), dict(size=512), dict(size=ctypes.sizeof(fa.capi.KvAppendDesc) - 8), dict(kv_dtype=2),
                        dict(kv_dtype=-1)):
                assert _acall(fa, kind, new=new, **bad) == INVALID, (kind, bad)
            if "fp8" not in kind:   # a 16-bit cache has no scales
                assert _acall(fa, kind, new=new, ks=16) == INVALID and _acall(fa, kind, new=new, vs=16) == INVALID
            if "rope" not in kind:  # arguments of the rotary forms without a table
                for bad in (dict(q=4096, qout=4096), dict(q=4096), dict(qout=4096), dict(sin=16)):
                    assert _acall(fa, kind, new=new, **bad) == INVALID, (kind, bad)
        # seqlens_new must not overlap seqlens_out: identity, partial overlaps, and with seqlens_out == seqlens_k (B = 4: 16 bytes)
        for cnt, out in ((4096, 4096), (4096, 4100), (4096, 4108), (4108, 4096)):
            assert _acall(fa, kind, B=4, new=cnt, out=out) == INVALID, (kind, cnt, out)
            assert _acall(fa, kind, B=4, new=cnt, out=out, lens=out) == INVALID, (kind, cnt, out)


@pytest.mark.parametrize("kind", KINDS)
def test_append_descriptor_rejects_what_the_flat_entry_rejects(fa, kind):
    """every case of the flat entries' CPU tiers, with and without seqlens_new"""
    cases = base.COMMON + (base.PAGED if "paged" in kind else base.CONTIG)
    if "rope" in kind:
        cases = cases + [c for c in rope.ROPE if c.get("cos", 1) != 0]   # cos = 0 names the plain form here
    for bad in cases:
        for new in (None, 8192):
            assert _acall(fa, kind, new=new, **bad) == INVALID, (kind, bad, new)
    if "rope" in kind:
        assert _acall(fa, kind, sin=0) == INVALID and _acall(fa, kind, sin=0, new=8192) == INVALID


# ---- the Python front ends ------------------------------------------------------------------------------------------------------------
def test_python_checks_on_the_two_vectors(fa):
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd import ops
    cpu = torch.device("cpu")
    good = torch.zeros(3, dtype=torch.int32)
    for name in ("seqlens_q", "seqlens_new"):
        assert ops._counts_ptr(None, name, 3, cpu) is None
        for bad in (good.long(), good.float(), [0, 0, 0]):
            with pytest.raises(ValueError, match="int32"):
                ops._counts_ptr(bad, name, 3, cpu)
        for bad in (good[:2], torch.zeros(4, dtype=torch.int32), torch.zeros(3, 1, dtype=torch.int32)):
            with pytest.raises(ValueError, match="per sequence"):
                ops._counts_ptr(bad, name, 3, cpu)
        with pytest.raises(ValueError, match="contiguous"):
            ops._counts_ptr(torch.zeros(6, dtype=torch.int32)[::2], name, 3, cpu)
        with pytest.raises(ValueError, match="is on"):
            ops._counts_ptr(good, name, 3, torch.device("meta"))
        with pytest.raises(ValueError, match=name + " must be a device tensor"):
            ops._counts_ptr(good, name, 3, cpu)          # everything else in order: the HIP path has no CPU fallback
    # the eight front ends take the keywords and still refuse CPU tensors
    q = torch.zeros(2, 4, 3, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.float16)
    k8, pool8 = k.to(torch.float8_e4m3fn), pool.to(torch.float8_e4m3fn)
    table = torch.zeros(2, 5, dtype=torch.int32)
    n = torch.zeros(2, dtype=torch.int32)
    new = torch.zeros(2, 2, 3, 64, dtype=torch.float16)
    cos = torch.zeros(8, 32)
    for call in (lambda **kw: fa.fa_forward_kvcache(q, k, k, **kw), lambda **kw: fa.fa_forward_kvcache_paged(q, pool, pool, table, **kw),
                 lambda **kw: fa.fa_forward_kvcache_fp8(q, k8, k8, **kw), lambda **kw: fa.fa_forward_kvcache_paged_fp8(q, pool8, pool8, table, **kw)):
        with pytest.raises(ValueError):
            call(seqlens_q=n)
        with pytest.raises(ValueError):
            call(seqlens_q=n, window=5, softcap=1.0)
    for call in (lambda **kw: fa.fa_kvcache_append(new, new, k, k, **kw), lambda **kw: fa.fa_kvcache_append_paged(new, new, pool, pool, table, **kw),
                 lambda **kw: fa.fa_kvcache_append_fp8(new, new, k8, k8, **kw),
                 lambda **kw: fa.fa_kvcache_append_paged_fp8(new, new, pool8, pool8, table, **kw)):
        with pytest.raises(ValueError):
            call(seqlens_new=n)
        with pytest.raises(ValueError):
            call(seqlens_new=n, q=q, rotary_cos=cos, rotary_sin=cos)


def test_ragged_custom_ops_register(fa):
    """the eight _ragged ops exist after register(), trace on meta tensors, have no CPU kernel, and have the schemas the _ex and _rope
    ops have with the one argument more (and the rotary arguments optional)"""
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
    new = torch.empty(2, 2, 3, 128, dtype=torch.bfloat16, device="meta")
    cos = torch.empty(64, 64, dtype=torch.float32, device="meta")
    for nq, s, f32 in ((lens, sinks, True), (None, None, False), (lens, None, False)):
        want = torch.float32 if f32 else torch.bfloat16
        for o in (ops.decode_ragged(q, k, k, lens, nq, 0.125, True, 100, s, 0.0, f32),
                  ops.decode_paged_ragged(q, pool, pool, table, None, nq, 0.125, False, 0, s, 1.0, f32),
                  ops.decode_fp8_ragged(q, k8, k8, sc, None, lens, nq, 0.125, True, 64, s, 0.0, f32),
                  ops.decode_paged_fp8_ragged(q, pool8, pool8, table, sc, sc, lens, nq, 0.125, True, 0, s, 0.0, f32)):
            assert o.shape == q.shape and o.dtype == want and o.device.type == "meta"
    for rot in ((q, cos, cos), (None, cos, cos), (None, None, None)):
        assert ops.append_ragged(new, new, k, k, lens, lens, lens, *rot, False) is None
        assert ops.append_paged_ragged(new, new, pool, pool, table, lens, None, lens, *rot, True) is None
        assert ops.append_fp8_ragged(new, new, k8, k8, sc, None, None, lens, None, *rot, False) is None
        assert ops.append_paged_fp8_ragged(new, new, pool8, pool8, table, sc, sc, lens, lens, lens, *rot, False) is None

    def args(name):
        return [(a.name, str(a.type)) for a in getattr(ops, name).default._schema.arguments]

    for form in ("", "_paged", "_fp8", "_paged_fp8"):
        ex, rg = args("decode" + form + "_ex"), args("decode" + form + "_ragged")
        i = [n for n, _ in ex].index("cache_seqlens") + 1
        assert rg == ex[:i] + [("seqlens_q", "Optional[Tensor]")] + ex[i:], form
        rp, ra = args("append" + form + "_rope"), args("append" + form + "_ragged")
        i = [n for n, _ in rp].index("seqlens_out") + 1
        opt = {"rotary_cos": "Optional[Tensor]", "rotary_sin": "Optional[Tensor]"}
        assert ra == rp[:i] + [("seqlens_new", "Optional[Tensor]")] + [(n, opt.get(n, t)) for n, t in rp[i:]], form
        schema = getattr(ops, "append" + form + "_ragged").default._schema
        mutated = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
        assert mutated == {"k_pool" if "paged" in form else "k_cache", "v_pool" if "paged" in form else "v_cache", "seqlens_out", "q"}
        assert len(schema.returns) == 0
    c = torch.zeros(1, 1, 64, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.decode_ragged(c, c, c, None, None, 0.125, False, 0, None, 0.0, True)
    with pytest.raises(Exception):
        ops.append_ragged(c[:, :, :1], c[:, :, :1].clone(), c, c.clone(), None, None, None, None, None, None, False)
