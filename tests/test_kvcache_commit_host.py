"""CPU tier of fa_kvcache_commit through the C ABI: the symbol is exported, declared and bound, the ctypes structure mirrors the header
under the C compiler, every refusal the header lists holds before the device is touched, the Python front end checks shapes and dtypes,
the torch op registers, and tree_accept_mask gives the words of tree_from_parents' trees.  Only calls that must be rejected are issued,
so the file is safe where a GPU is visible."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_kvcache_append_host as base
import test_kvcache_append_varlen_host as appendv
import tree_inputs as ti

INVALID = 1  # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fa_kvcache_commit"
KINDS = ("", "paged_", "fp8_", "paged_fp8_")
FIELDS = ["size", "K", "V", "seqlens_k", "seqlens_out", "accept_mask", "block_table", "kv_dtype", "dtype", "B", "Hkv", "d", "max_new", "Ncap",
          "num_pages", "page_size", "max_pages", "stream"]
WORDS = 1 << 12   # a made-up device address with the alignment the entry asks for


def _desc(fa, kind="", **kw):
    """a descriptor with small made-up addresses that WOULD be launched; test_kvcache_append_host's keyword names where they exist"""
    names = dict(k="K", v="V", lens="seqlens_k", out="seqlens_out", table="block_table", dt="dtype", words="accept_mask")
    f = dict(K=16, V=16, accept_mask=WORDS, B=1, Hkv=1, d=64, max_new=64, dtype=0)
    if "paged" in kind:
        f.update(block_table=16, num_pages=8, page_size=16, max_pages=12)
    else:
        f.update(Ncap=192)
    if "fp8" in kind:
        f.update(kv_dtype=fa.capi.KV_FP8_E4M3)
    for k, v in kw.items():
        f[names.get(k, k)] = v
    if "paged" in kind:
        f.pop("Ncap", None)
    return fa.capi.KvCommitDesc(**f)


def _call(fa, kind="", **kw):
    return getattr(fa.lib(), NAME)(ctypes.byref(_desc(fa, kind, **kw)))


def test_symbol_struct_and_declaration(fa):
    raw = ctypes.CDLL(fa.capi.LIB_PATH)
    sym = fa.capi.SYMBOLS
    assert NAME in sym and hasattr(raw, NAME)
    assert NAME not in sym[:9] and NAME not in sym[-2:]   # between the head slice and the pinned tail
    fn = getattr(fa.lib(), NAME)
    S = fa.capi.KvCommitDesc
    assert fn.argtypes == [ctypes.POINTER(S)] and fn.restype is ctypes.c_int
    assert appendv._header_fields("fa_kvcommit_desc") == [f[0] for f in S._fields_] == FIELDS
    assert S().size == ctypes.sizeof(S) == fa.capi.new_desc(S).size
    header = appendv._header()
    assert "int fa_kvcache_commit(const fa_kvcommit_desc* desc);" in header
    # the tree step's entries no longer list the commit by copies as missing, and point here
    assert "the commit after verification" not in header and header.count(NAME + ", below") >= 2
    assert "a commit by page-table edits" in header and "moving rows between sequences" in header
    for name in ("fa_kvcache_commit", "tree_accept_mask"):
        assert name in fa.__all__ and callable(getattr(fa, name))


def test_layout_matches_the_c_compiler(fa, tmp_path):
    src = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(fa_kvcommit_desc, {n})" for n in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fa_mi355.h"\nint main(void) { size_t o[] = {sizeof(fa_kvcommit_desc), '
                   + offs + '}; for (size_t i = 0; i < sizeof o / sizeof *o; ++i) printf("%zu\\n", o[i]); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = fa.capi.KvCommitDesc
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in FIELDS]


COMMON = [
    dict(size=0), dict(size=8), dict(size=512), dict(kv_dtype=2), dict(kv_dtype=-1),
    dict(k=0), dict(v=0), dict(words=0),
    dict(words=WORDS + 1), dict(words=WORDS + 2), dict(words=WORDS + 4), dict(words=WORDS + 7),   # 8-byte words
    dict(max_new=0), dict(max_new=-1), dict(max_new=65), dict(max_new=1 << 20),
    dict(B=0), dict(B=-1), dict(Hkv=0), dict(Hkv=-2),
    dict(d=32), dict(d=96), dict(d=256), dict(d=0), dict(dt=2), dict(dt=-1),
    dict(B=1 << 16, Hkv=1 << 16),                                                        # B * Hkv beyond int
    # seqlens_out overlapping seqlens_k without being it (B = 4: 16 bytes each)
    dict(B=4, lens=1 << 16, out=(1 << 16) + 4), dict(B=4, lens=1 << 16, out=(1 << 16) + 12), dict(B=4, lens=1 << 16, out=(1 << 16) - 12),
    # accept_mask (B = 4: 32 bytes) overlapping seqlens_out (16 bytes), with and without seqlens_k = seqlens_out
    dict(B=4, words=1 << 16, out=1 << 16), dict(B=4, words=1 << 16, out=(1 << 16) + 28), dict(B=4, words=1 << 16, out=(1 << 16) - 12),
    dict(B=4, words=1 << 16, out=(1 << 16) + 16, lens=(1 << 16) + 16), dict(B=4, words=(1 << 16) + 8, out=1 << 16, lens=1 << 16),
]


@pytest.mark.parametrize("kind", KINDS)
def test_rejections(fa, kind):
    L = fa.lib()
    assert getattr(L, NAME)(None) == INVALID
    assert _call(fa, kind, size=ctypes.sizeof(fa.capi.KvCommitDesc) - 8) == INVALID
    assert _call(fa, kind, size=ctypes.sizeof(fa.capi.KvAppendDesc)) == INVALID
    for bad in COMMON + (base.PAGED if "paged" in kind else base.CONTIG):
        assert _call(fa, kind, **bad) == INVALID, (kind, bad)


def test_python_front_end_checks(fa):
    torch = pytest.importorskip("torch")
    f16, i32, i64 = torch.float16, torch.int32, torch.int64
    cache = torch.zeros(3, 2, 32, 64, dtype=f16)
    pool = torch.zeros(9, 2, 16, 128, dtype=torch.bfloat16)
    cache8 = cache.to(torch.float8_e4m3fn)
    words, lens, table = torch.zeros(3, dtype=i64), torch.zeros(3, dtype=i32), torch.zeros(3, 2, dtype=i32)
    commit = fa.fa_kvcache_commit
    bad = [
        (lambda: commit(cache.float(), cache.float(), words), "fp16"),
        (lambda: commit(cache, cache8, words), "fp16"),
        (lambda: commit(cache[0], cache[0], words), "Hkv,Ncap,d"),
        (lambda: commit(cache, cache[:, :1], words), "Hkv,Ncap,d"),
        (lambda: commit(cache[..., :32], cache[..., :32], words), "64 or 128"),
        (lambda: commit(cache, cache, words.int()), "int64"),
        (lambda: commit(cache, cache, [0, 0, 0]), "int64"),
        (lambda: commit(cache, cache, words[:2]), r"\[B\] = \[3\]"),
        (lambda: commit(cache, cache, torch.zeros(6, dtype=i64)[::2]), r"\[B\] = \[3\]"),
        (lambda: commit(pool, pool, words, block_table=table[0]), "block_table"),
        (lambda: commit(pool, pool, words[:2], block_table=table), r"\[B\] = \[3\]"),
        (lambda: commit(torch.zeros(9, 2, 24, 64, dtype=f16), torch.zeros(9, 2, 24, 64, dtype=f16), words, block_table=table), "power of two"),
        (lambda: commit(cache, cache, words, cache_seqlens=lens[:2]), "cache_seqlens"),
        (lambda: commit(cache, cache, words, seqlens_out=lens.long()), "seqlens_out"),
        (lambda: commit(cache, cache, words, max_new=0), "1..64"),
        (lambda: commit(cache, cache, words, max_new=65), "1..64"),
        (lambda: commit(cache, cache, words, max_new=8.0), "1..64"),
    ]
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
    # a call that is right in shape and dtype still has no CPU path
    for call in (lambda: commit(cache, cache, words, lens, lens), lambda: commit(cache8, cache8, words, max_new=8),
                 lambda: commit(pool, pool, words, lens, None, table)):
        with pytest.raises(ValueError, match="must be a device tensor"):
            call()


def test_custom_op_registers(fa):
    """the op exists after register(), traces on meta tensors, mutates what it says, returns nothing and has no CPU kernel"""
    torch = pytest.importorskip("torch")
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    meta = dict(device="meta")
    cache = torch.empty(3, 2, 500, 128, dtype=torch.bfloat16, **meta)
    pool8 = torch.empty(40, 2, 32, 128, dtype=torch.float8_e4m3fn, **meta)
    words, lens = torch.empty(3, dtype=torch.int64, **meta), torch.empty(3, dtype=torch.int32, **meta)
    table = torch.empty(3, 16, dtype=torch.int32, **meta)
    assert ops.commit(cache, cache, words, lens, lens, None, 64) is None
    assert ops.commit(pool8, pool8, words, None, None, table, 8) is None
    schema = ops.commit.default._schema
    assert [a.name for a in schema.arguments] == ["k_cache", "v_cache", "accept_mask", "cache_seqlens", "seqlens_out", "block_table", "max_new"]
    mutated = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert mutated == {"k_cache", "v_cache", "seqlens_out"} and len(schema.returns) == 0
    c = torch.zeros(1, 1, 64, 64, dtype=torch.float16)
    with pytest.raises(Exception):   # no CPU implementation: the product path is the HIP library only
        ops.commit(c, c.clone(), torch.zeros(1, dtype=torch.int64), None, None, None, 64)


def test_tree_accept_mask(fa):
    """the word of each sequence's last accepted token, against tree_from_parents' words and tree_inputs' own walk of the chains"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9960)
    n = [13, 64, 0, 5, 1]
    cu = np.cumsum([2] + n)
    total = int(cu[-1]) + 3
    parents = np.full(total, -1, np.int32)
    for b, m in enumerate(n):
        parents[cu[b]:cu[b + 1]] = ti.parents_of("random", m, rng) if m else []
    dcu = torch.tensor(cu, dtype=torch.int32)
    mask, _ = fa.tree_from_parents(torch.from_numpy(parents), dcu)
    last = [12, 63, -1, 2, 0]
    got = fa.tree_accept_mask(mask, dcu, torch.tensor(last, dtype=torch.int32))
    assert got.dtype == torch.int64 and got.shape == (len(n),)
    for b, m in enumerate(n):
        if last[b] < 0:
            assert int(got[b]) == 0
            continue
        words, depth = ti.closed_masks([int(p) for p in parents[cu[b]:cu[b + 1]]])
        want = words[last[b]]
        assert int(got[b]) & ((1 << 64) - 1) == want, b
        assert bin(want).count("1") == depth[last[b]] + 1 and want >> last[b] == 1, "the node's bit is the word's highest"
    assert int(got[1]) < 0, "bit 63 is the sign bit of the int64 word"
    # int64 `last` and cu; an index outside the tensor clamps, -1 wins over it
    assert torch.equal(fa.tree_accept_mask(mask, dcu.long(), torch.tensor(last)), got)
    far = fa.tree_accept_mask(mask, dcu, torch.tensor([10 ** 6, -1, -1, -1, -10 ** 6]))
    assert int(far[0]) == int(mask[-1]) and far[1:].tolist() == [0, 0, 0, 0]
    for bad, what in ((mask.int(), "int64"), (mask[None], "int64"), (mask[:0], "non-empty")):
        with pytest.raises(ValueError, match=what):
            fa.tree_accept_mask(bad, dcu, torch.tensor(last))
    with pytest.raises(ValueError, match=r"\(B,\)"):
        fa.tree_accept_mask(mask, dcu, torch.tensor(last[:3]))
    with pytest.raises(ValueError, match="B\\+1"):
        fa.tree_accept_mask(mask, dcu[:1], torch.tensor(last))
