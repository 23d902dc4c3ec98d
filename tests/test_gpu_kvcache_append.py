"""GPU tier of the KV-cache append entries (fa_kvcache_append, _paged, _fp8, _paged_fp8).

Every check is an equality of bytes.  The 16-bit entries copy, so the cache after an append must EQUAL the cache tests/append_inputs.py
assembles by plain indexing; the fp8 entries quantise as fa.quantize_kv_fp8 does, so their bytes must equal that recipe run by torch
on the CPU and placed by the same helper.  Caches and pools start as seeded random bytes (K distinct from V) and are compared WHOLE:
a stray or misplaced store anywhere shows, as does a dropped token that was written after all.

Common shape: B = 6, Hkv = 2, Ncap = 128 with the lengths (0, 17, 123, 128, -3, 1000) -- empty, mid-page, nearly full, full, clamped up,
clamped down -- as a contiguous cache and as pages of 16 and of 64 keys, scattered through a pool with spare pages and garbage in the
table entries no token reaches.
"""
import numpy as np
import pytest

import append_inputs as ai
import common_inputs as cm
import decode_inputs as di
import fp8_inputs as f8

pytestmark = pytest.mark.gpu

B, HKV, NCAP = ai.SHAPE["B"], ai.SHAPE["Hkv"], ai.SHAPE["Ncap"]
LENS = ai.LENS
FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
LAYOUTS = [pytest.param(0, id="contiguous"), pytest.param(16, id="p16"), pytest.param(64, id="p64")]
K_SCALES, V_SCALES = (1.0, 0.37), (1.9, 0.5)   # per head, all different: a wrong head index shows


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _ints(torch, values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _scales(torch, values):
    return None if values is None else torch.tensor(list(values), dtype=torch.float32, device="cuda")


def _bytes_equal(torch, dev, want):
    """the device tensor's raw bytes against a numpy array of the same bytes, whole"""
    raw = dev.view(torch.int16 if dev.element_size() == 2 else torch.uint8)
    want = np.ascontiguousarray(want)
    want_t = torch.from_numpy(want.view(np.int16) if want.itemsize == 2 else want).cuda()
    return raw.shape == want_t.shape and torch.equal(raw, want_t)


def _quantized_cpu(fa, torch, bits, fmt, scales):
    """fa.quantize_kv_fp8 on the CPU: new rows [B, Hkv, Nnew, d] (uint16 encodings) -> uint8 codes"""
    x = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(_tdtype(torch, fmt))
    s = torch.tensor(list(scales) if scales is not None else [1.0] * bits.shape[1], dtype=torch.float32)
    x8, _ = fa.quantize_kv_fp8(x, s)
    return x8.view(torch.uint8).numpy()


class _Case:
    """Start state of one append: K and V caches (ps = 0) or pools and a table, of seeded random bytes, on the host and the device."""

    def __init__(self, torch, d, fmt, ps, nnew, seed, fp8=False, lens=LENS, table_edit=None):
        self.torch, self.ps, self.fp8, self.fmt, self.lens = torch, ps, fp8, fmt, lens
        size = 1 if fp8 else 2
        if ps == 0:
            self.table, shape = None, (B, HKV, NCAP, d)
        else:
            self.table, num_pages = ai.make_table(lens, B, NCAP, nnew, ps, seed)
            if table_edit is not None:
                table_edit(self.table, num_pages)
            shape = (num_pages, HKV, ps, d)
        self.k0, self.v0 = ai.random_bytes(shape, size, seed + 1), ai.random_bytes(shape, size, seed + 2)
        to_dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
        self.dk, self.dv = to_dev(self.k0), to_dev(self.v0)
        self.dtable = None if ps == 0 else torch.from_numpy(self.table).cuda()

    def append(self, fa, dk_new, dv_new, dlens, out=None, k_scale=None, v_scale=None):
        kw = dict(cache_seqlens=dlens, seqlens_out=out)
        if self.fp8:
            kw.update(k_scale=k_scale, v_scale=v_scale)
        name = "fa_kvcache_append" + ("_paged" if self.ps else "") + ("_fp8" if self.fp8 else "")
        args = (dk_new, dv_new, self.dk, self.dv) + ((self.dtable,) if self.ps else ())
        assert getattr(fa, name)(*args, **kw) is None
        self.torch.cuda.synchronize()

    def expected(self, k_new, v_new, lens="same"):
        lens = self.lens if lens == "same" else lens
        if self.ps == 0:
            return ai.expected_contiguous(self.k0, k_new, lens), ai.expected_contiguous(self.v0, v_new, lens)
        return ai.expected_paged(self.k0, k_new, lens, self.table), ai.expected_paged(self.v0, v_new, lens, self.table)

    def check(self, want_k, want_v, what):
        assert _bytes_equal(self.torch, self.dk, want_k), f"{what}: K differs"
        assert _bytes_equal(self.torch, self.dv, want_v), f"{what}: V differs"


# ---- 1. exact copy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnew", [1, 5, 37])
@pytest.mark.parametrize("ps", LAYOUTS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_append_is_an_exact_copy(fa, torch_cuda, fmt, d, ps, nnew):
    """Random 16-bit patterns (NaN payloads among them) land bit for bit where the helper puts them and nowhere else.  5 fits exactly
    behind length 123; 37 crosses two page boundaries from 17 and is cut short at 123; lengths 128 and 1000 write nothing."""
    torch = torch_cuda
    case = _Case(torch, d, fmt, ps, nnew, seed=100 * d + 10 * ps + nnew)
    k_new, v_new = ai.random_bytes((B, HKV, nnew, d), 2, 7 + nnew), ai.random_bytes((B, HKV, nnew, d), 2, 8 + nnew)
    want_k, want_v = case.expected(k_new, v_new)
    if ps == 0:
        assert np.array_equal(want_k[[3, 5]], case.k0[[3, 5]])   # the full sequences: nothing fits
    assert not np.array_equal(want_k, case.k0) and not np.array_equal(want_k, want_v)
    case.append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), _ints(torch, LENS))
    case.check(want_k, want_v, f"Nnew={nnew} ps={ps}")


@pytest.mark.parametrize("ps", LAYOUTS)
def test_append_null_lengths_is_a_prefill(fa, torch_cuda, ps):
    """cache_seqlens = None: every sequence is empty (not full, as None means to the decode entries)"""
    torch = torch_cuda
    fmt, d, nnew = 1, 128, 21
    case = _Case(torch, d, fmt, ps, nnew, seed=31 + ps, lens=None)
    k_new, v_new = ai.random_bytes((B, HKV, nnew, d), 2, 1), ai.random_bytes((B, HKV, nnew, d), 2, 2)
    case.append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), None)
    case.check(*case.expected(k_new, v_new), f"prefill ps={ps}")


# ---- 2. bad live table entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1, "num_pages + 5"])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_bad_live_table_entries_drop_their_tokens(fa, torch_cuda, fmt, d, ps, bad):
    """The entry of a page that should receive tokens is out of range: the pool is unchanged for those tokens, right for the rest."""
    torch = torch_cuda
    nnew = 37
    victims = [(1, 32 // ps), (0, 0), (2, 7 * 16 // ps)]   # the page of positions 32.. of sequence 1; sequence 0's first; sequence 2's last
    assert all(v in ai.written_pages(LENS, B, NCAP, nnew, ps) for v in victims)
    lost = []

    def edit(table, num_pages):
        for (b, pi) in victims:
            lost.append(int(table[b, pi]))
            table[b, pi] = -1 if bad == -1 else num_pages + 5

    case = _Case(torch, d, fmt, ps, nnew, seed=900 + d + ps, table_edit=edit)
    k_new, v_new = ai.random_bytes((B, HKV, nnew, d), 2, 11), ai.random_bytes((B, HKV, nnew, d), 2, 12)
    want_k, want_v = case.expected(k_new, v_new)
    for page in lost:   # the pages the tokens would have reached are as they were
        assert np.array_equal(want_k[page], case.k0[page]) and np.array_equal(want_v[page], case.v0[page])
    assert not np.array_equal(want_k, case.k0)
    case.append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), _ints(torch, LENS))
    case.check(want_k, want_v, f"bad entry {bad} ps={ps}")


# ---- 3. fp8 exactness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_scales", [True, False], ids=["scales", "null-scales"])
@pytest.mark.parametrize("ps", LAYOUTS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_fp8_append_is_quantize_kv_fp8(fa, torch_cuda, fmt, d, ps, with_scales):
    """Sources built from every e4m3fn magnitude, every midpoint between two of them and values beyond 448, both signs, times the
    head's scale: the stored bytes equal fa.quantize_kv_fp8 on the CPU, code for code, for per-head scales and for NULL scales."""
    torch = torch_cuda
    nnew = 37
    ks, vs = (K_SCALES, V_SCALES) if with_scales else (None, None)
    k_new = ai.fp8_new_rows(B, HKV, nnew, d, ks or (1.0, 1.0), fmt, seed=41)
    v_new = ai.fp8_new_rows(B, HKV, nnew, d, vs or (1.0, 1.0), fmt, seed=42)
    k8, v8 = _quantized_cpu(fa, torch, k_new, fmt, ks), _quantized_cpu(fa, torch, v_new, fmt, vs)
    for codes in (k8[0], v8[0]):   # sequence 0 keeps all 37 tokens: every finite code is demanded of both heads, and no NaN code
        for h in range(HKV):
            assert set(codes[h].ravel().tolist()) == set(f8.FINITE_CODES.tolist())
    case = _Case(torch, d, fmt, ps, nnew, seed=500 + d + ps, fp8=True)
    want_k, want_v = case.expected(k8, v8)
    case.append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), _ints(torch, LENS), k_scale=_scales(torch, ks),
                v_scale=_scales(torch, vs))
    got_k = case.dk.view(torch.uint8).cpu().numpy()
    print(f"fp8 K bytes differing: {int((got_k != want_k).sum())} of {want_k.size}")
    case.check(want_k, want_v, f"fp8 ps={ps} scales={with_scales}")


@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_fp8_append_of_inf_and_nan(fa, torch_cuda, fmt):
    """+-inf saturates to +-448 (0x7E / 0xFE); a NaN source becomes a NaN code (0x7F or 0xFF); finite neighbours are untouched."""
    torch = torch_cuda
    d, nnew = 64, 2
    dt = _tdtype(torch, fmt)
    row = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.0, -2.0, 448.0, -448.0, 0.0] * (d // 8), dtype=dt)
    neg_nan = torch.tensor([-1], dtype=torch.int16).view(dt)   # 0xFFFF: a NaN with the sign bit set
    new = row.repeat(1, 1, nnew, 1).contiguous()
    new[0, 0, 1, 3] = neg_nan[0]
    cache = cm.dev8(torch, ai.random_bytes((1, 1, 16, d), 1, 5))
    before = cache.view(torch.uint8).clone()
    vcache = cache.clone()
    for scale in (None, torch.tensor([0.37], dtype=torch.float32, device="cuda")):
        fa.fa_kvcache_append_fp8(new.cuda(), new.cuda(), cache, vcache, k_scale=scale, v_scale=scale,
                                 cache_seqlens=_ints(torch, [3]))
        torch.cuda.synchronize()
        got = cache.view(torch.uint8).cpu().numpy()[0, 0]
        assert np.array_equal(got[:3], before.cpu().numpy()[0, 0, :3]) and np.array_equal(got[5:], before.cpu().numpy()[0, 0, 5:])
        assert torch.equal(cache.view(torch.uint8), vcache.view(torch.uint8))
        for t in (3, 4):
            r = got[t].reshape(-1, 8)
            assert (r[:, 0] == 0x7E).all() and (r[:, 1] == 0xFE).all(), r[0]
            assert ((r[:, 2] & 0x7F) == 0x7F).all(), r[0]
            assert (r[:, 5] == 0x7E).all() and (r[:, 6] == 0xFE).all() and (r[:, 7] == 0x00).all(), r[0]
            if scale is None:
                assert (r[:, 4] == f8.encode(np.float32(-2.0))).all()
        assert got[3, 3] == f8.encode(np.float32(1.0) / np.float32(1.0 if scale is None else 0.37))
        assert got[4, 3] & 0x7F == 0x7F   # the negative NaN


# ---- 4. seqlens_out ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS)
def test_seqlens_out(fa, torch_cuda, ps, fp8):
    """A separate buffer and the in-place form both receive min(clamp(L) + Nnew, Ncap); with None the lengths are untouched; the cache
    is the same in all three; a partial overlap is refused."""
    torch = torch_cuda
    fmt, d, nnew = 0, 64, 5
    k_new, v_new = ai.random_bytes((B, HKV, nnew, d), 2, 3), ai.random_bytes((B, HKV, nnew, d), 2, 4)
    k_new, v_new = k_new & 0x3FFF, v_new & 0x3FFF   # finite, so that the fp8 form has a CPU reference
    dk_new, dv_new = cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt)
    want_lens = _ints(torch, ai.lens_after(LENS, B, nnew, NCAP))
    assert want_lens.tolist() == [5, 22, 128, 128, 5, 128]
    src_k, src_v = (_quantized_cpu(fa, torch, k_new, fmt, None), _quantized_cpu(fa, torch, v_new, fmt, None)) if fp8 else (k_new, v_new)
    for mode in ("separate", "in place", "none"):
        case = _Case(torch, d, fmt, ps, nnew, seed=77 + ps, fp8=fp8)
        dlens = _ints(torch, LENS)
        out = {"separate": torch.full((B,), -7, dtype=torch.int32, device="cuda"), "in place": dlens, "none": None}[mode]
        case.append(fa, dk_new, dv_new, dlens, out=out)
        case.check(*case.expected(src_k, src_v), mode)
        if mode == "none":
            assert dlens.tolist() == list(LENS)
        else:
            assert torch.equal(out, want_lens), (mode, out.tolist())
            assert mode == "in place" or dlens.tolist() == list(LENS)
    # no lengths in: every sequence is empty, so every length out is min(Nnew, Ncap)
    case = _Case(torch, d, fmt, ps, nnew, seed=78 + ps, fp8=fp8, lens=None)
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    case.append(fa, dk_new, dv_new, None, out=out)
    assert out.tolist() == [nnew] * B
    case.check(*case.expected(src_k, src_v), "null lengths")
    buf = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    before = case.dk.view(torch.uint8).clone() if fp8 else case.dk.view(torch.int16).clone()
    with pytest.raises(fa.FaError) as err:
        case.append(fa, dk_new, dv_new, buf[:B], out=buf[1:])
    assert err.value.code == 1
    torch.cuda.synchronize()
    assert torch.equal(case.dk.view(before.dtype), before) and buf.tolist() == [0] * (B + 1)


# ---- 5. stream order and graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous-16bit", "p16-fp8"])
def test_captured_append_then_decode_follows_a_growing_cache(fa, oracle, torch_cuda, layout):
    """append(seqlens_out = lens, in place) -> decode(lens), captured once and replayed for three steps with k_new, v_new and q
    rewritten in place: O and lse of every step EQUAL the eager decode on a cache assembled on the host for that step."""
    torch = torch_cuda
    fp8 = layout == "p16-fp8"
    ps, fmt, d, G = (16 if fp8 else 0), (1 if fp8 else 0), 64, 2
    steps = 3
    (q_all, k_all, v_all), (qb, kb, vb) = di.inputs(oracle, B, HKV, G, steps + 1, NCAP + steps + 1, d, fmt, 6100 + fmt)
    # start caches: finite values in every row, so that O can be compared with torch.equal; new rows: the tail of the same draw
    kb4, vb4 = kb.reshape(B, HKV, -1, d), vb.reshape(B, HKV, -1, d)
    qb4 = qb.reshape(B, HKV * G, -1, d)
    ks, vs = ((1.0, 0.37), (1.9, 0.5)) if fp8 else (None, None)

    def stored(bits, scales):   # what the cache holds for 16-bit rows: the rows themselves, or their codes
        return _quantized_cpu(fa, torch, bits, fmt, scales) if fp8 else np.array(bits)

    k0, v0 = stored(kb4[:, :, :NCAP], ks), stored(vb4[:, :, :NCAP], vs)
    if ps:
        table, num_pages = ai.make_table(LENS, B, NCAP, steps, ps, seed=9)
        # the start caches dealt into the live pages (lengths None: all 128 rows are placed; dead entries drop theirs)
        pool_k = ai.expected_paged(np.zeros((num_pages, HKV, ps, d), k0.dtype), k0, None, table)
        pool_v = ai.expected_paged(np.zeros((num_pages, HKV, ps, d), v0.dtype), v0, None, table)
        host_k, host_v = pool_k, pool_v
        dtable = torch.from_numpy(table).cuda()
    else:
        host_k, host_v = k0, v0
    to_dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    dscale = dict(k_scale=_scales(torch, ks), v_scale=_scales(torch, vs)) if fp8 else {}
    ws = torch.empty(max(fa.kvcache_workspace_bytes(B, HKV, G, 1, NCAP, d), 1), dtype=torch.uint8, device="cuda")

    def append(dkn, dvn, dk, dv, lens):
        if fp8:
            fa.fa_kvcache_append_paged_fp8(dkn, dvn, dk, dv, dtable, cache_seqlens=lens, seqlens_out=lens, **dscale)
        else:
            fa.fa_kvcache_append(dkn, dvn, dk, dv, cache_seqlens=lens, seqlens_out=lens)

    def decode(dq, dk, dv, lens):
        if fp8:
            return fa.fa_forward_kvcache_paged_fp8(dq, dk, dv, dtable, cache_seqlens=lens, return_lse=True, workspace=ws, **dscale)
        return fa.fa_forward_kvcache(dq, dk, dv, lens, return_lse=True, workspace=ws)

    def new_rows(step):
        return kb4[:, :, NCAP + step:NCAP + step + 1], vb4[:, :, NCAP + step:NCAP + step + 1], qb4[:, :, step:step + 1]

    # the reference of every step: the cache assembled on the host, decoded eagerly
    want, lens_h = [], list(LENS)
    for step in range(steps):
        kn, vn, qn = new_rows(step)
        place = (lambda c, n: ai.expected_paged(c, n, lens_h, table)) if ps else (lambda c, n: ai.expected_contiguous(c, n, lens_h))
        host_k, host_v = place(host_k, stored(kn, ks)), place(host_v, stored(vn, vs))
        lens_h = list(ai.lens_after(lens_h, B, 1, NCAP))
        o, lse = decode(cm.dev16(torch, qn, fmt), to_dev(host_k), to_dev(host_v), _ints(torch, lens_h))
        torch.cuda.synchronize()
        assert torch.isfinite(o).all()
        want.append((o.clone(), lse.clone(), list(lens_h)))
    assert want[0][2] == [1, 18, 124, 128, 1, 128] and not torch.equal(want[0][0], want[1][0])

    # the device side: one warm-up of both calls on scratch state, then the capture on the real state
    dk, dv = to_dev(pool_k if ps else k0), to_dev(pool_v if ps else v0)
    dlens = _ints(torch, LENS)
    kn, vn, qn = new_rows(0)
    dkn, dvn, dq = cm.dev16(torch, kn, fmt), cm.dev16(torch, vn, fmt), cm.dev16(torch, qn, fmt)
    scratch_k, scratch_v, scratch_lens = dk.clone(), dv.clone(), dlens.clone()
    append(dkn, dvn, scratch_k, scratch_v, scratch_lens)
    decode(dq, scratch_k, scratch_v, scratch_lens)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        append(dkn, dvn, dk, dv, dlens)
        o, lse = decode(dq, dk, dv, dlens)
    assert dlens.tolist() == list(LENS)   # a capture runs nothing
    for step in range(steps):
        kn, vn, qn = new_rows(step)
        dkn.copy_(cm.dev16(torch, kn, fmt)), dvn.copy_(cm.dev16(torch, vn, fmt)), dq.copy_(cm.dev16(torch, qn, fmt))
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eo, el, lens_want = want[step]
        assert dlens.tolist() == lens_want, (step, dlens.tolist())
        assert torch.equal(o, eo) and torch.equal(lse, el), f"step {step}"
    assert _bytes_equal(torch, dk, host_k) and _bytes_equal(torch, dv, host_v)


# ---- 6. 64-bit page addresses -----------------------------------------------------------------------------------------------------
def test_page_addresses_are_64_bit(fa, torch_cuda):
    """Pools of 65 600 pages of 256 keys at d = 128 (4.3 GB each), zero-filled; the new token goes to page 65 590.  That page, its two
    neighbours and its 32-bit alias (page 65 590 - 65 536) are compared on the device: only the target row may change."""
    torch = torch_cuda
    num_pages, ps, d, target, row = 65600, 256, 128, 65590, 44
    alias = target - 65536
    assert num_pages * ps * d * 2 > 1 << 32 and (target * ps * d * 2) % (1 << 32) == alias * ps * d * 2
    pools = [torch.zeros(num_pages, 1, ps, d, dtype=torch.float16, device="cuda") for _ in range(2)]
    table = torch.tensor([[3, target, -1, 1 << 30]], dtype=torch.int32, device="cuda")
    new = [cm.dev16(torch, ai.random_bytes((1, 1, 1, d), 2, s) | 1, 0) for s in (1, 2)]   # | 1: no element is zero
    fa.fa_kvcache_append_paged(new[0], new[1], pools[0], pools[1], table, cache_seqlens=_ints(torch, [ps + row]))
    torch.cuda.synchronize()
    for pool, src in zip(pools, new):
        raw = pool.view(torch.int16)
        assert torch.equal(raw[target, 0, row], src.view(torch.int16)[0, 0, 0])
        assert int(torch.count_nonzero(raw[target])) == d
        for page in (target - 1, target + 1, alias, 3, 0, num_pages - 1):
            assert int(torch.count_nonzero(raw[page])) == 0, page
        assert int(torch.count_nonzero(pool.view(torch.int64))) == d // 4   # the whole pool: nothing else anywhere


# ---- 7. the one lengths kernel, past one block ------------------------------------------------------------------------------------
LENS_B, LENS_CAP, LENS_NNEW, LENS_D = 257, 8, 2, 64
LENS_IN = np.array([(-3, 0, 5, 7, 8, 100)[b % 6] for b in range(LENS_B)], dtype=np.int64)
LENS_CNT = np.array([(-1, 0, 1, 2, 9)[b % 5] for b in range(LENS_B)], dtype=np.int64)


@pytest.mark.parametrize("entry", ["flat", "seqlens_new", "varlen", "mla"])
def test_lengths_past_one_block(fa, torch_cuda, entry):
    """B = 257: the lengths kernel that serves the flat append, the append with seqlens_new, fa_kvcache_append_varlen and fa_mla_append
    runs a second 256-thread block with one live thread.  Lengths (-3, 0, 5, 7, 8, 100) and counts (-1, 0, 1, 2, 9) cycle with
    coprime periods, capacity 8, Nnew 2: the lengths out EQUAL minimum(clip(L, 0, 8) + m, 8), into a separate buffer and in place, and
    the whole cache -- sequence 256 named -- is the source rows at their slots and untouched elsewhere, bit for bit."""
    torch = torch_cuda
    Bn, cap, nnew, d = LENS_B, LENS_CAP, LENS_NNEW, LENS_D
    width = 576 if entry == "mla" else d
    start = np.clip(LENS_IN, 0, cap)
    m = np.full(Bn, nnew) if entry == "flat" else np.clip(LENS_CNT, 0, nnew)
    want_lens = np.minimum(start + m, cap)
    assert want_lens[256] == cap and len(set(want_lens.tolist())) >= 3   # several lengths, and the last one at the capacity
    cu = np.concatenate([[0], np.cumsum(np.clip(LENS_CNT, 0, nnew))])
    packed = entry in ("varlen", "mla")
    k0, v0 = ai.random_bytes((Bn, 1, cap, width), 2, 71), ai.random_bytes((Bn, 1, cap, width), 2, 72)
    src_shape = (int(cu[-1]), 1, width) if packed else (Bn, 1, nnew, width)
    k_new, v_new = ai.random_bytes(src_shape, 2, 73), ai.random_bytes(src_shape, 2, 74)
    want_k, want_v = k0.copy(), v0.copy()
    for b in range(Bn):
        for i in range(int(m[b])):
            p = int(start[b]) + i
            if p < cap:
                want_k[b, 0, p] = k_new[cu[b] + i, 0] if packed else k_new[b, 0, i]
                want_v[b, 0, p] = v_new[cu[b] + i, 0] if packed else v_new[b, 0, i]
    assert not np.array_equal(want_k, k0) and np.array_equal(want_k[256], k0[256])   # sequence 256 is full: 256 % 6 == 4, L = 8
    dk_new, dv_new = cm.dev16(torch, k_new, 0), cm.dev16(torch, v_new, 0)
    dcu, dcnt = _ints(torch, cu), _ints(torch, LENS_CNT)
    for mode in ("separate", "in place"):
        dk, dv = cm.dev16(torch, k0, 0), cm.dev16(torch, v0, 0)
        dlens = _ints(torch, LENS_IN)
        out = torch.full((Bn,), -7, dtype=torch.int32, device="cuda") if mode == "separate" else dlens
        if entry == "flat":
            fa.fa_kvcache_append(dk_new, dv_new, dk, dv, cache_seqlens=dlens, seqlens_out=out)
        elif entry == "seqlens_new":
            fa.fa_kvcache_append(dk_new, dv_new, dk, dv, cache_seqlens=dlens, seqlens_out=out, seqlens_new=dcnt)
        elif entry == "varlen":
            fa.fa_kvcache_append_varlen(dk_new, dv_new, dk, dv, dcu, cache_seqlens=dlens, seqlens_out=out)
        else:
            fa.fa_mla_append(dk_new[:, 0], dk[:, 0], dcu, cache_seqlens=dlens, seqlens_out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        print(f"{entry} {mode}: lengths differing {int((got != want_lens).sum())} of {Bn}; last {int(got[256])} want {int(want_lens[256])}")
        assert np.array_equal(got, want_lens), (entry, mode, np.nonzero(got != want_lens)[0].tolist())
        assert mode == "in place" or dlens.tolist() == LENS_IN.tolist()
        assert _bytes_equal(torch, dk[256], want_k[256]), f"{entry} {mode}: sequence 256 of K differs"
        assert _bytes_equal(torch, dk, want_k), f"{entry} {mode}: K differs"
        if entry != "mla":
            assert _bytes_equal(torch, dv[256], want_v[256]), f"{entry} {mode}: sequence 256 of V differs"
            assert _bytes_equal(torch, dv, want_v), f"{entry} {mode}: V differs"
