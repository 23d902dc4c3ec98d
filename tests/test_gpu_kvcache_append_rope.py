"""GPU tier of the rotary append entries (fa_kvcache_append_rope, _paged_rope, _fp8_rope, _paged_fp8_rope).

Every check is an equality of bytes against tests/rope_inputs.py, the numpy restatement of the pinned arithmetic (stepwise fp32, no
fused multiply-add, one rounding into the 16-bit type or the e4m3fn recipe on the fp32 value) -- never against the code under test
and never against the plain entries.  Caches, pools and Q start as seeded random bytes and are compared WHOLE.

Common shape, the append tier's: B = 6, Hkv = 2, Ncap = 128 with the lengths (0, 17, 123, 128, -3, 1000), as a contiguous cache and as
pages of 16 and of 64 keys.  Sequences 3 and 5 are full: all their tokens are dropped, and their Q rows are rotated all the same.
"""
import functools

import numpy as np
import pytest

import append_inputs as ai
import common_inputs as cm
import decode_inputs as di
import fp8_inputs as f8
import rope_inputs as ri
import test_gpu_kvcache_append as ta

pytestmark = pytest.mark.gpu

B, HKV, NCAP, LENS = ta.B, ta.HKV, ta.NCAP, ta.LENS
FMT_D, LAYOUTS = ta.FMT_D, ta.LAYOUTS
K_SCALES, V_SCALES = ta.K_SCALES, ta.V_SCALES
NNEWS, GS = (1, 5, 37), (1, 3)
MAX_POS = 165   # 128 + 37: no position of the common shape reaches the table's clamp


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _scrambled(max_pos, half, seed=11):
    cos, sin = ri.scrambled_table(max_pos, half, seed)
    cos.setflags(write=False), sin.setflags(write=False)
    return cos, sin


def _finite(bits, fmt):
    """random encodings with inf and NaN taken out (the exponent's lowest bit cleared where the exponent is all ones)"""
    emask, low = (0x7C00, 0x0400) if fmt == 0 else (0x7F80, 0x0080)
    return np.where((bits & emask) == emask, bits ^ low, bits).astype(np.uint16)


def _sources(shape, fmt, rot_dim, seed):
    """rows of random bits: finite in the rotated part, anything (NaN payloads included) in the pass-through part"""
    bits = ai.random_bytes(shape, 2, seed)
    bits[..., :rot_dim] = _finite(bits[..., :rot_dim], fmt)
    return bits


def _f32(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


class _Case(ta._Case):
    def rope_append(self, fa, dk_new, dv_new, dlens, cos, sin, interleaved, q=None, q_out=None, out=None, k_scale=None, v_scale=None):
        torch = self.torch
        kw = dict(cache_seqlens=dlens, seqlens_out=out, q=q, q_out=q_out, rotary_cos=_f32(torch, cos), rotary_sin=_f32(torch, sin),
                  rotary_interleaved=interleaved)
        if self.fp8:
            kw.update(k_scale=k_scale, v_scale=v_scale)
        name = "fa_kvcache_append" + ("_paged" if self.ps else "") + ("_fp8" if self.fp8 else "")
        args = (dk_new, dv_new, self.dk, self.dv) + ((self.dtable,) if self.ps else ())
        assert getattr(fa, name)(*args, **kw) is None
        torch.cuda.synchronize()


def _run16(fa, torch, fmt, d, ps, nnew, G, rot_dim, interleaved, max_pos, seed, lens=LENS, table_edit=None, q_mode="in place"):
    """One 16-bit rotary append on the common shape, checked whole: K cache against the rotated rows placed by append_inputs, V cache
    against the plain copy, Q against its rotation (dropped tokens' rows included)."""
    case = _Case(torch, d, fmt, ps, nnew, seed, lens=lens, table_edit=table_edit)
    cos, sin = _scrambled(max_pos, rot_dim // 2)
    k_new = _sources((B, HKV, nnew, d), fmt, rot_dim, seed + 3)
    v_new = ai.random_bytes((B, HKV, nnew, d), 2, seed + 4)
    q = _sources((B, HKV * G, nnew, d), fmt, rot_dim, seed + 5)
    want_k = ri.rotated_rows16(k_new, fmt, lens, NCAP, cos, sin, interleaved)
    want_q = ri.rotated_rows16(q, fmt, lens, NCAP, cos, sin, interleaved)
    assert not np.array_equal(want_k[..., :rot_dim], k_new[..., :rot_dim]) and np.array_equal(want_k[..., rot_dim:], k_new[..., rot_dim:])
    want_kc, want_vc = case.expected(want_k, v_new, lens)
    dq = cm.dev16(torch, q, fmt)
    dq_out = {"in place": None, "separate": cm.dev16(torch, ai.random_bytes(q.shape, 2, seed + 6), fmt), "absent": None}[q_mode]
    dlens = None if lens is None else ta._ints(torch, lens)
    case.rope_append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), dlens, cos, sin, interleaved,
                     q=None if q_mode == "absent" else dq, q_out=dq_out)
    what = f"d={d} ps={ps} Nnew={nnew} G={G} rot={rot_dim} il={interleaved} q {q_mode}"
    case.check(want_kc, want_vc, what)
    if q_mode == "separate":
        assert ta._bytes_equal(torch, dq, q), f"{what}: the source q changed"
        assert ta._bytes_equal(torch, dq_out, want_q), f"{what}: q_out differs"
    else:
        assert ta._bytes_equal(torch, dq, q if q_mode == "absent" else want_q), f"{what}: q differs"
    return case


# ---- 1. the bytes of K, V and Q -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nnew", NNEWS)
@pytest.mark.parametrize("rot", ["16", "d/2", "d"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half-split", "interleaved"])
@pytest.mark.parametrize("ps", LAYOUTS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_rope_append_bytes(fa, torch_cuda, fmt, d, ps, interleaved, rot, nnew, G):
    """The whole product d x format x layout x convention x rot_dim x Nnew x G (a case takes some 10 ms).  Scrambled table of 165
    rows: no clamp.  5 fits exactly behind length 123; 37 crosses two page boundaries from 17 and is cut short at 123."""
    rot_dim = {"16": 16, "d/2": d // 2, "d": d}[rot]
    _run16(fa, torch_cuda, fmt, d, ps, nnew, G, rot_dim, interleaved, MAX_POS, seed=1000 * d + 100 * ps + 10 * nnew + fmt + G)


@pytest.mark.parametrize("ps", LAYOUTS)
def test_null_lengths_rotate_from_position_zero(fa, torch_cuda, ps):
    _run16(fa, torch_cuda, 1, 128, ps, 21, 2, 64, False, MAX_POS, seed=31 + ps, lens=None)


# ---- 2. the table's clamp -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [False, True], ids=["half-split", "interleaved"])
@pytest.mark.parametrize("ps", LAYOUTS)
def test_positions_past_the_table_use_its_last_row(fa, torch_cuda, ps, interleaved):
    """max_pos = 100: positions 100 .. 127 of sequence 2 (123 + t) and the dropped tokens' Q rows (128 + t) use row 99."""
    nnew = 37
    rows = ri.table_rows(ri.positions(LENS, B, NCAP, nnew), 100)
    assert rows[2].tolist() == [99] * nnew and rows[3].tolist() == [99] * nnew and rows[1].max() == 53
    _run16(fa, torch_cuda, 0 if interleaved else 1, 128, ps, nnew, 3, 128 if ps else 64, interleaved, 100, seed=7000 + ps)


# ---- 3. Q in place, into q_out, absent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_mode", ["in place", "separate", "absent"])
@pytest.mark.parametrize("ps", LAYOUTS)
def test_q_in_place_separate_and_absent(fa, torch_cuda, ps, q_mode):
    for interleaved in (False, True):
        _run16(fa, torch_cuda, 0, 64, ps, 5, 3, 32, interleaved, MAX_POS, seed=8000 + ps, q_mode=q_mode)


def test_q_overlap_is_refused(fa, torch_cuda):
    torch = torch_cuda
    case = _Case(torch, 64, 0, 0, 1, seed=5)
    cos, sin = ri.identity_table(8, 8)
    new = cm.dev16(torch, ai.random_bytes((B, HKV, 1, 64), 2, 1), 0)
    buf = torch.zeros(B * HKV * 64 + 64, dtype=torch.float16, device="cuda")
    before = case.dk.view(torch.int16).clone()
    with pytest.raises(fa.FaError) as err:
        case.rope_append(fa, new, new, None, cos, sin, False, q=buf[:-64].view(B, HKV, 1, 64), q_out=buf[64:].view(B, HKV, 1, 64))
    assert err.value.code == 1
    torch.cuda.synchronize()
    assert torch.equal(case.dk.view(torch.int16), before) and int(torch.count_nonzero(buf)) == 0


# ---- 4. dropped tokens and bad live table entries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1, "num_pages + 5"])
@pytest.mark.parametrize("ps", [16, 64])
def test_bad_live_table_entries_drop_k_and_v_but_rotate_q(fa, torch_cuda, ps, bad):
    """The entry of a page that should receive tokens is out of range: the pool is unchanged for those tokens and right for the rest;
    entries of pages no kept token reaches hold garbage (make_table) and are not read; every Q row is rotated."""
    nnew = 37
    victims = [(1, 32 // ps), (0, 0), (2, 7 * 16 // ps)]
    assert all(v in ai.written_pages(LENS, B, NCAP, nnew, ps) for v in victims)
    lost = []

    def edit(table, num_pages):
        for (b, pi) in victims:
            lost.append(int(table[b, pi]))
            table[b, pi] = -1 if bad == -1 else num_pages + 5

    for interleaved in (False, True):
        del lost[:]
        case = _run16(fa, torch_cuda, 1, 64, ps, nnew, 3, 64, interleaved, MAX_POS, seed=900 + ps, table_edit=edit)
        got = case.dk.view(torch_cuda.int16).cpu().numpy().view(np.uint16)
        for page in lost:
            assert np.array_equal(got[page], case.k0[page])


# ---- 5. inputs a fused multiply-add gets wrong --------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [False, True], ids=["half-split", "interleaved"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_contraction_witnesses_get_the_pinned_bytes(fa, torch_cuda, fmt, interleaved):
    """128 (x1, x2, c, s) on which fma(x1, c, -x2*s) or fma(-x2, s, x1*c) rounds to another 16-bit value than the stepwise
    expression, as K and as Q: a kernel the compiler contracted fails here on every pair."""
    torch = torch_cuda
    d, rot_dim = 64, 16
    rows, cos, sin = ri.witness_case(fmt, d, rot_dim, interleaved)
    nnew = rows.shape[2]
    want = ri.rotated_rows16(rows, fmt, (0,), 32, cos, sin, interleaved)
    i1, i2 = ri.pair_slices(rot_dim, interleaved)
    x = ai.widen16(rows, fmt)[0, 0]
    for form, contracted in enumerate(ri.contracted_y1(x[:, i1], x[:, i2], cos, sin)):
        sl = slice(0, nnew // 2) if form == 0 else slice(nnew // 2, nnew)
        assert (ai.round16_bits(contracted, fmt)[sl] != want[0, 0][:, i1][sl]).all()
    k0 = ai.random_bytes((1, 1, 32, d), 2, 3)
    dk, dv = cm.dev16(torch, k0, fmt), cm.dev16(torch, k0, fmt)
    dnew, dq = cm.dev16(torch, rows, fmt), cm.dev16(torch, rows, fmt)
    fa.fa_kvcache_append(dnew, dnew, dk, dv, q=dq, rotary_cos=_f32(torch, cos), rotary_sin=_f32(torch, sin),
                         rotary_interleaved=interleaved)
    torch.cuda.synchronize()
    got = dk.view(torch.int16).cpu().numpy().view(np.uint16)
    wrong = int((got[0, 0, :nnew][:, i1] != want[0, 0][:, i1]).sum())
    print(f"witness pairs with other bytes than the pinned arithmetic: {wrong} of {nnew * rot_dim // 2}")
    assert ta._bytes_equal(torch, dk, ai.expected_contiguous(k0, want, None)), "K"
    assert ta._bytes_equal(torch, dv, ai.expected_contiguous(k0, rows, None)), "V"
    assert ta._bytes_equal(torch, dq, want), "Q"


# ---- 6. fp8 caches ------------------------------------------------------------------------------------------------------------------
def _quantized_f32(fa, torch, y, scales):
    """fa.quantize_kv_fp8 on the CPU of fp32 rows [B, Hkv, Nnew, d] -> uint8 codes"""
    s = torch.tensor(list(scales) if scales is not None else [1.0] * y.shape[1], dtype=torch.float32)
    return fa.quantize_kv_fp8(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)), s)[0].view(torch.uint8).numpy()


def _normal_rows(shape, fmt, seed, scale=3.0):
    return ai.round16_bits(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale, fmt)


@pytest.mark.parametrize("with_scales", [True, False], ids=["scales", "null-scales"])
@pytest.mark.parametrize("ps", LAYOUTS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_fp8_rope_append_is_the_recipe_on_the_fp32_value(fa, torch_cuda, fmt, d, ps, with_scales):
    """K codes = quantize_kv_fp8 (CPU) of the fp32 rotated value -- no 16-bit rounding in between --, pass-through elements and V as
    the plain fp8 entry quantises them, Q rotated in 16 bit."""
    torch = torch_cuda
    nnew, G = 37, 3
    interleaved = bool((d // 64 + fmt + ps // 16) % 2)
    rot_dim = d // 2 if with_scales else d
    ks, vs = (K_SCALES, V_SCALES) if with_scales else (None, None)
    mag = (0.02, 0.01) if with_scales else (3.0, 3.0)
    cos, sin = _scrambled(MAX_POS, rot_dim // 2)
    k_new, v_new = _normal_rows((B, HKV, nnew, d), fmt, 51, 100 * mag[0]), _normal_rows((B, HKV, nnew, d), fmt, 52, 100 * mag[1])
    q = _sources((B, HKV * G, nnew, d), fmt, rot_dim, 53)
    y = ri.rotated_rows_fp32(k_new, fmt, LENS, NCAP, cos, sin, interleaved)
    k8, v8 = _quantized_f32(fa, torch, y, ks), _quantized_f32(fa, torch, ai.widen16(v_new, fmt), vs)
    assert np.array_equal(k8, ri.fp8_codes(y, ks))
    y16 = ai.widen16(ri.rotated_rows16(k_new, fmt, LENS, NCAP, cos, sin, interleaved), fmt)
    print(f"codes the unfused path (a 16-bit rounding first) would store differently: {int((ri.fp8_codes(y16, ks) != k8).sum())}")
    case = _Case(torch, d, fmt, ps, nnew, seed=500 + d + ps, fp8=True)
    want_k, want_v = case.expected(k8, v8)
    dq = cm.dev16(torch, q, fmt)
    case.rope_append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), ta._ints(torch, LENS), cos, sin, interleaved, q=dq,
                     k_scale=ta._scales(torch, ks), v_scale=ta._scales(torch, vs))
    got_k = case.dk.view(torch.uint8).cpu().numpy()
    print(f"fp8 K bytes differing: {int((got_k != want_k).sum())} of {want_k.size}")
    case.check(want_k, want_v, f"fp8 rope ps={ps} scales={with_scales}")
    assert ta._bytes_equal(torch, dq, ri.rotated_rows16(q, fmt, LENS, NCAP, cos, sin, interleaved)), "Q"


@pytest.mark.parametrize("interleaved", [False, True], ids=["half-split", "interleaved"])
@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="p16")])
@pytest.mark.parametrize("fmt", [0, 1], ids=["fp16", "bf16"])
def test_fp8_every_code_and_tie_through_the_rope_kernels(fa, torch_cuda, fmt, ps, interleaved):
    """The identity table and append_inputs.fp8_new_rows: every e4m3fn magnitude, every midpoint and the values beyond 448, times the
    head's scale, go through the rotation (x*1 -+ x'*0) and the quantisation; the bytes are the restatement's."""
    torch = torch_cuda
    d, nnew = 64, 37
    cos, sin = ri.identity_table(MAX_POS, d // 2)
    k_new = ai.fp8_new_rows(B, HKV, nnew, d, K_SCALES, fmt, seed=41)
    v_new = ai.fp8_new_rows(B, HKV, nnew, d, V_SCALES, fmt, seed=42)
    y = ri.rotated_rows_fp32(k_new, fmt, LENS, NCAP, cos, sin, interleaved)
    k8, v8 = ri.fp8_codes(y, K_SCALES), _quantized_f32(fa, torch, ai.widen16(v_new, fmt), V_SCALES)
    assert np.array_equal(k8, _quantized_f32(fa, torch, y, K_SCALES))
    for h in range(HKV):   # sequence 0 keeps all 37 tokens: every finite code is demanded of both heads
        assert set(k8[0][h].ravel().tolist()) == set(f8.FINITE_CODES.tolist())
    case = _Case(torch, d, fmt, ps, nnew, seed=600 + ps, fp8=True)
    want_k, want_v = case.expected(k8, v8)
    case.rope_append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), ta._ints(torch, LENS), cos, sin, interleaved,
                     k_scale=ta._scales(torch, K_SCALES), v_scale=ta._scales(torch, V_SCALES))
    case.check(want_k, want_v, f"fp8 identity ps={ps}")


# ---- 7. seqlens_out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS)
def test_rope_seqlens_out(fa, torch_cuda, ps, fp8):
    """A separate buffer and the in-place form both receive min(clamp(L) + Nnew, Ncap); with None the lengths are untouched; the
    cache and Q are the same in all three (the rotation saw the OLD lengths)."""
    torch = torch_cuda
    fmt, d, nnew, rot_dim = 0, 64, 5, 64
    cos, sin = _scrambled(MAX_POS, rot_dim // 2)
    k_new, v_new, q = (_normal_rows((B, HKV, nnew, d), fmt, s) for s in (3, 4, 5))
    y = ri.rotated_rows_fp32(k_new, fmt, LENS, NCAP, cos, sin, False)
    if fp8:
        src_k, src_v = _quantized_f32(fa, torch, y, None), _quantized_f32(fa, torch, ai.widen16(v_new, fmt), None)
    else:
        src_k, src_v = ri.rotated_rows16(k_new, fmt, LENS, NCAP, cos, sin, False), v_new
    want_q = ri.rotated_rows16(q, fmt, LENS, NCAP, cos, sin, False)
    want_lens = ta._ints(torch, ai.lens_after(LENS, B, nnew, NCAP))
    for mode in ("separate", "in place", "none"):
        case = _Case(torch, d, fmt, ps, nnew, seed=77 + ps, fp8=fp8)
        dlens, dq = ta._ints(torch, LENS), cm.dev16(torch, q, fmt)
        out = {"separate": torch.full((B,), -7, dtype=torch.int32, device="cuda"), "in place": dlens, "none": None}[mode]
        case.rope_append(fa, cm.dev16(torch, k_new, fmt), cm.dev16(torch, v_new, fmt), dlens, cos, sin, False, q=dq, out=out)
        case.check(*case.expected(src_k, src_v), mode)
        assert ta._bytes_equal(torch, dq, want_q), mode
        if mode == "none":
            assert dlens.tolist() == list(LENS)
        else:
            assert torch.equal(out, want_lens), (mode, out.tolist())
            assert mode == "in place" or dlens.tolist() == list(LENS)


# ---- 8. a captured step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous-16bit", "p16-fp8"])
def test_captured_rope_append_then_decode_follows_a_growing_cache(fa, oracle, torch_cuda, layout):
    """append(rotary_cos=..., q=..., seqlens_out = lens, in place) -> fa_forward_kvcache(causal), Nnew = 1, captured once on one
    stream and replayed for three steps with k_new, v_new and q rewritten in place: O of every step and the caches at the end EQUAL
    eager decodes of caches assembled on the host from host-rotated rows, with host-rotated q."""
    torch = torch_cuda
    fp8 = layout == "p16-fp8"
    ps, fmt, d, G = (16 if fp8 else 0), (1 if fp8 else 0), 64, 2
    steps = 3
    cos, sin = ri.real_table(NCAP + steps, d)
    (q_all, k_all, v_all), (qb, kb, vb) = di.inputs(oracle, B, HKV, G, steps + 1, NCAP + steps + 1, d, fmt, 6200 + fmt)
    kb4, vb4 = kb.reshape(B, HKV, -1, d), vb.reshape(B, HKV, -1, d)
    qb4 = qb.reshape(B, HKV * G, -1, d)
    ks, vs = ((1.0, 0.37), (1.9, 0.5)) if fp8 else (None, None)

    def stored_v(bits):
        return _quantized_f32(fa, torch, ai.widen16(bits, fmt), vs) if fp8 else np.array(bits)

    def stored_k(bits, lens_h):   # rotated at the positions the lengths give; the start cache is stored as it is
        if lens_h is None:
            return _quantized_f32(fa, torch, ai.widen16(bits, fmt), ks) if fp8 else np.array(bits)
        if fp8:
            return _quantized_f32(fa, torch, ri.rotated_rows_fp32(bits, fmt, lens_h, NCAP, cos, sin, False), ks)
        return ri.rotated_rows16(bits, fmt, lens_h, NCAP, cos, sin, False)

    k0, v0 = stored_k(kb4[:, :, :NCAP], None), stored_v(vb4[:, :, :NCAP])
    if ps:
        table, num_pages = ai.make_table(LENS, B, NCAP, steps, ps, seed=9)
        pool_k = ai.expected_paged(np.zeros((num_pages, HKV, ps, d), k0.dtype), k0, None, table)
        pool_v = ai.expected_paged(np.zeros((num_pages, HKV, ps, d), v0.dtype), v0, None, table)
        host_k, host_v = pool_k, pool_v
        dtable = torch.from_numpy(table).cuda()
    else:
        host_k, host_v = k0, v0
    to_dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    dscale = dict(k_scale=ta._scales(torch, ks), v_scale=ta._scales(torch, vs)) if fp8 else {}
    dcos, dsin = _f32(torch, cos), _f32(torch, sin)
    ws = torch.empty(max(fa.kvcache_workspace_bytes(B, HKV, G, 1, NCAP, d), 1), dtype=torch.uint8, device="cuda")

    def append(dkn, dvn, dq, dk, dv, lens):
        kw = dict(cache_seqlens=lens, seqlens_out=lens, q=dq, rotary_cos=dcos, rotary_sin=dsin, **dscale)
        if fp8:
            fa.fa_kvcache_append_paged_fp8(dkn, dvn, dk, dv, dtable, **kw)
        else:
            fa.fa_kvcache_append(dkn, dvn, dk, dv, **kw)

    def decode(dq, dk, dv, lens):
        if fp8:
            return fa.fa_forward_kvcache_paged_fp8(dq, dk, dv, dtable, cache_seqlens=lens, causal=True, workspace=ws, **dscale)
        return fa.fa_forward_kvcache(dq, dk, dv, lens, causal=True, workspace=ws)

    def new_rows(step):
        return kb4[:, :, NCAP + step:NCAP + step + 1], vb4[:, :, NCAP + step:NCAP + step + 1], qb4[:, :, step:step + 1]

    want, lens_h = [], list(LENS)
    for step in range(steps):
        kn, vn, qn = new_rows(step)
        place = (lambda c, n: ai.expected_paged(c, n, lens_h, table)) if ps else (lambda c, n: ai.expected_contiguous(c, n, lens_h))
        host_k, host_v = place(host_k, stored_k(kn, lens_h)), place(host_v, stored_v(vn))
        q_rot = ri.rotated_rows16(qn, fmt, lens_h, NCAP, cos, sin, False)
        lens_h = list(ai.lens_after(lens_h, B, 1, NCAP))
        o = decode(cm.dev16(torch, q_rot, fmt), to_dev(host_k), to_dev(host_v), ta._ints(torch, lens_h))
        torch.cuda.synchronize()
        assert torch.isfinite(o).all()
        want.append((o.clone(), q_rot, list(lens_h)))
    assert want[0][2] == [1, 18, 124, 128, 1, 128] and not torch.equal(want[0][0], want[1][0])

    dk, dv = to_dev(pool_k if ps else k0), to_dev(pool_v if ps else v0)
    dlens = ta._ints(torch, LENS)
    kn, vn, qn = new_rows(0)
    dkn, dvn, dq = cm.dev16(torch, kn, fmt), cm.dev16(torch, vn, fmt), cm.dev16(torch, qn, fmt)
    scratch_k, scratch_v, scratch_lens, scratch_q = dk.clone(), dv.clone(), dlens.clone(), dq.clone()
    append(dkn, dvn, scratch_q, scratch_k, scratch_v, scratch_lens)
    decode(scratch_q, scratch_k, scratch_v, scratch_lens)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        append(dkn, dvn, dq, dk, dv, dlens)
        o = decode(dq, dk, dv, dlens)
    assert dlens.tolist() == list(LENS)   # a capture runs nothing
    for step in range(steps):
        kn, vn, qn = new_rows(step)
        dkn.copy_(cm.dev16(torch, kn, fmt)), dvn.copy_(cm.dev16(torch, vn, fmt)), dq.copy_(cm.dev16(torch, qn, fmt))
        ws.fill_(0xFF), o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eo, q_rot, lens_want = want[step]
        assert dlens.tolist() == lens_want, (step, dlens.tolist())
        assert ta._bytes_equal(torch, dq, q_rot), f"step {step}: q"
        assert torch.equal(o, eo), f"step {step}"
    assert ta._bytes_equal(torch, dk, host_k) and ta._bytes_equal(torch, dv, host_v)
