"""GPU tier of the MLA entries fa_mla_decode and fa_mla_append (fa.fa_mla_decode, fa.fa_mla_append, torch.ops.fa_mi355.mla_*).

Inputs, packing, the float64 reference and the check are tests/mla_inputs.py's (its CPU tier shows that ten numpy "wrong kernels" fail
that check).  Bounds are the project's: cm.MAX_ABS and cm.REL_L2 on O, 2 * cm.P_EPS absolute on the lse of live rows with a key, exact
0 / -inf on rows without one.  A 16-bit result is held against the fp32 result of the same call rounded once, bit for bit.

Poison: O and lse are pre-filled with sentinels, the workspace with NaN bytes; Q rows of no sequence hold NaN; every cache row at or
past L_b holds NaN bit patterns; every pool page no table names holds NaN; every table entry past the live pages holds garbage.
"""
import numpy as np
import pytest

import common_inputs as cm
import decode_varlen_inputs as dv
import mla_inputs as mi

pytestmark = pytest.mark.gpu

FMTS = [pytest.param(fmt, id=cm.FMT_NAME[fmt]) for fmt in (0, 1)]
FORMS = [pytest.param(ps, id=f"page{ps}" if ps else "contiguous") for ps in (0, 16, 64, 128)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ints(torch, values):
    return None if values is None else torch.tensor([int(x) for x in values], dtype=torch.int32, device="cuda")


def _sentinel_out(torch, shape, out_dtype):
    if out_dtype == torch.float32:
        return torch.full(shape, dv.SENTINEL_O32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, dv.SENTINEL_O16, dtype=torch.int16, device="cuda").view(out_dtype)


def _bits(torch, t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _tdt(torch, fmt):
    return torch.bfloat16 if fmt else torch.float16


def _run(fa, torch, q, cache, cu, max_q, lens, table, Hq, causal=True, S=0, out_dtype=None, out=None, lse=None, scale=None):
    """one call of the entry under test with a NaN-filled workspace -> (O, lse), pre-filled with the sentinels unless given"""
    out_dtype = out_dtype or torch.float32
    T = q.shape[0]
    if out is None:
        out = _sentinel_out(torch, (T, Hq, mi.DC), out_dtype)
    if lse is None:
        lse = torch.full((Hq, T), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    B = cu.numel() - 1
    geo = dict(max_pages=table.shape[1], page_size=cache.shape[1]) if table is not None else dict(Ncap=cache.shape[1])
    need = fa.mla_decode_workspace_bytes(B, Hq, max_q, num_splits=S, **geo)
    assert (need == 0) == (S == 1) or S == 0
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN
    o, l = fa.fa_mla_decode(q, cache, cu, max_q, cache_seqlens=lens, block_table=table, causal=causal, num_splits=S, out=out, lse=lse,
                            workspace=ws, scale=scale)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr() and l.data_ptr() == lse.data_ptr() and o.dtype == out_dtype
    return o, l


class Case:
    """The device tensors of one (family, fmt, cache form): made once per test"""

    def __init__(self, oracle, torch, name, fmt, ps=0):
        self.name, self.fmt, self.ps = name, fmt, ps
        self.f, self.lay = mi.family(name), mi.layout(name)
        self.q = cm.dev16(torch, mi.packed_q_bits(oracle, name, fmt), fmt)
        if ps:
            pool, table = mi.paged_cache(oracle, name, fmt, ps)
            self.cache, self.table = cm.dev16(torch, pool, fmt), torch.from_numpy(table).cuda()
        else:
            self.cache, self.table = cm.dev16(torch, mi.poisoned_cache(oracle, name, fmt), fmt), None
        self.cu, self.lens = _ints(torch, self.lay.cu), _ints(torch, self.f["lens"])

    def run(self, fa, torch, **kw):
        return _run(fa, torch, self.q, self.cache, self.cu, self.f["max_q"], self.lens, self.table, self.f["Hq"], **kw)


def _check(oracle, case, o, lse, causal, what):
    want, want_lse = mi.reference(oracle, case.name, case.fmt, causal)
    mi.check(oracle, case.name, o.float().cpu().numpy(), lse.cpu().numpy(), want, want_lse, case.fmt, what)


def _check_16bit(torch, lay, o16, lse16, o32, lse32, what):
    """a same-type result is the fp32 result rounded once; tokens of no sequence keep the 16-bit sentinel"""
    owned = torch.from_numpy(lay.owned).cuda()
    assert torch.equal(_bits(torch, o16[owned]), _bits(torch, o32[owned].to(o16.dtype))), what + ": 16-bit O is not the rounded fp32 O"
    assert (_bits(torch, o16[~owned]) == int(dv.SENTINEL_O16)).all(), what + ": a 16-bit O row of no sequence was written"
    assert torch.equal(_bits(torch, lse16), _bits(torch, lse32)), what + ": lse depends on the output type"


# ---- 1. the families, on every cache form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", FORMS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", mi.NAMES)
def test_families(fa, oracle, torch_cuda, name, fmt, ps):
    """Hq in {1, 5, 16, 48, 128}; n_b in {0, 1, 2, max_q} and a sequence that owns more; L in {0, 1, 63, 64, 65, 200, capacity} and
    below n_b; raw lengths outside [0, capacity]: causal and not, the library's split count, fp32 and same-type output"""
    torch = torch_cuda
    case = Case(oracle, torch, name, fmt, ps)
    for causal in (True, False):
        what = f"{name} {cm.FMT_NAME[fmt]} page={ps} causal={causal}"
        o, lse = case.run(fa, torch, causal=causal)
        _check(oracle, case, o, lse, causal, what)
        if causal:
            o16, lse16 = case.run(fa, torch, causal=causal, out_dtype=_tdt(torch, fmt))
            _check_16bit(torch, case.lay, o16, lse16, o, lse, what)


# ---- 2. split counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, "max", 0])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["h5", "h16", "h48"])
def test_splits(fa, oracle, torch_cuda, name, fmt, S):
    """one pass, two and three splits, as many splits as the capacity has 64-key tiles (more than any shorter sequence has), and the
    library's choice; every family holds sequences that leave some splits without a key"""
    torch = torch_cuda
    case = Case(oracle, torch, name, fmt)
    S = case.f["Ncap"] // 64 if S == "max" else S
    o, lse = case.run(fa, torch, S=S)
    _check(oracle, case, o, lse, True, f"{name} {cm.FMT_NAME[fmt]} S={S}")
    o16, lse16 = case.run(fa, torch, S=S, out_dtype=_tdt(torch, fmt))
    _check_16bit(torch, case.lay, o16, lse16, o, lse, f"{name} S={S}")


# ---- 3. bit ties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["h5", "h16"])
def test_paged_returns_the_contiguous_bits(fa, oracle, torch_cuda, name, fmt, S):
    torch = torch_cuda
    base = Case(oracle, torch, name, fmt).run(fa, torch, S=S)
    for ps in (16, 64, 128):
        got = Case(oracle, torch, name, fmt, ps).run(fa, torch, S=S)
        for x, y, n in zip(got, base, ("O", "lse")):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{name} S={S} page={ps}: {n} differs from the contiguous cache's"


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["h5", "h48"])
def test_a_sequence_alone_returns_its_bits_in_the_batch(fa, oracle, torch_cuda, name, fmt, S):
    torch = torch_cuda
    case = Case(oracle, torch, name, fmt)
    o, lse = case.run(fa, torch, S=S)
    f, lay = case.f, case.lay
    for b in range(f["B"]):
        s, n = lay.s[b], lay.n[b]
        if n == 0:
            continue
        span = f["spans"][b]
        o1, lse1 = _run(fa, torch, case.q[s:s + span], case.cache[b:b + 1], _ints(torch, [0, span]), f["max_q"], case.lens[b:b + 1], None,
                        f["Hq"], S=S)
        assert torch.equal(_bits(torch, o1[:n]), _bits(torch, o[s:s + n])), f"{name} S={S}: O of sequence {b} depends on the batch"
        assert torch.equal(_bits(torch, lse1[:, :n]), _bits(torch, lse[:, s:s + n])), f"{name} S={S}: lse of sequence {b}"


# ---- 4. a live table entry outside the pool ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda, fmt):
    """entries of one live page of two sequences point outside [0, num_pages), one above and one below: the keys of those pages are
    rows of zeros (logit 0, V row 0), checked against the reference on the cache with those rows zeroed"""
    torch = torch_cuda
    name, ps = "h16", 16
    case = Case(oracle, torch, name, fmt, ps)
    f, lay = case.f, case.lay
    table = case.table.clone()
    table[0, 3], table[1, 0] = case.cache.shape[0] + 7, -2
    (q, c), _ = mi.inputs(oracle, name, fmt)
    c = c.copy()
    c[0, 3 * ps:4 * ps], c[1, 0:ps] = 0.0, 0.0
    want, want_lse = mi.expected_f64(q, c, f["lens"], lay.n, f["max_q"], f["Hq"], True)
    for S in (1, 3):
        o, lse = _run(fa, torch, case.q, case.cache, case.cu, f["max_q"], case.lens, table, f["Hq"], S=S)
        mi.check(oracle, name, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"bad live page {cm.FMT_NAME[fmt]} S={S}")


# ---- 5. exact census -------------------------------------------------------------------------------------------------------------------
def _census_case(torch, fmt, ps, rope):
    """B = 3, Hq = 5, max_q = 3, capacity 256: key j of every sequence is the one-hot row e_j in its first 512 columns and `rope` in
    its last 64; lengths (200, 65, 2), rows (3, 1, 3): the last sequence has a row without a key"""
    B, Hq, Nq, Ncap = 3, 5, 3, 256
    lens, spans = (200, 65, 2), (3, 1, 3)
    cu = np.cumsum([1] + list(spans))
    lay = dv.Layout(cu, int(cu[-1]) + 1, Nq)
    c = np.zeros((B, Ncap, mi.DQK), np.float32)
    c[:, np.arange(Ncap), np.arange(Ncap)] = 1.0
    c[:, :, mi.DC:] = rope
    tdt = _tdt(torch, fmt)
    cache = torch.from_numpy(c).cuda().to(tdt)
    for b in range(B):
        cache[b, lens[b]:] = float("nan")
    table = None
    if ps:
        max_pages = Ncap // ps
        perm = torch.randperm(B * max_pages + 2, generator=torch.Generator().manual_seed(11)).to(torch.int32)[:B * max_pages]
        table = perm.view(B, max_pages).cuda()
        pool = torch.full((B * max_pages + 2, ps, mi.DQK), float("nan"), dtype=tdt, device="cuda")
        pool[table.view(-1).long()] = cache.view(B * max_pages, ps, mi.DQK)
        cache = pool
    return lay, lens, cache, table, _ints(torch, cu), _ints(torch, lens), c, (B, Hq, Nq, Ncap)


@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="page16")])
@pytest.mark.parametrize("fmt", FMTS)
def test_census_every_visible_key_once(fa, torch_cuda, fmt, ps):
    """q = 0 makes every weight 1: column j of O is exactly 1 / c_i for j < c_i and 0 for every other key, for every split count --
    a key counted twice, dropped, or taken from a row at or past L_b (NaN) shows as a wrong bit"""
    torch = torch_cuda
    lay, lens, cache, table, cu, dl, _, (B, Hq, Nq, Ncap) = _census_case(torch, fmt, ps, 3.0)
    q = torch.zeros((lay.total_q, Hq, mi.DQK), dtype=_tdt(torch, fmt), device="cuda")
    for causal in (True, False):
        want = np.zeros((lay.total_q, Hq, mi.DC), np.float32)
        want_lse = np.full((Hq, lay.total_q), -np.inf, np.float32)
        for b in range(B):
            for i in range(lay.n[b]):
                lim = max(0, lens[b] - lay.n[b] + 1 + i) if causal else lens[b]
                if lim:
                    want[lay.tok[b, i], :, :lim] = np.float32(1.0) / np.float32(lim)
                    want_lse[:, lay.tok[b, i]] = np.log(np.float64(lim))
        for S in (1, 2, 3, 4, 0):
            o, lse = _run(fa, torch, q, cache, cu, Nq, dl, table, Hq, causal=causal, S=S)
            o, lse = o.cpu().numpy(), lse.cpu().numpy()
            assert np.array_equal(o[lay.owned], want[lay.owned]), f"census causal={causal} S={S} page={ps}"
            got = lse[:, lay.owned]
            ref = want_lse[:, lay.owned]
            fin = np.isfinite(ref)
            assert (got[~fin] == -np.inf).all() and np.abs(got[fin] - ref[fin]).max() <= 1e-6 * np.log(256.0) + 1e-6


@pytest.mark.parametrize("fmt", FMTS)
def test_rope_elements_never_reach_o(fa, oracle, torch_cuda, fmt):
    """the last 64 columns of the cache hold values of magnitude 2^12 and the first 512 columns of Q are zero: the rotary part alone
    makes the logits (as it should; q's rotary elements are small multiples of 2^-10, so the logits stay O(1)), and O -- the softmax
    weights themselves, V being one-hot -- stays finite and within the bounds of the float64 reference; a V that took any of the last
    64 columns would be off by thousands"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    rope = (rng.standard_normal((3, 256, mi.DR)) * 2.0 ** 12).astype(np.float32)
    lay, lens, cache, table, cu, dl, c, (B, Hq, Nq, Ncap) = _census_case(torch, fmt, 0, rope)
    qv = np.zeros((B * Hq, Nq, mi.DQK), np.float32)
    qv[:, :, mi.DC:] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (B * Hq, Nq, mi.DR)) * 2.0 ** -10
    qb, cb = oracle.encode16(qv, fmt), oracle.encode16(c, fmt)
    want, want_lse = mi.expected_f64(oracle.decode16(qb, fmt), oracle.decode16(cb, fmt), lens, lay.n, Nq, Hq, True)
    assert np.ptp(want_lse[np.isfinite(want_lse)]) > 0.05   # the rotary values do move the logits
    q = cm.dev16(torch, dv.pack_rows(lay, qb, np.uint16(cm.NAN16)), fmt)
    cache = cm.dev16(torch, cm.poisoned(cb[:, None], lens)[:, 0], fmt)
    for S in (1, 2):
        o, lse = _run(fa, torch, q, cache, cu, Nq, dl, None, Hq, S=S)
        dv.check(oracle, lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"rope census {cm.FMT_NAME[fmt]} S={S}")


@pytest.mark.parametrize("fmt", FMTS)
def test_scale_zero_gives_uniform_weights(fa, oracle, torch_cuda, fmt):
    torch = torch_cuda
    case = Case(oracle, torch, "h5", fmt)
    f, lay = case.f, case.lay
    (q, c), _ = mi.inputs(oracle, "h5", fmt)
    want, want_lse = mi.expected_f64(q, c, f["lens"], lay.n, f["max_q"], f["Hq"], True, scale=0.0)
    for S in (1, 2):
        o, lse = case.run(fa, torch, S=S, scale=0.0)
        mi.check(oracle, "h5", o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"scale 0 {cm.FMT_NAME[fmt]} S={S}")


# ---- 6. views and clamps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_strided_q_and_o_views(fa, oracle, torch_cuda, fmt):
    """q as a slice of a fused (total, Hq, 576 + 128) buffer (q_stride_h = 704) and, transposed, of a (Hq, total, 576) one; O into a
    slice of a wider buffer: the bits of the dense call, and nothing outside the view is written"""
    torch = torch_cuda
    case = Case(oracle, torch, "h5", fmt)
    f, lay = case.f, case.lay
    T, Hq = lay.total_q, f["Hq"]
    for S in (1, 2):
        o, lse = case.run(fa, torch, S=S)
        fused = torch.full((T, Hq, mi.DQK + 128), float("nan"), dtype=case.q.dtype, device="cuda")
        fused[:, :, :mi.DQK] = case.q
        wide = _sentinel_out(torch, (T, Hq, mi.DC + 64), torch.float32)
        o2, lse2 = _run(fa, torch, fused[:, :, :mi.DQK], case.cache, case.cu, f["max_q"], case.lens, None, Hq, S=S, out=wide[:, :, :mi.DC])
        assert torch.equal(_bits(torch, o2), _bits(torch, o)) and torch.equal(_bits(torch, lse2), _bits(torch, lse)), f"fused view S={S}"
        assert (_bits(torch, wide[:, :, mi.DC:]) == dv.SENTINEL_O32).all(), "written outside the O view"
        head_major = case.q.transpose(0, 1).contiguous()           # (Hq, T, 576): q_stride_t = 576, q_stride_h = T * 576
        o_hm = _sentinel_out(torch, (Hq, T, mi.DC), torch.float32)
        o3, lse3 = _run(fa, torch, head_major.transpose(0, 1), case.cache, case.cu, f["max_q"], case.lens, None, Hq, S=S,
                        out=o_hm.transpose(0, 1))
        assert torch.equal(_bits(torch, o3), _bits(torch, o)) and torch.equal(_bits(torch, lse3), _bits(torch, lse)), f"head-major S={S}"


@pytest.mark.parametrize("fmt", FMTS)
def test_clamps_of_cu_seqlens_q(fa, oracle, torch_cuda, fmt):
    """a negative entry, a decreasing pair and an entry beyond total_q, on h5's caches (B = 4, max_q = 4): the result is the call on the
    clamped vector, and nothing outside O and lse is written (guard rows around both allocations)"""
    torch = torch_cuda
    case = Case(oracle, torch, "h5", fmt)
    f = case.f
    Hq, Nq, T, GUARD = f["Hq"], f["max_q"], 16, 5
    raw = [-7, 10, 5, 8, 99]               # s = (0, 10, 5, 8), e = (10, 10, 8, 16): n = (4, 0, 3, 4)
    lay = dv.Layout(raw, T, Nq)
    assert lay.n == [4, 0, 3, 4] and lay.s == [0, 10, 5, 8]
    clamped = dv.Layout([0, 10, 5, 8, 16], T, Nq)
    assert clamped.n == lay.n and np.array_equal(clamped.tok, lay.tok)
    (qv, c), (qb, _) = mi.inputs(oracle, "h5", fmt)
    q = cm.dev16(torch, dv.pack_rows(lay, qb, np.uint16(cm.NAN16)), fmt)
    want, want_lse = mi.expected_f64(qv, c, f["lens"], lay.n, Nq, Hq, True)
    for S in (1, 2):
        res = []
        for cu in (raw, clamped.cu):
            obuf = _sentinel_out(torch, (T + 2 * GUARD, Hq, mi.DC), torch.float32)
            lbuf = torch.full((Hq * T + 2 * GUARD * T,), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
            o, lse = _run(fa, torch, q, case.cache, _ints(torch, cu), Nq, case.lens, None, Hq, S=S, out=obuf[GUARD:GUARD + T],
                          lse=lbuf[GUARD * T:GUARD * T + Hq * T].view(Hq, T))
            assert (_bits(torch, obuf[:GUARD]) == dv.SENTINEL_O32).all() and (_bits(torch, obuf[GUARD + T:]) == dv.SENTINEL_O32).all()
            assert (lbuf[:GUARD * T] == dv.SENTINEL_LSE).all() and (lbuf[GUARD * T + Hq * T:] == dv.SENTINEL_LSE).all()
            res.append((o.clone(), lse.clone()))
        for x, y in zip(*res):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), "the raw vector and its clamp differ"
        dv.check(oracle, lay, res[0][0].cpu().numpy(), res[0][1].cpu().numpy(), want, want_lse, fmt, f"clamped cu_seqlens_q S={S}")


# ---- 7. fa_mla_append ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="page16"), pytest.param(64, id="page64")])
@pytest.mark.parametrize("fmt", FMTS)
def test_append_bytes(fa, torch_cuda, fmt, ps):
    """bytes against the numpy model: tokens of no sequence, drops at the capacity, a raw length above it and a negative one, NaN
    payloads kept, a strided source; paged: a shuffled table with a -1 and an out-of-range entry; seqlens_out aliasing seqlens_k, a
    separate vector, and none"""
    torch = torch_cuda
    rng = np.random.default_rng(31 + ps)
    B, cap, T = 4, 128, 14
    cu = [2, 6, 8, 9, 13]                      # m = (4, 2, 1, 4); tokens 0, 1 and 13 belong to no sequence
    lens = [126, 17, -4, 500]                  # sequence 0 drops two tokens at the capacity, sequence 3 is full: all four dropped
    new = rng.integers(0, 1 << 16, (T, mi.DQK + 64), dtype=np.uint16)   # every bit pattern, NaNs included; token stride 640
    if ps:
        max_pages = cap // ps
        num_pages = B * max_pages + 3
        cache = rng.integers(0, 1 << 16, (num_pages, ps, mi.DQK), dtype=np.uint16)
        table = rng.permutation(num_pages)[:B * max_pages].astype(np.int32).reshape(B, max_pages)
        table[1, 17 // ps] = -1                # the page of sequence 1's slots 17 and 18: both writes are skipped
        table[2, 0] = num_pages + 5            # ... and of sequence 2's slot 0
        dtable = torch.from_numpy(table).cuda()
    else:
        cache, table, dtable = rng.integers(0, 1 << 16, (B, cap, mi.DQK), dtype=np.uint16), None, None
    want, want_lens = mi.append_model(cache, new[:, :mi.DQK], cu, lens, T, table)
    dnew = cm.dev16(torch, new, fmt)[:, :mi.DQK]
    for mode in ("alias", "separate", "none"):
        dcache, dl = cm.dev16(torch, cache, fmt), _ints(torch, lens)
        out = dl if mode == "alias" else (torch.full((B,), -77, dtype=torch.int32, device="cuda") if mode == "separate" else None)
        fa.fa_mla_append(dnew, dcache, _ints(torch, cu), cache_seqlens=dl, seqlens_out=out, block_table=dtable)
        torch.cuda.synchronize()
        assert np.array_equal(dcache.view(torch.int16).cpu().numpy().view(np.uint16), want), f"append bytes page={ps} {mode}"
        if out is not None:
            assert out.cpu().tolist() == list(want_lens), f"lengths page={ps} {mode}"
        if mode != "alias":
            assert dl.cpu().tolist() == lens, "seqlens_k was written"
    # a fresh cache: no lengths at all
    dcache = cm.dev16(torch, cache, fmt)
    fa.fa_mla_append(dnew, dcache, _ints(torch, cu), block_table=dtable)
    torch.cuda.synchronize()
    want0, _ = mi.append_model(cache, new[:, :mi.DQK], cu, None, T, table)
    assert np.array_equal(dcache.view(torch.int16).cpu().numpy().view(np.uint16), want0)


# ---- 8. append -> decode, captured once ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_captured_append_then_decode_follows_its_vectors(fa, oracle, torch_cuda, fmt):
    """fa_mla_append -> fa_mla_decode captured once in a graph and replayed three times with the tokens, cu_seqlens, the lengths and the
    block table rewritten in place: each replay against the float64 reference of its own state"""
    torch = torch_cuda
    B, Hq, max_q, T, ps, max_pages = 2, 16, 2, 5, 16, 8
    cap, num_pages, tdt = ps * max_pages, 2 * 8 + 4, _tdt(torch, fmt)
    rng = np.random.default_rng(404 + fmt)
    pool0_bits = oracle.encode16(rng.standard_normal((num_pages, ps, mi.DQK)).astype(np.float32), fmt)
    pool0 = cm.dev16(torch, pool0_bits, fmt)
    pool, q, cnew = pool0.clone(), torch.zeros((T, Hq, mi.DQK), dtype=tdt, device="cuda"), torch.zeros((T, mi.DQK), dtype=tdt, device="cuda")
    cu, lens = _ints(torch, [0, 1, 2]), _ints(torch, [0, 0])
    table = torch.zeros((B, max_pages), dtype=torch.int32, device="cuda")
    out = torch.zeros((T, Hq, mi.DC), dtype=torch.float32, device="cuda")
    lse = torch.zeros((Hq, T), dtype=torch.float32, device="cuda")
    S = 2
    ws = torch.full((fa.mla_decode_workspace_bytes(B, Hq, max_q, max_pages=max_pages, page_size=ps, num_splits=S),), 0xFF, dtype=torch.uint8,
                    device="cuda")
    assert ws.numel() > 0

    def step(pl, ln, o, l):
        fa.fa_mla_append(cnew, pl, cu, cache_seqlens=ln, seqlens_out=ln, block_table=table)
        fa.fa_mla_decode(q, pl, cu, max_q, cache_seqlens=ln, block_table=table, causal=True, num_splits=S, out=o, lse=l, workspace=ws)

    step(pool.clone(), lens.clone(), out.clone(), lse.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pool, lens, out, lse)
    states = [([1, 3, 4], [100, 37]), ([0, 1, 2], [0, 126]), ([2, 2, 5], [64, 65])]   # n = (2, 1); (1, 1); (0, 2 of 3: cut at max_q)
    for s, (vec, before) in enumerate(states):
        qb = oracle.encode16(rng.standard_normal((T, Hq, mi.DQK)).astype(np.float32), fmt)
        nb = oracle.encode16(rng.standard_normal((T, mi.DQK)).astype(np.float32), fmt)
        tb = rng.permutation(num_pages)[:B * max_pages].astype(np.int32).reshape(B, max_pages)
        for dst, src in ((q, cm.dev16(torch, qb, fmt)), (cnew, cm.dev16(torch, nb, fmt)), (cu, _ints(torch, vec)), (lens, _ints(torch, before)),
                         (table, torch.from_numpy(tb).cuda()), (pool, pool0)):
            dst.copy_(src)
        ws.fill_(0xFF)
        out.copy_(_sentinel_out(torch, tuple(out.shape), torch.float32)), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        want_pool, after = mi.append_model(pool0_bits, nb, vec, before, T, tb)
        assert np.array_equal(pool.view(torch.int16).cpu().numpy().view(np.uint16), want_pool), f"step {s}: the pool after the append"
        assert lens.cpu().tolist() == list(after), f"step {s}: the lengths after the append"
        lay = dv.Layout(vec, T, max_q)
        cache = oracle.decode16(want_pool[tb.reshape(-1)].reshape(B, cap, mi.DQK), fmt)
        qpad = dv.unpack_rows(lay, oracle.decode16(qb, fmt), B)
        want, want_lse = mi.expected_f64(qpad, cache, after, lay.n, max_q, Hq, True)
        dv.check(oracle, lay, out.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"replay {s} {cm.FMT_NAME[fmt]}")


# ---- 9. a second oracle, and the torch ops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_against_torch_fp32_on_the_device(fa, oracle, torch_cuda, fmt):
    """softmax(q C^T) C[:, :512] in fp32 torch matmuls on the gathered rows, at h16's shape"""
    torch = torch_cuda
    case = Case(oracle, torch, "h16", fmt)
    f, lay = case.f, case.lay
    o, lse = case.run(fa, torch, S=0)
    for b in range(f["B"]):
        L = min(max(f["lens"][b], 0), f["Ncap"])
        for i in range(lay.n[b]):
            lim = max(0, L - lay.n[b] + 1 + i)
            t = int(lay.tok[b, i])
            keys = case.cache[b, :lim].float()
            s = (case.q[t].float() @ keys.T) * mi.SCALE
            ref = torch.softmax(s, dim=-1) @ keys[:, :mi.DC]
            ref_lse = torch.logsumexp(s, dim=-1)
            ma = float((o[t] - ref).abs().max())
            rl = float((o[t] - ref).norm() / ref.norm())
            le = float((lse[:, t] - ref_lse).abs().max())
            print(f"torch fp32 b={b} i={i}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e}")
            assert ma <= cm.MAX_ABS and rl <= cm.REL_L2[fmt] and le <= 2 * cm.P_EPS[fmt]


def test_torch_ops(fa, oracle, torch_cuda):
    """torch.ops.fa_mi355.mla_append and .mla_decode are the front end's calls: the same bits"""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    case = Case(oracle, torch, "h16", 0, 16)
    f = case.f
    o, lse = fa.fa_mla_decode(case.q, case.cache, case.cu, f["max_q"], cache_seqlens=case.lens, block_table=case.table, return_lse=True,
                              num_splits=2)
    o2, lse2 = torch.ops.fa_mi355.mla_decode(case.q, case.cache, case.cu, f["max_q"], case.lens, case.table, mi.SCALE, True, 2, True)
    torch.cuda.synchronize()
    owned = torch.from_numpy(case.lay.owned).cuda()
    assert torch.equal(_bits(torch, o2[owned]), _bits(torch, o[owned])) and torch.equal(_bits(torch, lse2[:, owned]), _bits(torch, lse[:, owned]))
    assert (o2[~owned] == 0).all() and (lse2[:, ~owned] == -float("inf")).all()
    o16, _ = torch.ops.fa_mi355.mla_decode(case.q, case.cache, case.cu, f["max_q"], case.lens, case.table, mi.SCALE, True, 2, False)
    assert o16.dtype == case.q.dtype and o16.shape == (case.q.shape[0], f["Hq"], mi.DC)
    new = case.q[:4, 0].contiguous()
    pools = [case.cache.clone(), case.cache.clone()]
    before, after = _ints(torch, [5, 5, 5]), [torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(2)]
    cu = _ints(torch, [0, 1, 3, 4])
    table = case.table.clamp(0, case.cache.shape[0] - 1)   # slots 5 .. 6 lie in each sequence's first page, which is live and its own
    fa.fa_mla_append(new, pools[0], cu, cache_seqlens=before, seqlens_out=after[0], block_table=table)
    torch.ops.fa_mi355.mla_append(new, pools[1], cu, before, after[1], table)
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch, pools[0]), _bits(torch, pools[1])) and not torch.equal(_bits(torch, pools[0]), _bits(torch, case.cache))
    assert torch.equal(after[0], after[1]) and after[0].tolist() == [6, 7, 6]
