"""GPU tier of the fp8 MLA entries fa_mla_decode_fp8 and fa_mla_append_fp8 (fa.fa_mla_decode_fp8, fa.fa_mla_append_fp8,
fa.quantize_mla_fp8, torch.ops.fa_mi355.mla_*_fp8).

Inputs and the float64 reference are tests/mla_fp8_inputs.py's: the families of tests/mla_inputs.py with their caches held as e4m3fn
codes under c_scale = 12 / 448, the reference computed on the decoded codes (its CPU tier shows that ten numpy "wrong kernels" fail the
check).  Bounds are the project's, unchanged: cm.MAX_ABS and cm.REL_L2 on O, 2 * cm.P_EPS absolute on the lse of live rows with a
key, exact 0 / -inf on rows without one -- the device widens the codes exactly, so the fp8 cache adds no error of its own.  Where the
arithmetic is fa_mla_decode's on the widened cache, the two entries are compared bit for bit.

Poison: as in tests/test_gpu_mla.py, with the NaN CODE 0x7F in every cache row at or past L_b and in every pool page no table names.
"""
import numpy as np
import pytest

import common_inputs as cm
import decode_varlen_inputs as dv
import fp8_inputs as f8
import mla_fp8_inputs as m8
import mla_inputs as mi
import softmax_range_inputs as sr
import test_gpu_mla as tgm

pytestmark = pytest.mark.gpu

FMTS = tgm.FMTS
FORMS = tgm.FORMS
_ints, _bits, _tdt, _sentinel_out = tgm._ints, tgm._bits, tgm._tdt, tgm._sentinel_out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _scale(torch, value):
    return None if value is None else torch.tensor([float(value)], dtype=torch.float32, device="cuda")


def _run8(fa, torch, q, cache, cu, max_q, lens, table, Hq, c_scale=m8.C_SCALE, causal=True, S=0, out_dtype=None, out=None, lse=None,
          scale=None):
    """one call of fa_mla_decode_fp8 with a NaN-filled workspace -> (O, lse), pre-filled with the sentinels unless given; c_scale is a
    number, None or a device tensor"""
    out_dtype = out_dtype or torch.float32
    T = q.shape[0]
    if out is None:
        out = _sentinel_out(torch, (T, Hq, mi.DC), out_dtype)
    if lse is None:
        lse = torch.full((Hq, T), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
    B = cu.numel() - 1
    geo = dict(max_pages=table.shape[1], page_size=cache.shape[1]) if table is not None else dict(Ncap=cache.shape[1])
    need = fa.mla_decode_workspace_bytes(B, Hq, max_q, num_splits=S, **geo)
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    cs = c_scale if c_scale is None or isinstance(c_scale, torch.Tensor) else _scale(torch, c_scale)
    o, l = fa.fa_mla_decode_fp8(q, cache, cu, max_q, cache_seqlens=lens, block_table=table, c_scale=cs, causal=causal, num_splits=S,
                                out=out, lse=lse, workspace=ws, scale=scale)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr() and l.data_ptr() == lse.data_ptr() and o.dtype == out_dtype
    return o, l


class Case:
    """The device tensors of one (family, fmt, cache form) with the cache as codes: made once per test"""

    def __init__(self, oracle, torch, name, fmt, ps=0):
        self.name, self.fmt, self.ps = name, fmt, ps
        self.f, self.lay = mi.family(name), mi.layout(name)
        self.q = cm.dev16(torch, mi.packed_q_bits(oracle, name, fmt), fmt)
        if ps:
            pool, table = m8.paged_cache(oracle, name, fmt, ps)
            self.cache, self.table = cm.dev8(torch, pool), torch.from_numpy(table).cuda()
        else:
            self.cache, self.table = cm.dev8(torch, m8.poisoned_cache(oracle, name, fmt)), None
        self.cu, self.lens = _ints(torch, self.lay.cu), _ints(torch, self.f["lens"])

    def run(self, fa, torch, **kw):
        return _run8(fa, torch, self.q, self.cache, self.cu, self.f["max_q"], self.lens, self.table, self.f["Hq"], **kw)


def _check(oracle, case, o, lse, causal, what):
    want, want_lse = m8.reference(oracle, case.name, case.fmt, causal)
    mi.check(oracle, case.name, o.float().cpu().numpy(), lse.cpu().numpy(), want, want_lse, case.fmt, what)


def _same(torch, got, want, what):
    for x, y, n in zip(got, want, ("O", "lse")):
        assert torch.equal(_bits(torch, x), _bits(torch, y)), f"{what}: {n} differs"


# ---- 1. the families, on every cache form, against the float64 reference ---------------------------------------------------------------
@pytest.mark.parametrize("ps", FORMS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", mi.NAMES)
def test_families(fa, oracle, torch_cuda, name, fmt, ps):
    """every family of the 16-bit tier on codes: causal and not, the library's split count, fp32 and same-type output; the NaN code in
    every row and page nothing may read, NaN in the Q rows of no sequence, sentinels in O and lse"""
    torch = torch_cuda
    case = Case(oracle, torch, name, fmt, ps)
    assert (case.cache.view(torch.uint8) == m8.NAN_CODE).any() and torch.isnan(case.q[~torch.from_numpy(case.lay.owned).cuda()]).all()
    for causal in (True, False):
        what = f"fp8 {name} {cm.FMT_NAME[fmt]} page={ps} causal={causal}"
        o, lse = case.run(fa, torch, causal=causal)
        _check(oracle, case, o, lse, causal, what)
        if causal:
            o16, lse16 = case.run(fa, torch, causal=causal, out_dtype=_tdt(torch, fmt))
            tgm._check_16bit(torch, case.lay, o16, lse16, o, lse, what)


@pytest.mark.parametrize("S", [1, 2, 3, "max"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["h5", "h16"])
def test_splits(fa, oracle, torch_cuda, name, fmt, S):
    torch = torch_cuda
    case = Case(oracle, torch, name, fmt)
    S = case.f["Ncap"] // 64 if S == "max" else S
    o, lse = case.run(fa, torch, S=S)
    _check(oracle, case, o, lse, True, f"fp8 {name} {cm.FMT_NAME[fmt]} S={S}")


# ---- 2. bit for bit against fa_mla_decode on the widened cache ---------------------------------------------------------------------------
class AllCodes:
    """h16's rows and lengths over a cache whose live rows run through all 254 finite codes; dead rows hold the NaN code.  `wide` is the
    same cache widened to Q's type on the host (every e4m3fn value is an fp16 and a bf16 number), NaN where the NaN code is."""

    def __init__(self, oracle, torch, fmt):
        self.f, self.lay = mi.family("h16"), mi.layout("h16")
        f = self.f
        codes = f8.all_codes((f["B"], f["Ncap"], mi.DQK), 4711 + fmt)
        self.codes = cm.poisoned(codes[:, None], f["lens"], nan=m8.NAN_CODE)[:, 0]
        live = self.codes[0, :cm.clamp(f["lens"][0], f["Ncap"])]
        assert np.unique(live).size == 254
        self.q = cm.dev16(torch, mi.packed_q_bits(oracle, "h16", fmt), fmt)
        self.cache = cm.dev8(torch, self.codes)
        self.wide = torch.from_numpy(f8.decode(self.codes)).cuda().to(_tdt(torch, fmt))
        self.cu, self.lens = _ints(torch, self.lay.cu), _ints(torch, f["lens"])

    def run8(self, fa, torch, **kw):
        return _run8(fa, torch, self.q, self.cache, self.cu, self.f["max_q"], self.lens, None, self.f["Hq"], **kw)

    def run16(self, fa, torch, **kw):
        return tgm._run(fa, torch, self.q, self.wide, self.cu, self.f["max_q"], self.lens, None, self.f["Hq"], **kw)


@pytest.mark.parametrize("S", [1, 2, 3, "max", 0])
@pytest.mark.parametrize("fmt", FMTS)
def test_without_a_scale_the_bits_are_fa_mla_decodes(fa, oracle, torch_cuda, fmt, S):
    """c_scale = None: the bits of fa_mla_decode on the cache widened to Q's type, for both output types; c_scale = [1.0]: the same"""
    torch = torch_cuda
    ac = AllCodes(oracle, torch, fmt)
    fin = ~torch.isnan(ac.wide)
    assert torch.equal(ac.wide[fin].float().cpu(), torch.from_numpy(f8.decode(ac.codes))[fin.cpu()])   # the host widening is exact
    S = ac.f["Ncap"] // 64 if S == "max" else S
    for out_dtype in (torch.float32, _tdt(torch, fmt)):
        want = ac.run16(fa, torch, S=S, out_dtype=out_dtype)
        _same(torch, ac.run8(fa, torch, c_scale=None, S=S, out_dtype=out_dtype), want, f"all codes S={S} {out_dtype} no scale")
        _same(torch, ac.run8(fa, torch, c_scale=1.0, S=S, out_dtype=out_dtype), want, f"all codes S={S} {out_dtype} scale of ones")
    assert torch.isfinite(want[0][torch.from_numpy(ac.lay.owned).cuda()].float()).all()


@pytest.mark.parametrize("c_scale", [2.0 ** -3, 2.0 ** 2])
@pytest.mark.parametrize("fmt", FMTS)
def test_a_power_of_two_scale_commutes(fa, oracle, torch_cuda, fmt, c_scale):
    """fp32 output: O is c_scale x the bits of fa_mla_decode(scale = scale * c_scale) on the widened cache and lse is its lse, bit for
    bit -- a multiplication by a power of two commutes with every rounding in range"""
    torch = torch_cuda
    ac = AllCodes(oracle, torch, fmt)
    owned = torch.from_numpy(ac.lay.owned).cuda()
    for S in (1, 3, 0):
        o16, lse16 = ac.run16(fa, torch, S=S, scale=mi.SCALE * c_scale)
        o8, lse8 = ac.run8(fa, torch, c_scale=c_scale, S=S, scale=mi.SCALE)
        assert torch.equal(_bits(torch, o8[owned]), _bits(torch, o16[owned] * c_scale)), f"S={S} c_scale={c_scale}: O"
        assert torch.equal(_bits(torch, lse8), _bits(torch, lse16)), f"S={S} c_scale={c_scale}: lse"
        assert (_bits(torch, o8[~owned]) == dv.SENTINEL_O32).all()


# ---- 3. isolation and bad pages -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["h5", "h16"])
def test_paged_returns_the_contiguous_bits(fa, oracle, torch_cuda, name, fmt, S):
    torch = torch_cuda
    base = Case(oracle, torch, name, fmt).run(fa, torch, S=S)
    for ps in (16, 64, 128):
        _same(torch, Case(oracle, torch, name, fmt, ps).run(fa, torch, S=S), base, f"fp8 {name} S={S} page={ps} against contiguous")


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
        o1, lse1 = _run8(fa, torch, case.q[s:s + span], case.cache[b:b + 1], _ints(torch, [0, span]), f["max_q"], case.lens[b:b + 1], None,
                         f["Hq"], S=S)
        assert torch.equal(_bits(torch, o1[:n]), _bits(torch, o[s:s + n])), f"fp8 {name} S={S}: O of sequence {b} depends on the batch"
        assert torch.equal(_bits(torch, lse1[:, :n]), _bits(torch, lse[:, s:s + n])), f"fp8 {name} S={S}: lse of sequence {b}"


@pytest.mark.parametrize("fmt", FMTS)
def test_a_bad_live_page_reads_as_zeros(fa, oracle, torch_cuda, fmt):
    """entries of one live page of two sequences point outside [0, num_pages): the keys of those pages are rows of the code 0"""
    torch = torch_cuda
    name, ps = "h16", 16
    case = Case(oracle, torch, name, fmt, ps)
    f, lay = case.f, case.lay
    table = case.table.clone()
    table[0, 3], table[1, 0] = case.cache.shape[0] + 7, -2
    (q, _), _ = mi.inputs(oracle, name, fmt)
    c = m8.values(m8.codes(oracle, name, fmt)).copy()
    c[0, 3 * ps:4 * ps], c[1, 0:ps] = 0.0, 0.0
    want, want_lse = mi.expected_f64(q, c, f["lens"], lay.n, f["max_q"], f["Hq"], True)
    for S in (1, 3):
        o, lse = _run8(fa, torch, case.q, case.cache, case.cu, f["max_q"], case.lens, table, f["Hq"], S=S)
        mi.check(oracle, name, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"fp8 bad live page {cm.FMT_NAME[fmt]} S={S}")


# ---- 4. census and masking ------------------------------------------------------------------------------------------------------------------
def _census_codes(torch, ps, one, rope_codes):
    """test_gpu_mla's census shape: key j of every sequence holds the code `one` at column j of its first 512 and rope_codes [B, Ncap, 64]
    behind them; dead rows and unnamed pages hold the NaN code"""
    B, Hq, Nq, Ncap = 3, 5, 3, 256
    lens, spans = (200, 65, 2), (3, 1, 3)
    cu = np.cumsum([1] + list(spans))
    lay = dv.Layout(cu, int(cu[-1]) + 1, Nq)
    codes = np.zeros((B, Ncap, mi.DQK), np.uint8)
    codes[:, np.arange(Ncap), np.arange(Ncap)] = one
    codes[:, :, mi.DC:] = rope_codes
    clean = codes.copy()
    table = None
    if ps:
        pool, _, tb = cm.scatter(codes[:, None], codes[:, None], lens, ps, 11, nan=m8.NAN_CODE)
        cache, table = cm.dev8(torch, np.ascontiguousarray(pool[:, 0])), torch.from_numpy(tb).cuda()
    else:
        cache = cm.dev8(torch, cm.poisoned(codes[:, None], lens, nan=m8.NAN_CODE)[:, 0])
    return lay, lens, cache, table, _ints(torch, cu), _ints(torch, lens), clean, (B, Hq, Nq, Ncap)


@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="page16")])
@pytest.mark.parametrize("fmt", FMTS)
def test_census_every_visible_key_once_and_scaled(fa, torch_cuda, fmt, ps):
    """scale = 0 makes every weight 1 whatever q holds, the one-hot code is 1.0 and c_scale = 2^-2: column j of O is exactly
    (1 / c_i) * 0.25 for j < c_i and 0 for every other key, for every split count"""
    torch = torch_cuda
    rng = np.random.default_rng(91)
    rope = rng.choice(f8.FINITE_CODES, (3, 256, mi.DR))
    lay, lens, cache, table, cu, dl, _, (B, Hq, Nq, Ncap) = _census_codes(torch, ps, f8.encode(np.float32(1.0)), rope)
    q = torch.from_numpy(rng.standard_normal((lay.total_q, Hq, mi.DQK)).astype(np.float32)).cuda().to(_tdt(torch, fmt))
    for causal in (True, False):
        want = np.zeros((lay.total_q, Hq, mi.DC), np.float32)
        want_lse = np.full((Hq, lay.total_q), -np.inf, np.float32)
        for b in range(B):
            for i in range(lay.n[b]):
                lim = max(0, lens[b] - lay.n[b] + 1 + i) if causal else lens[b]
                if lim:
                    want[lay.tok[b, i], :, :lim] = (np.float32(1.0) / np.float32(lim)) * np.float32(0.25)
                    want_lse[:, lay.tok[b, i]] = np.log(np.float64(lim))
        for S in (1, 2, 3, 4, 0):
            o, lse = _run8(fa, torch, q, cache, cu, Nq, dl, table, Hq, c_scale=0.25, causal=causal, S=S, scale=0.0)
            o, lse = o.cpu().numpy(), lse.cpu().numpy()
            assert np.array_equal(o[lay.owned], want[lay.owned]), f"fp8 census causal={causal} S={S} page={ps}"
            got, ref = lse[:, lay.owned], want_lse[:, lay.owned]
            fin = np.isfinite(ref)
            assert (got[~fin] == -np.inf).all() and np.abs(got[fin] - ref[fin]).max() <= 1e-6 * np.log(256.0) + 1e-6


@pytest.mark.parametrize("fmt", FMTS)
def test_scale_zero_gives_uniform_weights(fa, oracle, torch_cuda, fmt):
    """scale = 0 under c_scale = 12 / 448: the product is clamped AFTER it is formed, so the weights are uniform over the visible keys"""
    torch = torch_cuda
    case = Case(oracle, torch, "h5", fmt)
    f, lay = case.f, case.lay
    (q, _), _ = mi.inputs(oracle, "h5", fmt)
    want, want_lse = mi.expected_f64(q, m8.values(m8.codes(oracle, "h5", fmt)), f["lens"], lay.n, f["max_q"], f["Hq"], True, scale=0.0)
    for S in (1, 2):
        o, lse = case.run(fa, torch, S=S, scale=0.0)
        mi.check(oracle, "h5", o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"fp8 scale 0 {cm.FMT_NAME[fmt]} S={S}")


@pytest.mark.parametrize("fmt", FMTS)
def test_rope_codes_never_reach_o(fa, oracle, torch_cuda, fmt):
    """c_scale = 16: the rotary codes stand for values of magnitude 2^12 (clamped at 448 * 16), the one-hot code for 1.0, and the first
    512 columns of Q are zero -- the rotary part alone makes the logits, and O (the weights themselves) stays within the bounds of the
    float64 reference; a V that took any rotary code would be off by thousands"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    cs = np.float32(16.0)
    rope = f8.encode((rng.standard_normal((3, 256, mi.DR)) * 2.0 ** 12).astype(np.float32) / cs)
    lay, lens, cache, table, cu, dl, clean, (B, Hq, Nq, Ncap) = _census_codes(torch, 0, f8.encode(np.float32(1.0) / cs), rope)
    assert m8.values(clean[:, :, :mi.DC], cs).max() == 1.0 and np.abs(m8.values(clean[:, :, mi.DC:], cs)).max() == 448.0 * 16.0
    qv = np.zeros((B * Hq, Nq, mi.DQK), np.float32)
    qv[:, :, mi.DC:] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (B * Hq, Nq, mi.DR)) * 2.0 ** -10
    qb = oracle.encode16(qv, fmt)
    want, want_lse = mi.expected_f64(oracle.decode16(qb, fmt), m8.values(clean, cs), lens, lay.n, Nq, Hq, True)
    assert np.ptp(want_lse[np.isfinite(want_lse)]) > 0.05   # the rotary values do move the logits
    q = cm.dev16(torch, dv.pack_rows(lay, qb, np.uint16(cm.NAN16)), fmt)
    for S in (1, 2):
        o, lse = _run8(fa, torch, q, cache, cu, Nq, dl, None, Hq, c_scale=cs, S=S)
        dv.check(oracle, lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"fp8 rope census {cm.FMT_NAME[fmt]} S={S}")


# ---- 5. views and clamps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_strided_q_and_o_views(fa, oracle, torch_cuda, fmt):
    torch = torch_cuda
    case = Case(oracle, torch, "h5", fmt)
    f, lay = case.f, case.lay
    T, Hq = lay.total_q, f["Hq"]
    for S in (1, 2):
        o, lse = case.run(fa, torch, S=S)
        fused = torch.full((T, Hq, mi.DQK + 128), float("nan"), dtype=case.q.dtype, device="cuda")
        fused[:, :, :mi.DQK] = case.q
        wide = _sentinel_out(torch, (T, Hq, mi.DC + 64), torch.float32)
        got = _run8(fa, torch, fused[:, :, :mi.DQK], case.cache, case.cu, f["max_q"], case.lens, None, Hq, S=S, out=wide[:, :, :mi.DC])
        _same(torch, got, (o, lse), f"fp8 fused view S={S}")
        assert (_bits(torch, wide[:, :, mi.DC:]) == dv.SENTINEL_O32).all(), "written outside the O view"
        head_major = case.q.transpose(0, 1).contiguous()
        o_hm = _sentinel_out(torch, (Hq, T, mi.DC), torch.float32)
        got = _run8(fa, torch, head_major.transpose(0, 1), case.cache, case.cu, f["max_q"], case.lens, None, Hq, S=S, out=o_hm.transpose(0, 1))
        _same(torch, got, (o, lse), f"fp8 head-major S={S}")


@pytest.mark.parametrize("fmt", FMTS)
def test_clamps_of_cu_seqlens_q(fa, oracle, torch_cuda, fmt):
    """test_gpu_mla's vector -- a negative entry, a decreasing pair, an entry beyond total_q -- behind guard rows"""
    torch = torch_cuda
    case = Case(oracle, torch, "h5", fmt)
    f = case.f
    Hq, Nq, T, GUARD = f["Hq"], f["max_q"], 16, 5
    raw = [-7, 10, 5, 8, 99]
    lay = dv.Layout(raw, T, Nq)
    clamped = dv.Layout([0, 10, 5, 8, 16], T, Nq)
    assert lay.n == [4, 0, 3, 4] and clamped.n == lay.n and np.array_equal(clamped.tok, lay.tok)
    (qv, _), (qb, _) = mi.inputs(oracle, "h5", fmt)
    q = cm.dev16(torch, dv.pack_rows(lay, qb, np.uint16(cm.NAN16)), fmt)
    want, want_lse = mi.expected_f64(qv, m8.values(m8.codes(oracle, "h5", fmt)), f["lens"], lay.n, Nq, Hq, True)
    for S in (1, 2):
        res = []
        for cu in (raw, clamped.cu):
            obuf = _sentinel_out(torch, (T + 2 * GUARD, Hq, mi.DC), torch.float32)
            lbuf = torch.full((Hq * T + 2 * GUARD * T,), dv.SENTINEL_LSE, dtype=torch.float32, device="cuda")
            o, lse = _run8(fa, torch, q, case.cache, _ints(torch, cu), Nq, case.lens, None, Hq, S=S, out=obuf[GUARD:GUARD + T],
                           lse=lbuf[GUARD * T:GUARD * T + Hq * T].view(Hq, T))
            assert (_bits(torch, obuf[:GUARD]) == dv.SENTINEL_O32).all() and (_bits(torch, obuf[GUARD + T:]) == dv.SENTINEL_O32).all()
            assert (lbuf[:GUARD * T] == dv.SENTINEL_LSE).all() and (lbuf[GUARD * T + Hq * T:] == dv.SENTINEL_LSE).all()
            res.append((o.clone(), lse.clone()))
        _same(torch, res[0], res[1], "the raw vector and its clamp")
        dv.check(oracle, lay, res[0][0].cpu().numpy(), res[0][1].cpu().numpy(), want, want_lse, fmt, f"fp8 clamped cu_seqlens_q S={S}")


# ---- 6. the wide logit range ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 0])
@pytest.mark.parametrize("causal", [pytest.param(True, id="causal"), pytest.param(False, id="full")])
@pytest.mark.parametrize("fmt", FMTS)
def test_wide_logit_range(fa, oracle, torch_cuda, fmt, causal, S):
    """softmax_range_inputs' hostile MLA keys, quantised with c_scale = amax / 448 (mla_fp8_inputs.range_case): the reference is float64
    on the decoded codes, the bounds are softmax_range_inputs.bounds on the decoded values.  tests/test_mla_fp8_inputs.py shows on the
    CPU that EVERY event of the 16-bit tier still fires on the decoded codes -- the staircase of 7 per tile with moves and quiet steps,
    the jumps by 40 and by 150, the fall by 210, the spike the mask hides, the levels of -300 and +300: none is lost to the e4m3
    rounding, so none is left out here.  The paged cache returns the contiguous cache's bits."""
    torch = torch_cuda
    f, lay, rc = sr.MLA, sr.mla_layout(), m8.range_case(fmt)
    q = cm.dev16(torch, sr.mla_packed_q_bits(fmt), fmt)
    cache = cm.dev8(torch, cm.poisoned(rc["codes"][:, None], f["lens"], nan=m8.NAN_CODE)[:, 0])
    cu, lens = _ints(torch, lay.cu), _ints(torch, f["lens"])
    o, lse = _run8(fa, torch, q, cache, cu, f["max_q"], lens, None, f["Hq"], c_scale=rc["c_scale"], causal=causal, S=S)
    want, want_lse = m8.range_reference(fmt, causal)
    vmax = float(np.abs(rc["c"][:, :, :mi.DC]).max())
    sr.check_packed(oracle, lay, o.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, vmax, "fa_mla_decode_fp8",
                    f"{cm.FMT_NAME[fmt]} causal={int(causal)} S={S}")
    cb = rc["codes"][:, None]
    pool, _, table = cm.scatter(cb, cb, f["lens"], 16, 5, nan=m8.NAN_CODE)
    got = _run8(fa, torch, q, cm.dev8(torch, np.ascontiguousarray(pool[:, 0])), cu, f["max_q"], lens, torch.from_numpy(table).cuda(), f["Hq"],
                c_scale=rc["c_scale"], causal=causal, S=S)
    _same(torch, got, (o, lse), f"fp8 wide range pages of 16 S={S}")


# ---- 7. fa_mla_append_fp8 --------------------------------------------------------------------------------------------------------------------
def _append_sources(oracle, fmt, rng, T, c_scale):
    """[T, 640] uint16 encodings (token stride 640): random bit patterns -- NaN, infinities, subnormals and values far beyond
    448 * c_scale among them -- with one token of exact ties between neighbouring codes, +-448 * c_scale and its neighbours, and +-0"""
    new = rng.integers(0, 1 << 16, (T, mi.DQK + 64), dtype=np.uint16)
    mags = f8.TABLE[:0x7F].astype(np.float64)
    ties = (mags[:-1] + mags[1:]) / 2.0                     # 5 significant bits: fp16 and bf16 numbers, and so is each times 2^k
    vals = np.concatenate([ties, -ties, [448.0, -448.0, 464.0, -464.0, 480.0, 0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 2.0 ** -11]])
    row = np.zeros(mi.DQK, np.float32)
    row[:vals.size] = (vals * float(c_scale)).astype(np.float32)
    enc = oracle.encode16(row[None], fmt)[0]
    if float(c_scale) in (0.5, 4.0):
        assert np.array_equal(oracle.decode16(enc[None], fmt)[0], row), "the tie values are exact in the 16-bit type"
    new[3, :mi.DQK] = enc
    return new


@pytest.mark.parametrize("c_scale", [0.5, float(m8.C_SCALE)], ids=["half", "12_448"])
@pytest.mark.parametrize("ps", [pytest.param(0, id="contiguous"), pytest.param(16, id="page16"), pytest.param(64, id="page64")])
@pytest.mark.parametrize("fmt", FMTS)
def test_append_bytes(fa, oracle, torch_cuda, fmt, ps, c_scale):
    """the whole cache or pool, byte for byte, against mla_inputs.append_model on fp8_inputs.encode(x / c_scale): tokens of no sequence,
    drops at the capacity, raw lengths outside the capacity, a strided source; paged: a shuffled table with a -1 and an out-of-range
    entry; every byte no kept token touches is unchanged; the codes are quantize_mla_fp8's on the device; seqlens_out aliasing
    seqlens_k, a separate vector, and none"""
    torch = torch_cuda
    rng = np.random.default_rng(31 + ps + fmt)
    B, cap, T = 4, 128, 14
    cu = [2, 6, 8, 9, 13]
    lens = [126, 17, -4, 500]
    cs = np.float32(c_scale)
    new = _append_sources(oracle, fmt, rng, T, cs)
    with np.errstate(over="ignore", invalid="ignore"):
        want_codes = f8.encode(oracle.decode16(new[:, :mi.DQK], fmt).astype(np.float32) / cs)
    assert (want_codes == 0x7F).any() and (want_codes == 0x7E).any() and (want_codes == 0xFE).any() and (want_codes[3] == 0x80).any()
    if ps:
        max_pages = cap // ps
        num_pages = B * max_pages + 3
        cache = rng.integers(0, 256, (num_pages, ps, mi.DQK), dtype=np.uint8)
        table = rng.permutation(num_pages)[:B * max_pages].astype(np.int32).reshape(B, max_pages)
        table[1, 17 // ps] = -1
        table[2, 0] = num_pages + 5
        dtable = torch.from_numpy(table).cuda()
    else:
        cache, table, dtable = rng.integers(0, 256, (B, cap, mi.DQK), dtype=np.uint8), None, None
    want, want_lens = mi.append_model(cache, want_codes, cu, lens, T, table)
    assert (want != cache).any()
    dnew = cm.dev16(torch, new, fmt)[:, :mi.DQK]
    dscale = _scale(torch, cs)
    q8, s8 = fa.quantize_mla_fp8(dnew, dscale)
    assert s8.data_ptr() == dscale.data_ptr() and np.array_equal(q8.view(torch.uint8).cpu().numpy(), want_codes), "quantize_mla_fp8 on the device"
    for mode in ("alias", "separate", "none"):
        dcache, dl = cm.dev8(torch, cache), _ints(torch, lens)
        out = dl if mode == "alias" else (torch.full((B,), -77, dtype=torch.int32, device="cuda") if mode == "separate" else None)
        fa.fa_mla_append_fp8(dnew, dcache, _ints(torch, cu), cache_seqlens=dl, seqlens_out=out, block_table=dtable, c_scale=dscale)
        torch.cuda.synchronize()
        assert np.array_equal(dcache.view(torch.uint8).cpu().numpy(), want), f"fp8 append bytes page={ps} {mode}"
        if out is not None:
            assert out.cpu().tolist() == list(want_lens), f"lengths page={ps} {mode}"
        if mode != "alias":
            assert dl.cpu().tolist() == lens, "seqlens_k was written"
    # a fresh cache and no scale: no lengths at all, c_scale = 1.0
    dcache = cm.dev8(torch, cache)
    fa.fa_mla_append_fp8(dnew, dcache, _ints(torch, cu), block_table=dtable)
    torch.cuda.synchronize()
    with np.errstate(over="ignore", invalid="ignore"):
        codes1 = f8.encode(oracle.decode16(new[:, :mi.DQK], fmt).astype(np.float32))
    want0, _ = mi.append_model(cache, codes1, cu, None, T, table)
    assert np.array_equal(dcache.view(torch.uint8).cpu().numpy(), want0)


# ---- 8. append -> decode, captured once ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_captured_append_then_decode_follows_its_vectors_and_its_scale(fa, oracle, torch_cuda, fmt):
    """fa_mla_append_fp8 -> fa_mla_decode_fp8 captured once in a (linear) graph and replayed with the tokens, cu_seqlens, the lengths,
    the block table AND c_scale rewritten in place: each replay against the float64 reference of its own state"""
    torch = torch_cuda
    B, Hq, max_q, T, ps, max_pages = 2, 16, 2, 5, 16, 8
    cap, num_pages, tdt = ps * max_pages, 2 * 8 + 4, _tdt(torch, fmt)
    rng = np.random.default_rng(414 + fmt)
    pool0_codes = rng.choice(f8.FINITE_CODES[(f8.FINITE_CODES & 0x7F) < 0x60], (num_pages, ps, mi.DQK))   # |value| < 32 code units
    pool0 = cm.dev8(torch, pool0_codes)
    pool, q, cnew = pool0.clone(), torch.zeros((T, Hq, mi.DQK), dtype=tdt, device="cuda"), torch.zeros((T, mi.DQK), dtype=tdt, device="cuda")
    cu, lens = _ints(torch, [0, 1, 2]), _ints(torch, [0, 0])
    table = torch.zeros((B, max_pages), dtype=torch.int32, device="cuda")
    c_scale = _scale(torch, 1.0)
    out = torch.zeros((T, Hq, mi.DC), dtype=torch.float32, device="cuda")
    lse = torch.zeros((Hq, T), dtype=torch.float32, device="cuda")
    S = 2
    ws = torch.full((fa.mla_decode_workspace_bytes(B, Hq, max_q, max_pages=max_pages, page_size=ps, num_splits=S),), 0xFF, dtype=torch.uint8,
                    device="cuda")
    assert ws.numel() > 0

    def step(pl, ln, o, l):
        fa.fa_mla_append_fp8(cnew, pl, cu, cache_seqlens=ln, seqlens_out=ln, block_table=table, c_scale=c_scale)
        fa.fa_mla_decode_fp8(q, pl, cu, max_q, cache_seqlens=ln, block_table=table, c_scale=c_scale, causal=True, num_splits=S, out=o, lse=l,
                             workspace=ws)

    step(pool.clone(), lens.clone(), out.clone(), lse.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pool, lens, out, lse)
    states = [([1, 3, 4], [100, 37], 0.125), ([0, 1, 2], [0, 126], float(m8.C_SCALE)), ([2, 2, 5], [64, 65], 0.3)]
    for s, (vec, before, cs) in enumerate(states):
        cs = np.float32(cs)
        qb = oracle.encode16(rng.standard_normal((T, Hq, mi.DQK)).astype(np.float32), fmt)
        nb = oracle.encode16(rng.standard_normal((T, mi.DQK)).astype(np.float32), fmt)
        tb = rng.permutation(num_pages)[:B * max_pages].astype(np.int32).reshape(B, max_pages)
        for dst, src in ((q, cm.dev16(torch, qb, fmt)), (cnew, cm.dev16(torch, nb, fmt)), (cu, _ints(torch, vec)), (lens, _ints(torch, before)),
                         (table, torch.from_numpy(tb).cuda()), (pool, pool0), (c_scale, _scale(torch, cs))):
            dst.copy_(src)
        ws.fill_(0xFF)
        out.copy_(_sentinel_out(torch, tuple(out.shape), torch.float32)), lse.fill_(dv.SENTINEL_LSE)
        graph.replay()
        torch.cuda.synchronize()
        want_pool, after = mi.append_model(pool0_codes, f8.encode(oracle.decode16(nb, fmt).astype(np.float32) / cs), vec, before, T, tb)
        assert np.array_equal(pool.view(torch.uint8).cpu().numpy(), want_pool), f"step {s}: the pool after the append"
        assert lens.cpu().tolist() == list(after), f"step {s}: the lengths after the append"
        lay = dv.Layout(vec, T, max_q)
        cache = m8.values(want_pool[tb.reshape(-1)].reshape(B, cap, mi.DQK), cs)
        qpad = dv.unpack_rows(lay, oracle.decode16(qb, fmt), B)
        want, want_lse = mi.expected_f64(qpad, cache, after, lay.n, max_q, Hq, True)
        dv.check(oracle, lay, out.cpu().numpy(), lse.cpu().numpy(), want, want_lse, fmt, f"fp8 replay {s} {cm.FMT_NAME[fmt]} c_scale={cs}")


# ---- 9. the torch ops -------------------------------------------------------------------------------------------------------------------------
def test_torch_ops(fa, oracle, torch_cuda):
    """torch.ops.fa_mi355.mla_append_fp8 and .mla_decode_fp8 are the front end's calls: the same bits"""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    case = Case(oracle, torch, "h16", 0, 16)
    f = case.f
    cs = _scale(torch, m8.C_SCALE)
    o, lse = fa.fa_mla_decode_fp8(case.q, case.cache, case.cu, f["max_q"], cache_seqlens=case.lens, block_table=case.table, c_scale=cs,
                                  return_lse=True, num_splits=2)
    o2, lse2 = torch.ops.fa_mi355.mla_decode_fp8(case.q, case.cache, case.cu, f["max_q"], case.lens, case.table, cs, mi.SCALE, True, 2, True)
    o3, _ = torch.ops.fa_mi355.mla_decode_fp8(case.q, case.cache, case.cu, f["max_q"], case.lens, case.table, None, mi.SCALE, True, 2, True)
    torch.cuda.synchronize()
    owned = torch.from_numpy(case.lay.owned).cuda()
    assert torch.equal(_bits(torch, o2[owned]), _bits(torch, o[owned])) and torch.equal(_bits(torch, lse2[:, owned]), _bits(torch, lse[:, owned]))
    assert (o2[~owned] == 0).all() and (lse2[:, ~owned] == -float("inf")).all()
    assert not torch.equal(_bits(torch, o3[owned]), _bits(torch, o[owned])), "the scale reaches the op"
    o16, _ = torch.ops.fa_mi355.mla_decode_fp8(case.q, case.cache, case.cu, f["max_q"], case.lens, case.table, cs, mi.SCALE, True, 2, False)
    assert o16.dtype == case.q.dtype and o16.shape == (case.q.shape[0], f["Hq"], mi.DC)
    new = case.q[:4, 0].contiguous()
    pools = [case.cache.clone(), case.cache.clone()]
    before, after = _ints(torch, [5, 5, 5]), [torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(2)]
    cu = _ints(torch, [0, 1, 3, 4])
    table = case.table.clamp(0, case.cache.shape[0] - 1)
    fa.fa_mla_append_fp8(new, pools[0], cu, cache_seqlens=before, seqlens_out=after[0], block_table=table, c_scale=cs)
    torch.ops.fa_mi355.mla_append_fp8(new, pools[1], cu, before, after[1], table, cs)
    torch.cuda.synchronize()
    p0, p1, base = (t.view(torch.uint8) for t in (pools[0], pools[1], case.cache))
    assert torch.equal(p0, p1) and not torch.equal(p0, base)
    assert torch.equal(after[0], after[1]) and after[0].tolist() == [6, 7, 6]
