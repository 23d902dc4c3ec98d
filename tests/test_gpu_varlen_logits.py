"""GPU tier of fa_forward_varlen_ex (the packed prefill with a sliding window, soft-capped logits and attention sinks), through the
Python front end, which goes through the C ABI.  Inputs and the float64 reference are tests/varlen_logit_inputs.py's, the check is
tests/varlen_inputs.py's; tests/test_varlen_logit_inputs.py shows without a GPU that the check rejects a kernel that ignores an option
and nine wrong kernels (a window off by one either way or aligned to the start, a first tile taken from the wrong row, a cap after
the masks, a sink that is scaled, counted per tile or given to rows of no sequence).  Every launch writes into O and lse buffers
pre-filled with a poison value."""
import ctypes

import numpy as np
import pytest

import common_inputs as cm
import varlen_inputs as vi
import varlen_logit_inputs as li

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _i32(torch, x):
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device="cuda")


def _f32(torch, x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.float32)).cuda()


def _dev(torch, c):
    return tuple(cm.dev16(torch, c[n], c["fmt"]) for n in ("qb", "kb", "vb"))


def _poisoned(torch, c, shape_q):
    tdt = torch.float32 if c["f32"] else (torch.bfloat16 if c["fmt"] else torch.float16)
    return (torch.full(shape_q, vi.POISON, dtype=tdt, device="cuda"),
            torch.full((shape_q[1], shape_q[0]), vi.POISON, dtype=torch.float32, device="cuda"))


def _opts(torch, c, over):
    o = dict(window=c["W"], softcap=c["softcap"], sinks=c["sinks"], scale=c["scale"], causal=c["causal"])
    o.update(over)
    if not (o["sinks"] is None or hasattr(o["sinks"], "is_cuda")):
        o["sinks"] = _f32(torch, o["sinks"])
    return o


def _run(torch, fa, c, q, k, v, cu_q, cu_k, **over):
    """one launch into poisoned buffers -> (O, lse) device tensors; the case's options unless `over` replaces them"""
    out, lse = _poisoned(torch, c, tuple(q.shape))
    o2, l2 = fa.fa_forward_varlen(q, k, v, cu_q, cu_k, out=out, lse=lse, **_opts(torch, c, over))
    torch.cuda.synchronize()
    assert o2 is out and l2 is lse
    return out, lse


def _raw_ex(torch, fa, c, q, k, v, cu_q, cu_k, opts):
    """fa_forward_varlen_ex itself on contiguous (total, H, d) tensors, `opts` a capi.VarlenOpts or None (a null pointer)"""
    out, lse = _poisoned(torch, c, tuple(q.shape))
    H, Hkv, d = q.shape[1], k.shape[1], q.shape[2]
    desc = fa.capi.VarlenDesc(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=out.data_ptr(), lse=lse.data_ptr(),
                              cu_seqlens_q=cu_q.data_ptr(), cu_seqlens_k=cu_k.data_ptr(), B=cu_q.numel() - 1, Hkv=Hkv, G=H // Hkv, d=d,
                              total_q=q.shape[0], total_k=k.shape[0], q_stride_t=H * d, q_stride_h=d, k_stride_t=Hkv * d, k_stride_h=d,
                              v_stride_t=Hkv * d, v_stride_h=d, o_stride_t=H * d, o_stride_h=d, scale=c["scale"], causal=int(c["causal"]),
                              in_dtype=c["fmt"], out_dtype=0 if c["f32"] else 1, stream=torch.cuda.current_stream().cuda_stream)
    code = fa.lib().fa_forward_varlen_ex(ctypes.byref(desc), None if opts is None else ctypes.byref(opts))
    torch.cuda.synchronize()
    assert code == 0
    return out, lse


def _np(t):
    return t.float().cpu().numpy()


def _judge(c, o, lse, want, want_lse, cu_q, what):
    own = vi.owned(cu_q, o.shape[0])
    got, got_lse = _np(o), _np(lse)
    ma, rl, le = vi.figures(got, got_lse, want, want_lse, own)
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {cm.REL_L2[c['fmt']]:.1e} "
          f"{2 * cm.P_EPS[c['fmt']]:.2e})")
    found = vi.problems(got, got_lse, want, want_lse, own, c["fmt"])
    assert not found, f"{what}: {found}"


def _same(torch, a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", li.CASES, ids=li.case_id)
def test_parity(fa, torch, case):
    c = li.make(case)
    q, k, v = _dev(torch, c)
    assert torch.isnan(q[-vi.TAIL:]).all() and torch.isnan(k[-vi.TAIL:]).all() and torch.isnan(v[-vi.TAIL:]).all()
    o, lse = _run(torch, fa, c, q, k, v, _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"]))
    want, want_lse = li.expected(case)
    _judge(c, o, lse, want, want_lse, c["cu_q"], li.case_id(case))


# ---- 2. ties, bit for bit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (li.CASES[4], li.CASES[1], li.CASES[11]), ids=li.case_id)
def test_options_off_is_the_base_entry(fa, torch, case):
    """a null opts and an all-off opts are fa_forward_varlen; a window no sequence can feel and sinks of -inf change no bit, neither
    against the base entry nor next to another option"""
    c = li.make(case)
    q, k, v = _dev(torch, c)
    cu_q, cu_k = _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"])
    base = _run(torch, fa, c, q, k, v, cu_q, cu_k, window=0, softcap=0.0, sinks=None)       # the front end calls the old symbol
    _same(torch, _raw_ex(torch, fa, c, q, k, v, cu_q, cu_k, None), base, "opts = NULL")
    _same(torch, _raw_ex(torch, fa, c, q, k, v, cu_q, cu_k, fa.capi.VarlenOpts()), base, "all-off opts")
    big = max(a + b for a, b in zip(c["lq"], c["lk"]))
    none = np.full(c["Hkv"] * c["G"], -np.inf, np.float32)
    for W in (big, big + 1, 2 ** 31 - 1):
        _same(torch, _run(torch, fa, c, q, k, v, cu_q, cu_k, window=W, softcap=0.0, sinks=None), base, f"W = {W} alone")
    _same(torch, _run(torch, fa, c, q, k, v, cu_q, cu_k, window=0, softcap=0.0, sinks=none), base, "sinks of -inf alone")
    capped = _run(torch, fa, c, q, k, v, cu_q, cu_k, window=0, softcap=li.SOFTCAP, sinks=None)
    _same(torch, _run(torch, fa, c, q, k, v, cu_q, cu_k, window=big, softcap=li.SOFTCAP, sinks=none), capped, "W, -inf sinks next to a cap")
    assert not torch.equal(capped[1], base[1])
    if c["sinks"] is not None:
        with_s = _run(torch, fa, c, q, k, v, cu_q, cu_k, window=0, softcap=0.0)
        _same(torch, _run(torch, fa, c, q, k, v, cu_q, cu_k, window=big, softcap=0.0), with_s, "W next to sinks")
        # a head whose sink is -inf returns the bits it returns without sinks
        off = torch.from_numpy(~np.isfinite(c["sinks"])).cuda()
        assert off.any() and torch.equal(with_s[0][:, off], base[0][:, off]) and torch.equal(with_s[1][off], base[1][off])


@pytest.mark.parametrize("case", (li.CASES[6], li.CASES[8]), ids=li.case_id)
def test_isolation(fa, torch, case):
    """a sequence alone returns the bits it returned inside the batch"""
    c = li.make(case)
    q, k, v = _dev(torch, c)
    o, lse = _run(torch, fa, c, q, k, v, _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"]))
    ran = 0
    for b, ((sq, eq), (sk, ek)) in enumerate(zip(vi.bounds(c["cu_q"], q.shape[0]), vi.bounds(c["cu_k"], k.shape[0]))):
        if eq == sq:
            continue
        ran += 1
        o1, l1 = _run(torch, fa, c, q[sq:eq].clone(), k[sk:ek + 1].clone(), v[sk:ek + 1].clone(), _i32(torch, [0, eq - sq]),
                      _i32(torch, [0, ek - sk]))     # one key row more than the sequence has: total_k stays positive when Lk = 0
        assert torch.equal(o1, o[sq:eq]) and torch.equal(l1, lse[:, sq:eq]), f"sequence {b} alone"
    assert ran >= 2


# ---- 3. census (exact) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,causal,d,fmt,W", [("self", 1, 64, 0, 17), ("cross", 0, 128, 1, 64), ("long", 1, 128, 0, 100),
                                                  ("long", 0, 64, 1, 1)])
def test_census(fa, torch, batch, causal, d, fmt, W):
    """scale 0 and one-hot V rows: every key of [lo_i, c_i) is counted exactly once and no other; with sinks alternating 0 and -inf a
    head divides by cnt + 1 resp. cnt.  With weights of exactly 1 the fp32 sums are exact, and both decisions -- the row total and
    exp(lse) -- are between neighbouring integers."""
    c = dict(li.make((batch, 2, 2, d, fmt, causal, 1, None, W, 0, 1)))
    Hq = 4
    sinks = np.array([0.0 if h % 2 == 0 else -np.inf for h in range(Hq)], np.float32)
    tq, tk = c["q"].shape[0], c["k"].shape[0]
    bq, bk = vi.bounds(c["cu_q"], tq), vi.bounds(c["cu_k"], tk)
    one = vi.encode16(np.float32([1.0]), fmt)[0]
    vb = np.full(c["vb"].shape, cm.NAN16, np.uint16)
    for b, (sk, ek) in enumerate(bk):
        vb[sk:ek] = 0
        for j in range(ek - sk):
            vb[sk + j, :, (j + 7 * b) % d] = one
    q, k = cm.dev16(torch, c["qb"], fmt), cm.dev16(torch, c["kb"], fmt)
    o, lse = _run(torch, fa, c, q, k, cm.dev16(torch, vb, fmt), _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"]), scale=0.0, sinks=sinks)
    got, got_lse = _np(o).astype(np.float64), _np(lse).astype(np.float64)
    worst = 0.0
    for b, ((sq, eq), (sk, ek)) in enumerate(zip(bq, bk)):
        lo, lim = li.limits(eq - sq, ek - sk, bool(causal), W)
        for i in range(eq - sq):
            cnt = max(int(lim[i] - lo[i]), 0)
            want = np.bincount((np.arange(lo[i], lim[i]) + 7 * b) % d, minlength=d) if cnt else np.zeros(d, np.int64)
            for hq in range(Hq):
                den = cnt + int(np.isfinite(sinks[hq]))
                if den == 0:
                    assert (got[sq + i, hq] == 0).all() and got_lse[hq, sq + i] == -np.inf, (b, i, hq)
                    continue
                n = np.exp(got_lse[hq, sq + i])
                col = got[sq + i, hq] * den
                worst = max(worst, abs(n - den), float(np.abs(col - want).max()), abs(col.sum() - cnt))
                assert np.rint(n) == den and abs(n - den) < 0.25, (b, i, hq, n, den)
                assert (np.rint(col) == want).all() and abs(col.sum() - cnt) < 0.25, (b, i, hq)
    print(f"CENSUS|fa_forward_varlen_ex|{batch} causal={causal} d={d} {cm.FMT_NAME[fmt]} W={W}|{worst:.3e}")
    own = vi.owned(c["cu_q"], tq)
    assert (got[~own] == vi.POISON).all() and (got_lse[:, ~own] == vi.POISON).all()


# ---- 4. second oracle on the device: the decode entry, whose arithmetic a prompt must share --------------------------------------------
@pytest.mark.parametrize("case", (li.CASES[6], li.CASES[8], li.CASES[10], li.CASES[15]), ids=li.case_id)
def test_against_the_decode_entry(fa, torch, case):
    """per sequence, fa_forward_kvcache with window=, sinks=, softcap= on [1,Hq,Lq,d] x [1,Hkv,Lk,d] has the same semantics"""
    c = li.make(case)
    q, k, v = _dev(torch, c)
    o, lse = _run(torch, fa, dict(c, f32=True), q, k, v, _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"]))
    sinks = _f32(torch, c["sinks"])
    vmax = float(np.abs(c["v"][:-vi.TAIL]).max())
    tol, ltol = cm.peaked_tol(c["fmt"], vmax, kernels=2), 4 * cm.P_EPS[c["fmt"]]
    worst = [0.0, 0.0]
    for b, ((sq, eq), (sk, ek)) in enumerate(zip(vi.bounds(c["cu_q"], q.shape[0]), vi.bounds(c["cu_k"], k.shape[0]))):
        if eq == sq or ek == sk:
            continue
        o1, l1 = fa.fa_forward_kvcache(q[sq:eq].transpose(0, 1).contiguous()[None], k[sk:ek].transpose(0, 1).contiguous()[None],
                                       v[sk:ek].transpose(0, 1).contiguous()[None], causal=c["causal"], scale=c["scale"],
                                       out_dtype=torch.float32, return_lse=True, window=c["W"], sinks=sinks, softcap=c["softcap"])
        torch.cuda.synchronize()
        a, al = _np(o[sq:eq]).transpose(1, 0, 2), _np(lse[:, sq:eq])
        r, rl = _np(o1[0]), _np(l1[0])
        assert (np.isfinite(al) == np.isfinite(rl)).all(), b
        live = np.isfinite(rl)
        worst = [max(worst[0], float(np.abs(a - r).max())), max(worst[1], float(np.abs(al[live] - rl[live]).max(initial=0.0)))]
        assert np.abs(a - r).max() <= tol and np.abs(al[live] - rl[live]).max(initial=0.0) <= ltol, (b, worst)
    print(f"{li.case_id(case)}: against fa_forward_kvcache max_abs={worst[0]:.3e} (tol {tol:.3e}) lse={worst[1]:.3e} (tol {ltol:.3e})")


# ---- 5. what is not read ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (li.CASES[8], li.CASES[15]), ids=li.case_id)
def test_rows_below_the_first_tile_are_not_read(fa, torch, case):
    """causal and windowed: the K/V rows of a sequence below the first streamed tile of its FIRST workgroup (no later one starts lower)
    hold NaN, and the result keeps its bits"""
    c = li.make(case)
    assert c["causal"] and c["W"]
    q, k, v = _dev(torch, c)
    cu_q, cu_k = _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"])
    o, lse = _run(torch, fa, c, q, k, v, cu_q, cu_k)
    nan = torch.tensor([cm.NAN16], dtype=torch.int16).view(q.dtype).cuda()
    kn, vn = k.clone(), v.clone()
    hidden = 0
    for (sq, eq), (sk, ek) in zip(vi.bounds(c["cu_q"], q.shape[0]), vi.bounds(c["cu_k"], k.shape[0])):
        if eq == sq:
            continue
        below = max(0, (ek - sk) - (eq - sq) + 1 - c["W"]) // li.TILE * li.TILE      # lo of row 0, down to its tile
        kn[sk:sk + below] = nan
        vn[sk:sk + below] = nan
        hidden += below
    assert hidden >= li.TILE
    _same(torch, _run(torch, fa, c, q, kn, vn, cu_q, cu_k), (o, lse), "NaN below the first tile")


# ---- 6. captured call ------------------------------------------------------------------------------------------------------------------
def test_captured_call_follows_rewritten_vectors_and_sinks(fa, torch):
    case = li.CASES[6]                     # cross, causal, W = 100, cap and sinks
    c = li.make(case)
    q, k, v = _dev(torch, c)
    cu_q, cu_k, sinks = _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"]), _f32(torch, c["sinks"])
    new_q, new_k = vi.cu_of((100, 0, 215, 64, 8, 128)), vi.cu_of((50, 300, 1, 90, 72, 128))    # the same totals, one sequence empty
    new_s = np.array([-np.inf, 0.75, 2.5], np.float32)
    assert new_q[-1] == c["cu_q"][-1] and new_k[-1] == c["cu_k"][-1] and new_s.shape == c["sinks"].shape
    eager0 = _run(torch, fa, c, q, k, v, cu_q, cu_k, sinks=sinks)
    eager1 = _run(torch, fa, c, q, k, v, _i32(torch, new_q), _i32(torch, new_k), sinks=new_s)
    assert not torch.equal(eager0[1], eager1[1])
    out, lse = _poisoned(torch, c, tuple(q.shape))
    kw = dict(causal=c["causal"], scale=c["scale"], window=c["W"], softcap=c["softcap"], sinks=sinks, out=out, lse=lse)
    fa.fa_forward_varlen(q, k, v, cu_q, cu_k, **kw)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.fa_forward_varlen(q, k, v, cu_q, cu_k, **kw)
    for vec_q, vec_k, vec_s, eager in ((c["cu_q"], c["cu_k"], c["sinks"], eager0), (new_q, new_k, new_s, eager1)):
        cu_q.copy_(_i32(torch, vec_q)), cu_k.copy_(_i32(torch, vec_k)), sinks.copy_(_f32(torch, vec_s))
        out.fill_(vi.POISON), lse.fill_(vi.POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(lse, eager[1])
    want, want_lse = li.varlen_logits_f64(c["q"], c["k"], c["v"], new_q, new_k, c["Hkv"], c["G"], c["causal"], c["scale"], W=c["W"],
                                          softcap=c["softcap"], sinks=new_s)
    _judge(c, out, lse, want, want_lse, new_q, "replayed on rewritten vectors and sinks")


# ---- 7. the torch op -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (li.CASES[6], li.CASES[3], li.CASES[9]), ids=li.case_id)
def test_torch_op_returns_the_front_ends_bits(fa, torch, case):
    from flashattention_kernel_project_amd.torch_op import register
    register()
    c = li.make(case)
    q, k, v = _dev(torch, c)
    cu_q, cu_k = _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"])
    o, lse = _run(torch, fa, c, q, k, v, cu_q, cu_k)
    o2, l2 = torch.ops.fa_mi355.forward_varlen_ex(q, k, v, cu_q, None if case[0] == "self" else cu_k, c["scale"], c["causal"], c["W"],
                                                  _f32(torch, c["sinks"]), c["softcap"], c["f32"])
    torch.cuda.synchronize()
    own = torch.from_numpy(vi.owned(c["cu_q"], q.shape[0])).cuda()
    assert o2.dtype == o.dtype and torch.equal(o2[own], o[own]) and torch.equal(l2[:, own], lse[:, own])


# ---- 8. layouts ------------------------------------------------------------------------------------------------------------------------
def test_head_major_layout(fa, torch):
    """(H, total, d) through .transpose(0, 1) gives the bits of (total, H, d); O goes through its own strides"""
    c = li.make(li.CASES[6])
    q, k, v = _dev(torch, c)
    cu_q, cu_k = _i32(torch, c["cu_q"]), _i32(torch, c["cu_k"])
    o, lse = _run(torch, fa, c, q, k, v, cu_q, cu_k)
    q2, k2, v2 = (t.transpose(0, 1).contiguous().transpose(0, 1) for t in (q, k, v))
    assert not q2.is_contiguous() and q2.stride(2) == 1
    obuf = torch.full((q.shape[1], q.shape[0], c["d"]), vi.POISON, dtype=o.dtype, device="cuda")
    l2 = torch.full_like(lse, vi.POISON)
    fa.fa_forward_varlen(q2, k2, v2, cu_q, cu_k, out=obuf.transpose(0, 1), lse=l2, **_opts(torch, c, {}))
    torch.cuda.synchronize()
    assert torch.equal(obuf.transpose(0, 1), o) and torch.equal(l2, lse)
