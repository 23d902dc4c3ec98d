"""GPU tier of the per-sequence counts of the KV-cache step: `seqlens_q` on the four decode front ends (fa_kvcache_decode) and
`seqlens_new` on the four append front ends (fa_kvcache_append_ex).

Inputs, the float64 reference and the placement are tests/ragged_inputs.py's (its CPU tier, tests/test_ragged_inputs.py, shows that no
causal parity launch here passes on a kernel that ignores seqlens_q).  Bounds are the project's: the max-abs bar and the relative-L2
bounds on O, 2 * P_EPS absolute on the log-sum-exp of live rows with a key, exact 0 and -inf elsewhere.

Poison: the workspace is filled with NaN bytes; every cache row at or past L_b holds NaN bit patterns; every pool page no table names
holds NaN; every table entry past the live pages holds garbage.
"""
import numpy as np
import pytest

import append_inputs as ai
import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import flat_entries as fe
import fp8_inputs as f8
import logit_inputs as li
import ragged_inputs as ri
import rope_inputs as rp

pytestmark = pytest.mark.gpu

FMT_D = [pytest.param(fmt, d, id=f"{cm.FMT_NAME[fmt]}-d{d}") for d in (64, 128) for fmt in (0, 1)]
NAMES = list(ri.FAMILIES)
MASKS = [pytest.param(c, W, id=f"{'causal' if c else 'full'}-W{W}") for c in (True, False) for W in ri.WINDOWS]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ints(torch, values):
    return None if values is None else torch.tensor(list(values), dtype=torch.int32, device="cuda")


def _floats(torch, values):
    return None if values is None else torch.tensor(np.asarray(values, np.float32), dtype=torch.float32, device="cuda")


def _nan_workspace(torch, need):
    return torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")   # fp32 0xFFFFFFFF is a NaN


def _run(fa, torch, f, d, fmt, qb, kb, vb, nq, W, causal, ps=0, seed=0, sinks=None, softcap=0.0, fp8=False, k_scale=None, v_scale=None,
         check_S=True):
    """One decode launch of a family: qb [B*Hq, Nq, d] encodings; kb, vb [B*Hkv, Ncap, d] encodings (fp8: codes), poisoned here at and
    past L_b; ps = 0 the contiguous entry, else the paged one on the scattered cache; nq a list, or None: the call without counts, which is
    the flat entry fa_forward_kvcache[_window] through the C ABI (tests/flat_entries.py).
    -> O, lse (device tensors)"""
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    lens = f["lens"]
    need = fa.kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, W)
    if check_S:
        assert di.splits_of(need, B * Hkv, G * Nq, d) == ri.want_S(f, W)
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    dev = (lambda a: cm.dev8(torch, a)) if fp8 else (lambda a: cm.dev16(torch, a, fmt))
    kw = dict(cache_seqlens=_ints(torch, lens), causal=causal, return_lse=True, workspace=_nan_workspace(torch, need), window=W,
              sinks=_floats(torch, sinks), softcap=softcap)
    if nq is not None:
        kw["seqlens_q"] = _ints(torch, nq)
    if fp8:
        kw.update(k_scale=_floats(torch, k_scale), v_scale=_floats(torch, v_scale))
    nan = f8.NAN_CODES[0] if fp8 else cm.NAN16
    kc, vc = (x.reshape(B, Hkv, Ncap, d) for x in (kb, vb))
    if nq is None:
        assert ps == 0 and not fp8 and sinks is None and softcap == 0.0
        o, lse = fe.decode(fa, torch, dq, dev(cm.poisoned(kc, lens, nan=nan)), dev(cm.poisoned(vc, lens, nan=nan)), kw["cache_seqlens"],
                           causal, fmt, kw["workspace"], window=W or None)
    elif ps == 0:
        o, lse = (fa.fa_forward_kvcache_fp8 if fp8 else fa.fa_forward_kvcache)(dq, dev(cm.poisoned(kc, lens, nan=nan)),
                                                                               dev(cm.poisoned(vc, lens, nan=nan)), **kw)
    else:
        kp, vp, table = cm.scatter(kc, vc, lens, ps, seed, nan=nan)
        o, lse = (fa.fa_forward_kvcache_paged_fp8 if fp8 else fa.fa_forward_kvcache_paged)(dq, dev(kp), dev(vp), torch.from_numpy(table).cuda(),
                                                                                       **kw)
    torch.cuda.synchronize()
    assert o.shape == dq.shape and lse.shape == dq.shape[:3] and lse.dtype == torch.float32
    return o, lse


def _check(oracle, o, lse, want, want_lse, live_rows, fmt, what):
    """the project's bounds; rows whose reference lse is -inf (dead rows, and live rows without a key or a sink) are exact 0 / -inf"""
    want = np.asarray(want, np.float32)
    got = o.float().cpu().numpy().reshape(want.shape)
    got_lse = lse.cpu().numpy().reshape(want_lse.shape)
    ma, rl = oracle.max_abs(got, want), oracle.rel_l2(got, want)
    fin = np.isfinite(want_lse)
    le = float(np.abs(got_lse[fin] - want_lse[fin]).max()) if fin.any() else 0.0
    print(f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e} lse_abs={le:.3e} (bounds {cm.MAX_ABS:.1e} {cm.REL_L2[fmt]:.1e} {2 * cm.P_EPS[fmt]:.2e})")
    assert np.isfinite(got).all(), what + ": O is not finite"
    assert not np.isnan(got_lse).any(), what + ": NaN in lse"
    assert (got[~live_rows] == 0.0).all() and (got_lse[~live_rows] == -np.inf).all(), what + ": a dead row is not exactly 0 / -inf"
    assert (got[~fin] == 0.0).all() and (got_lse[~fin] == -np.inf).all(), what + ": a row without a key is not exactly 0 / -inf"
    nokey = live_rows & (np.abs(want).max(-1) == 0)
    assert (got[nokey] == 0.0).all(), what + ": a live row without a key is not exactly zero"
    assert ma <= cm.MAX_ABS and rl <= cm.REL_L2[fmt], f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"
    assert np.isfinite(got_lse[fin]).all() and le <= 2 * cm.P_EPS[fmt], f"{what}: lse off by {le:.3e}"


def _pages(f):
    """the page sizes of the bit ties that divide the family's capacity (blocks' 200 rows are a multiple of neither)"""
    return [ps for ps in (16, 256) if f["Ncap"] % ps == 0]


def _same(torch, a, b, what):
    for x, y, n in zip(a, b, ("O", "lse")):
        assert torch.equal(x, y), f"{what}: {n} differs in {int((x != y).sum())} places"


# ---- 1., 2. parity; NaN in every dead Q row changes no bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("causal,W", MASKS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity_and_dead_row_poison(fa, oracle, torch_cuda, fmt, d, name, causal, W):
    torch, f = torch_cuda, ri.FAMILIES[name]
    _, (qb, kb, vb) = ri.inputs(oracle, name, d, fmt)
    want, want_lse = ri.reference(oracle, name, d, fmt, W, causal)
    live = ri.live_rows(name)
    first = _run(fa, torch, f, d, fmt, qb, kb, vb, f["nq"], W, causal)
    _check(oracle, *first, want, want_lse, live, fmt, f"{name} {'causal' if causal else 'full'} W={W}")
    second = _run(fa, torch, f, d, fmt, ri.poison_dead_q(qb, name), kb, vb, f["nq"], W, causal)
    _same(torch, second, first, "dead Q rows of NaN")


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_parity_with_sinks_and_softcap(fa, oracle, torch_cuda, fmt, d):
    """both options on the logits together with the counts: one pass (spec) and behind the merge (split); a live row without a key
    has the sink's logit, a dead row of the same head -inf"""
    torch = torch_cuda
    for name, causal, W in (("spec", True, 100), ("split", True, 0)):
        f = ri.FAMILIES[name]
        sinks = li.sinks_for(f["Hkv"] * f["G"])
        _, (qb, kb, vb) = ri.inputs(oracle, name, d, fmt)
        want, want_lse = ri.reference(oracle, name, d, fmt, W, causal, variant="both")
        o, lse = _run(fa, torch, f, d, fmt, ri.poison_dead_q(qb, name), kb, vb, f["nq"], W, causal, sinks=sinks, softcap=li.SOFTCAP)
        _check(oracle, o, lse, want, want_lse, ri.live_rows(name), fmt, f"{name} sinks + softcap")


# ---- 3. bit ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if _pages(ri.FAMILIES[n])])
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_paged_returns_the_contiguous_bits(fa, oracle, torch_cuda, fmt, d, name):
    torch, f = torch_cuda, ri.FAMILIES[name]
    _, (qb, kb, vb) = ri.inputs(oracle, name, d, fmt)
    for causal, W in ((True, 0), (False, 100)):
        base = _run(fa, torch, f, d, fmt, qb, kb, vb, f["nq"], W, causal)
        for ps in _pages(f):
            _same(torch, _run(fa, torch, f, d, fmt, qb, kb, vb, f["nq"], W, causal, ps=ps, seed=ps), base, f"{name} pages of {ps}")


@pytest.mark.parametrize("fmt,d", FMT_D)
def test_fp8_ties_and_per_head_scales(fa, oracle, torch_cuda, fmt, d):
    torch = torch_cuda
    for name, causal, W in (("spec", True, 0), ("split", True, 0), ("blocks", False, 100)):
        f = ri.FAMILIES[name]
        B, Hkv, G, Nq, Ncap = ri.shape(f)
        (q, k, v), (qb, _, _) = ri.inputs(oracle, name, d, fmt)
        k8, v8 = f8.encode(k), f8.encode(v)
        kw, vw = (oracle.encode16(f8.decode(x), fmt) for x in (k8, v8))            # the widened cache: exact in both formats
        wide = _run(fa, torch, f, d, fmt, qb, kw, vw, f["nq"], W, causal)
        _same(torch, _run(fa, torch, f, d, fmt, qb, k8, v8, f["nq"], W, causal, fp8=True), wide, f"{name} fp8, scales of 1")
        if _pages(f):
            _same(torch, _run(fa, torch, f, d, fmt, qb, k8, v8, f["nq"], W, causal, fp8=True, ps=16, seed=5), wide, f"{name} paged fp8")
        # per-head scales: the reference on the dequantised cache, the project's bounds
        ks, vs = np.array([0.5 + 0.25 * h for h in range(Hkv)], np.float32), np.array([2.0 - 0.5 * h for h in range(Hkv)], np.float32)
        kd = f8.decode(k8) * np.tile(ks, B)[:, None, None]
        vd = f8.decode(v8) * np.tile(vs, B)[:, None, None]
        want, want_lse = cm.expected_f64(q, kd, vd, f["lens"], B, Hkv, G, Nq, causal, W, nq=f["nq"])
        o, lse = _run(fa, torch, f, d, fmt, qb, k8, v8, f["nq"], W, causal, fp8=True, k_scale=ks, v_scale=vs)
        _check(oracle, o, lse, want, want_lse, ri.live_rows(name), fmt, f"{name} fp8 per-head scales")


@pytest.mark.parametrize("name", NAMES + list(ri.EXTRA))
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_full_counts_are_the_call_without_and_negative_counts_are_zero(fa, oracle, torch_cuda, fmt, d, name):
    """the three families and ri.EXTRA's shape with a partly filled wave, whose lanes past Nq must keep the un-ragged kernel's limits"""
    torch, f = torch_cuda, ri.family(name)
    B, Nq = f["B"], f["Nq"]
    _, (qb, kb, vb) = ri.inputs(oracle, name, d, fmt)
    for causal, W in ((True, 0), (True, 100), (False, 0)):
        plain = _run(fa, torch, f, d, fmt, qb, kb, vb, None, W, causal)
        assert torch.isfinite(plain[0]).all()
        for nq in ([Nq] * B, [Nq + b * 1000 for b in range(B)], [2 ** 31 - 1] * B):
            _same(torch, _run(fa, torch, f, d, fmt, qb, kb, vb, nq, W, causal), plain, f"{name} counts {nq}")
        for ps in _pages(f)[:1]:
            _same(torch, _run(fa, torch, f, d, fmt, qb, kb, vb, [Nq] * B, W, causal, ps=ps, seed=1), plain, f"{name} paged, full counts")
    # negative entries are the count 0
    zero = _run(fa, torch, f, d, fmt, qb, kb, vb, [0, *f["nq"][1:]], 0, True)
    for bad in (-1, -2 ** 31):
        _same(torch, _run(fa, torch, f, d, fmt, qb, kb, vb, [bad, *f["nq"][1:]], 0, True), zero, f"a count of {bad}")
    assert (zero[0][0] == 0).all() and (zero[1][0] == float("-inf")).all() and torch.isfinite(zero[1][1]).any() == (f["nq"][1] > 0)


# ---- 4. census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal,W", MASKS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_census(fa, oracle, torch_cuda, fmt, d, name, causal, W):
    """K = 0 and V in the residue coding: every live row counts each key it sees exactly once, decided between neighbouring integers;
    sinks alternate between 0 and -inf; dead rows are exact zeros"""
    torch, f = torch_cuda, ri.FAMILIES[name]
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    z = ci.z_decode(oracle, B, Hkv, G, Nq, Ncap, d, fmt, "residue")
    lo, c, live = ri.limits(f["lens"], f["nq"], B, Hkv, G, Nq, Ncap, causal, W)
    S, m_q = ci.decode_sums(z["m"], lo, c, G, Ncap, d, "residue")
    assert ci.z_exact(fmt, float(S.max()))
    sinks = li.census_sinks(Hkv * G)
    sink = np.tile(np.isfinite(sinks), B).astype(np.int64)
    qb, kb, vb = z["bits"]
    for ps in [0] + _pages(f)[:1]:
        o, lse = _run(fa, torch, f, d, fmt, ri.poison_dead_q(qb, name), kb, vb, f["nq"], W, causal, ps=ps, seed=9, sinks=sinks)
        ri.census_check(ci, o.cpu().numpy(), lse.cpu().numpy(), S, c - lo, m_q, sink, live, f"{name} census ps={ps}")


# ---- 5. append bytes ------------------------------------------------------------------------------------------------------------------
APPEND = dict(B=4, Hkv=2, G=2, Nnew=5, Ncap=64, ps=16, lens=(0, 14, 60, 30), new=(5, 3, 5, 0), seed=8400)
# rope: 0 no rotation, 1 half-split pairs, 2 interleaved pairs
FORMS = [pytest.param(p, q, r, id=("paged_" if p else "") + ("fp8_" if q else "") + ("plain", "rope", "rope_il")[r])
         for p in (False, True) for q in (False, True) for r in (0, 1, 2)]


def _append_table(a):
    """every page below the length after the (ragged) append is the sequence's own; the slot behind it -- which only padding tokens
    would reach -- names ANOTHER sequence's valid page where such a slot exists; the rest is garbage"""
    B, ps, Ncap = a["B"], a["ps"], a["Ncap"]
    max_pages = Ncap // ps
    after = ri.lens_after(a["lens"], a["new"], B, a["Nnew"], Ncap)
    num_pages = B * max_pages + 3
    perm = np.random.default_rng(a["seed"]).permutation(num_pages)
    table = np.empty((B, max_pages), np.int32)
    nxt, first = 0, {}
    for b in range(B):
        for pi in range(max_pages):
            if pi * ps < after[b]:
                table[b, pi] = perm[nxt]
                first.setdefault(b, int(perm[nxt]))
                nxt += 1
            else:
                table[b, pi] = cm.GARBAGE[pi % 2]
    foreign = []
    for b in range(B):
        L = cm.clamp(a["lens"][b], Ncap)
        padded_end = min(L + a["Nnew"], Ncap)
        for pi in range(-(-int(after[b]) // ps), -(-padded_end // ps)):          # slots only tokens t >= m_b would reach
            other = next(x for x in first if x != b)
            table[b, pi] = first[other]
            foreign.append((b, pi))
    return table, num_pages, foreign


@pytest.mark.parametrize("paged,fp8,rope", FORMS)
@pytest.mark.parametrize("fmt,d", FMT_D)
def test_append_bytes(fa, oracle, torch_cuda, fmt, d, paged, fp8, rope):
    import ctypes
    torch, a = torch_cuda, APPEND
    B, Hkv, G, Nnew, Ncap, ps, lens, new = (a[x] for x in ("B", "Hkv", "G", "Nnew", "Ncap", "ps", "lens", "new"))
    Hq, il = Hkv * G, rope == 2
    _, (qsrc, kdrawn, _) = di.inputs(oracle, B, Hkv, G, Nnew, Ncap, d, fmt, a["seed"])
    qsrc = qsrc.reshape(B, Hq, Nnew, d)
    if fp8:
        ks, vs = np.array([0.5, 1.75], np.float32), np.array([2.0, 0.37], np.float32)
        knb = ai.fp8_new_rows(B, Hkv, Nnew, d, ks, fmt, a["seed"] + 1)       # every code's value, the midpoints, beyond 448
        vnb = ai.fp8_new_rows(B, Hkv, Nnew, d, vs, fmt, a["seed"] + 2)
    else:
        ks = vs = None
        knb, vnb = (ai.random_bytes((B, Hkv, Nnew, d), 2, a["seed"] + s) for s in (1, 2))   # every pattern, NaN payloads included
    if rope:   # a rotated NaN's payload is not promised, nor is inf - inf: K is rotated from drawn, finite rows
        knb = np.ascontiguousarray(kdrawn.reshape(B, Hkv, Ncap, d)[:, :, :Nnew])
    cos, sin = rp.scrambled_table(40, d // 4, a["seed"])                                    # rot_dim = d / 2, max_pos < Ncap: the clamp
    item = 1 if fp8 else 2
    table, foreign = None, []
    if paged:
        table, num_pages, foreign = _append_table(a)
        assert foreign, "the table has no slot that only padding would reach"
        shape = (num_pages, Hkv, ps, d)
    else:
        shape = (B, Hkv, Ncap, d)
    kc0, vc0 = ai.random_bytes(shape, item, a["seed"] + 3), ai.random_bytes(shape, item, a["seed"] + 4)
    # the expected rows, in the cache's element type
    if rope:
        krot = rp.rotated_rows_fp32(knb, fmt, lens, Ncap, cos, sin, il)
        krows = rp.fp8_codes(krot, ks) if fp8 else rp.rotated_rows16(knb, fmt, lens, Ncap, cos, sin, il)
        qrot = rp.rotated_rows16(qsrc, fmt, lens, Ncap, cos, sin, il)
        qwant = ri.keep_dead_q(qrot, qsrc, new)
        assert not np.array_equal(qwant, qrot) and not np.array_equal(qwant, qsrc)          # kept and rotated rows both occur
    else:
        krows = rp.fp8_codes(ai.widen16(knb, fmt), ks) if fp8 else knb
    vrows = rp.fp8_codes(ai.widen16(vnb, fmt), vs) if fp8 else vnb
    fn = getattr(fa, "fa_kvcache_append" + ("_paged" if paged else "") + ("_fp8" if fp8 else ""))

    def launch(new_counts, flat=False, table=table, disjoint=False, by_desc=False):
        """-> K, V, lengths, Qout, Q after one append.  flat: no seqlens_new, the flat entry of the form through the C ABI
        (tests/flat_entries.py); by_desc: the same through fa_kvcache_append_ex with seqlens_new = NULL; neither: the Python front
        end with seqlens_new = new_counts; disjoint: Q goes to a NaN-filled q_out of its own instead of in place"""
        dev = (lambda x: cm.dev8(torch, x)) if fp8 else (lambda x: cm.dev16(torch, x, fmt))
        dk, dv, dl = dev(kc0), dev(vc0), _ints(torch, lens)
        dkn, dvn = cm.dev16(torch, knb, fmt), cm.dev16(torch, vnb, fmt)
        dq = cm.dev16(torch, qsrc, fmt) if rope else None
        dqo = cm.dev16(torch, np.full(qsrc.shape, cm.NAN16, np.uint16), fmt) if rope and disjoint else dq
        dt = torch.from_numpy(table).cuda() if paged else None
        dks, dvs, dcos, dsin = _floats(torch, ks), _floats(torch, vs), _floats(torch, cos), _floats(torch, sin)
        if by_desc:
            ptr = lambda t: None if t is None else t.data_ptr()
            desc = fa.capi.KvAppendDesc(
                Knew=ptr(dkn), Vnew=ptr(dvn), K=ptr(dk), V=ptr(dv), seqlens_k=ptr(dl), seqlens_out=ptr(dl), block_table=ptr(dt),
                k_scale=ptr(dks), v_scale=ptr(dvs), Q=ptr(dq), Qout=ptr(dqo), rope_cos=ptr(dcos) if rope else None,
                rope_sin=ptr(dsin) if rope else None, kv_dtype=fa.capi.KV_FP8_E4M3 if fp8 else fa.capi.KV_16BIT, B=B, Hkv=Hkv, Nnew=Nnew,
                d=d, Ncap=0 if paged else Ncap, num_pages=shape[0] if paged else 0, page_size=ps if paged else 0,
                max_pages=Ncap // ps if paged else 0, G=G if rope else 0, rot_dim=d // 2 if rope else 0, max_pos=cos.shape[0] if rope else 0,
                interleaved=int(il), dtype=fmt, stream=torch.cuda.current_stream().cuda_stream)
            assert fa.lib().fa_kvcache_append_ex(ctypes.byref(desc)) == 0
        elif flat:
            fe.append(fa, torch, dkn, dvn, dk, dv, dl, dl, fmt, table=dt, scales=(dks, dvs) if fp8 else None,
                      rope=(dq, dqo, dcos, dsin, il) if rope else None)
        else:
            args = [dkn, dvn, dk, dv] + ([dt] if paged else [])
            kw = dict(cache_seqlens=dl, seqlens_out=dl, seqlens_new=_ints(torch, new_counts))
            if fp8:
                kw.update(k_scale=dks, v_scale=dvs)
            if rope:
                kw.update(q=dq, rotary_cos=dcos, rotary_sin=dsin, rotary_interleaved=il)
                if disjoint:
                    kw.update(q_out=dqo)
            fn(*args, **kw)
        torch.cuda.synchronize()
        u = torch.uint8 if fp8 else torch.int16
        out = [x.view(u).cpu().numpy().view(np.uint8 if fp8 else np.uint16) for x in (dk, dv)]
        q16 = [x.view(torch.int16).cpu().numpy().view(np.uint16) if rope else None for x in (dqo, dq)]
        return out[0], out[1], dl.cpu().numpy(), q16[0], q16[1]

    def same(x, y):
        return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(x, y))

    wantk, wantv = ri.place(kc0, krows, lens, new, table), ri.place(vc0, vrows, lens, new, table)
    for disjoint in (False, True) if rope else (False,):
        gk, gv, gl, gqo, gq = launch(new, disjoint=disjoint)
        assert np.array_equal(gk, wantk), "K: the whole cache against the placement"
        assert np.array_equal(gv, wantv), "V: the whole cache against the placement"
        assert gl.tolist() == ri.lens_after(lens, new, B, Nnew, Ncap).tolist()
        if rope:
            assert np.array_equal(gqo, qwant), "Qout: rotated rows of kept tokens, the source bits of the rest"
            if disjoint:   # every byte of the NaN-filled q_out was written, and the source is as it was
                assert np.array_equal(gq, qsrc), "Q was written although q_out is a buffer of its own"
    # a slot that only padding would reach names another sequence's page: that page is what its owner alone made of it
    own = None
    if paged:
        own = table.copy()
        for b, pi in foreign:
            own[b, pi] = cm.GARBAGE[0]
        for b, pi in foreign:
            page = int(table[b, pi])
            assert np.array_equal(gk[page], ri.place(kc0, krows, lens, new, own)[page])
            assert np.array_equal(gv[page], ri.place(vc0, vrows, lens, new, own)[page])
    # m_b = Nnew everywhere (and beyond) is the flat entry, and so is the descriptor with seqlens_new = NULL: same bytes.  (On the
    # table with the borrowed slots back at garbage: with every token kept two sequences would write one page.)
    flat = launch(None, flat=True, table=own)
    assert flat[2].tolist() == ai.lens_after(lens, B, Nnew, Ncap).tolist()
    assert same(launch(None, table=own, by_desc=True), flat), "fa_kvcache_append_ex without seqlens_new"
    for counts in ([Nnew] * B, [Nnew + 7] * B):
        assert same(launch(counts, table=own), flat), counts
    if rope:
        flat_out = launch(None, flat=True, table=own, disjoint=True)
        assert np.array_equal(flat_out[3], flat[3]) and np.array_equal(flat_out[4], qsrc)
        assert same(launch([Nnew] * B, table=own, disjoint=True), flat_out)
        assert same(launch(None, table=own, disjoint=True, by_desc=True), flat_out)


# ---- 6. the captured step -------------------------------------------------------------------------------------------------------------
def test_captured_ragged_step(fa, oracle, torch_cuda):
    """append (paged, rotary, lengths in place, seqlens_new) -> decode (seqlens_q = the same tensor), captured once as a linear graph
    and replayed three times with the counts rewritten in place; O and lse against the reference on a cache kept on the CPU"""
    torch = torch_cuda
    fmt, d, B, Hkv, G, N, Ncap, ps = 0, 64, 3, 2, 2, 4, 64, 16
    Hq = Hkv * G
    steps = ((4, 1, 0), (1, 1, 2), (0, 4, 1))
    lens = [10, 31, 0]
    (q, k, v), (qb, kb, vb) = di.inputs(oracle, B, Hkv, G, 3 * N, Ncap, d, fmt, 8600)
    kcpu, vcpu = np.zeros((B * Hkv, Ncap, d), np.float32), np.zeros((B * Hkv, Ncap, d), np.float32)
    max_pages = Ncap // ps
    table = np.random.default_rng(8600).permutation(B * max_pages + 3)[:B * max_pages].astype(np.int32).reshape(B, max_pages)
    num_pages = B * max_pages + 3
    nan_pool = np.full((num_pages, Hkv, ps, d), cm.NAN16, np.uint16)
    for b in range(B):                                  # the keys the sequences start with: rows 0 .. L_b - 1 of the drawn cache
        kcpu[b * Hkv:(b + 1) * Hkv, :lens[b]] = k[b * Hkv:(b + 1) * Hkv, :lens[b]]
        vcpu[b * Hkv:(b + 1) * Hkv, :lens[b]] = v[b * Hkv:(b + 1) * Hkv, :lens[b]]
    kb4, vb4 = kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d)
    kp = ri.place(nan_pool, kb4, None, lens, table)     # a ragged "append into an empty cache" places the start
    vp = ri.place(nan_pool, vb4, None, lens, table)
    dkp, dvp, dt, dl = cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(table).cuda(), _ints(torch, lens)
    # angle 0: the fused rotation is on the captured path, and K and Q arrive as they were drawn
    cos = torch.ones(Ncap, d // 2, dtype=torch.float32, device="cuda")
    sin = torch.zeros(Ncap, d // 2, dtype=torch.float32, device="cuda")
    dn = _ints(torch, steps[0])
    dkn, dvn = torch.zeros(B, Hkv, N, d, dtype=torch.float16, device="cuda"), torch.zeros(B, Hkv, N, d, dtype=torch.float16, device="cuda")
    dq = torch.zeros(B, Hq, N, d, dtype=torch.float16, device="cuda")
    need = fa.kvcache_paged_workspace_bytes(B, Hkv, G, N, max_pages, ps, d)
    ws = _nan_workspace(torch, need)

    def step(ck, cv, cl, cq):
        fa.fa_kvcache_append_paged(dkn, dvn, ck, cv, dt, cache_seqlens=cl, seqlens_out=cl, q=cq, rotary_cos=cos, rotary_sin=sin,
                                   seqlens_new=dn)
        return fa.fa_forward_kvcache_paged(cq, ck, cv, dt, cl, causal=True, return_lse=True, workspace=ws, seqlens_q=dn)

    step(dkp.clone(), dvp.clone(), dl.clone(), dq.clone())   # warm-up on scratch state
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(dkp, dvp, dl, dq)
    assert dl.tolist() == lens   # a capture runs nothing
    used = [0] * B               # tokens of the drawn rows each sequence has consumed
    for s, cnt in enumerate(steps):
        newk, newv = np.zeros((B, Hkv, N, d), np.uint16), np.zeros((B, Hkv, N, d), np.uint16)
        newq = np.full((B, Hq, N, d), cm.NAN16, np.uint16)                       # dead Q rows: NaN
        qf = np.zeros((B * Hq, N, d), np.float32)
        for b in range(B):
            for t in range(cnt[b]):
                src = lens[b] + t                                                # the drawn row that becomes key lens[b] + t
                newk[b, :, t], newv[b, :, t] = kb4[b, :, src], vb4[b, :, src]
                kcpu[b * Hkv:(b + 1) * Hkv, src], vcpu[b * Hkv:(b + 1) * Hkv, src] = k[b * Hkv:(b + 1) * Hkv, src], v[b * Hkv:(b + 1) * Hkv, src]
                newq[b, :, t] = qb.reshape(B, Hq, 3 * N, d)[b, :, used[b] + t]
                qf[b * Hq:(b + 1) * Hq, t] = q.reshape(B, Hq, 3 * N, d)[b, :, used[b] + t]
            used[b] += cnt[b]
        dn.copy_(_ints(torch, cnt)), dkn.copy_(cm.dev16(torch, newk, fmt)), dvn.copy_(cm.dev16(torch, newv, fmt)), dq.copy_(cm.dev16(torch, newq, fmt))
        ws.fill_(0xFF), o.fill_(float("nan")), lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        lens = [L + c for L, c in zip(lens, cnt)]
        assert dl.tolist() == lens, s
        want, want_lse = cm.expected_f64(qf, kcpu, vcpu, lens, B, Hkv, G, N, True, nq=cnt)
        live = ri.limits(lens, cnt, B, Hkv, G, N, Ncap, True, 0)[2]
        _check(oracle, o, lse, want, want_lse, live, fmt, f"captured step {s}: counts {cnt}, lengths {lens}")
    assert dl.tolist() == [15, 37, 3]


# ---- 7. the torch ops -----------------------------------------------------------------------------------------------------------------
def test_ragged_ops_are_the_front_ends(fa, oracle, torch_cuda):
    """one call per _ragged op: the bits of the front end it stands for"""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    ops = torch.ops.fa_mi355
    fmt, d, name, W = 1, 128, "spec", 100
    f = ri.FAMILIES[name]
    B, Hkv, G, Nq, Ncap = ri.shape(f)
    (q, k, v), (qb, kb, vb) = ri.inputs(oracle, name, d, fmt)
    dq = cm.dev16(torch, qb, fmt).view(B, Hkv * G, Nq, d)
    dl, dn, ds = _ints(torch, f["lens"]), _ints(torch, f["nq"]), _floats(torch, li.sinks_for(Hkv * G))
    sc = 1.0 / np.sqrt(d)
    kp, vp, table = cm.scatter(kb.reshape(B, Hkv, Ncap, d), vb.reshape(B, Hkv, Ncap, d), f["lens"], 16, 3)
    dk, dv = (cm.dev16(torch, cm.poisoned(x.reshape(B, Hkv, Ncap, d), f["lens"]), fmt) for x in (kb, vb))
    dkp, dvp, dt = cm.dev16(torch, kp, fmt), cm.dev16(torch, vp, fmt), torch.from_numpy(table).cuda()
    z8 = lambda x: torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(-400, 400).to(torch.float8_e4m3fn)
    dk8, dv8, dkp8, dvp8 = z8(dk.float()), z8(dv.float()), z8(dkp.float()), z8(dvp.float())
    s8 = _floats(torch, [0.5, 2.0])
    kw = dict(cache_seqlens=dl, causal=True, scale=sc, window=W, sinks=ds, softcap=li.SOFTCAP, out_dtype=torch.float32, seqlens_q=dn)
    tail = (dl, dn, sc, True, W, ds, li.SOFTCAP, True)
    pairs = (
        (ops.decode_ragged(dq, dk, dv, *tail), fa.fa_forward_kvcache(dq, dk, dv, **kw)),
        (ops.decode_paged_ragged(dq, dkp, dvp, dt, *tail), fa.fa_forward_kvcache_paged(dq, dkp, dvp, dt, **kw)),
        (ops.decode_fp8_ragged(dq, dk8, dv8, s8, s8, *tail), fa.fa_forward_kvcache_fp8(dq, dk8, dv8, s8, s8, **kw)),
        (ops.decode_paged_fp8_ragged(dq, dkp8, dvp8, dt, s8, s8, *tail), fa.fa_forward_kvcache_paged_fp8(dq, dkp8, dvp8, dt, s8, s8, **kw)),
    )
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(pairs):
        assert torch.isfinite(want).all() and torch.equal(got, want), i
    assert not torch.equal(pairs[0][0], fa.fa_forward_kvcache(dq, dk, dv, **dict(kw, seqlens_q=None)))
    # the appends: contiguous and paged, 16 bit and fp8, with the rotary arguments and with None for all three
    Nnew = 3
    new = _ints(torch, [3, 1, 0, 2, 3])
    cos, sin = (_floats(torch, x) for x in rp.scrambled_table(Ncap, d // 2, 11))
    dkn, dvn = dk[:, :, :Nnew].contiguous(), dv[:, :, 7:7 + Nnew].contiguous()
    start = _ints(torch, [10, 20, 30, 317, 319])
    for rot in (True, False):
        for paged, fp8_, opname in ((False, False, "append_ragged"), (True, False, "append_paged_ragged"),
                                    (False, True, "append_fp8_ragged"), (True, True, "append_paged_fp8_ragged")):
            res = []
            for via_op in (True, False):
                ck, cv = (x.clone() for x in ((dkp8, dvp8) if paged and fp8_ else (dkp, dvp) if paged else (dk8, dv8) if fp8_ else (dk, dv)))
                cl, cq = start.clone(), dq[:, :, :Nnew].contiguous()
                mid = ([dt] if paged else []) + ([s8, s8] if fp8_ else [])
                if via_op:
                    getattr(ops, opname)(dkn, dvn, ck, cv, *mid, cl, cl, new, cq if rot else None, cos if rot else None,
                                         sin if rot else None, False)
                else:
                    fn = getattr(fa, "fa_kvcache_append" + ("_paged" if paged else "") + ("_fp8" if fp8_ else ""))
                    rk = dict(q=cq, rotary_cos=cos, rotary_sin=sin) if rot else {}
                    fn(dkn, dvn, ck, cv, *mid, cache_seqlens=cl, seqlens_out=cl, seqlens_new=new, **rk)
                torch.cuda.synchronize()
                u = torch.uint8 if fp8_ else torch.int16
                res.append((ck.view(u), cv.view(u), cl, cq.view(torch.int16)))
            for x, y in zip(*res):
                assert torch.equal(x, y), (opname, rot)
            assert res[0][2].tolist() == [13, 21, 30, 319, 320]
