"""Seeded inputs for tests/test_gpu_kvcache_merge.py -- fa_merge_states (the merge of attention states over disjoint key ranges) and
fa_forward_kvcache_shared_prefix (prefix decode with the batch folded into rows, suffix decode, merge) -- with the rule and the
composed call restated in float64 numpy, the derived error bound of the fp32 merge, and the helpers that show no parity launch could
pass on a wrong merge (tests/test_merge_inputs.py asserts them without a GPU).  Pure numpy plus the `oracle` fixture
(tests/conftest.py); nothing here touches a GPU.

The rule, for R parts (O_r, lse_r) over disjoint key ranges:   lse = ln sum_r exp(lse_r),   O = sum_r O_r exp(lse_r - lse).
A part with lse_r = -inf is neutral whatever its O row holds; all parts -inf: O = 0, lse = -inf.
A part is addressed by rows: row (b, h, r) is x = b * stride_b + h * stride_h + r of a flat [X, d] array (include/fa_mi355.h).

The composed call: sequence b holds the prefix keys [0, P) and then its own [0, L_b); row i of the sequence sees the WHOLE prefix and
the suffix keys [0, c_i), c_i = L_b without the causal mask and max(0, L_b - Nq + 1 + i) with it.  The reference is
common_inputs.expected_f64 (W = 0) on the concatenated keys, lengths P + c_i.  It is taken row by row, with the row's own length and no
mask: for L_b >= Nq that is exactly expected_f64 with causal on lengths P + L_b, and for L_b < Nq (rows that see no suffix key at
all) it keeps the whole prefix visible, as the entry defines it, where a mask aligned to the end of P + L_b keys would cut into the
prefix.
"""
import functools

import numpy as np

import census_inputs as ci
import common_inputs as cm
import decode_inputs as di
import fp8_inputs as f8
import logit_inputs as li

U = 2.0 ** -24                       # unit roundoff of fp32
OUT_EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}   # half an ulp of the output format, relative
STATE_DTYPES = ("f16", "bf16", "f32")
SPREAD = 40.0                        # the merge parity draws its parts with |lse_r - M| <= SPREAD
NEAR = 2.0                           # ... and half of them within NEAR of the row's maximum


# ---- the rule in float64 ------------------------------------------------------------------------------------------------------------
def rows_of(stride_b, stride_h, B, H, rows):
    """[B, H, rows] int64: the row index x of every (b, h, r) of a part"""
    b, h, r = np.meshgrid(np.arange(B), np.arange(H), np.arange(rows), indexing="ij")
    return b * stride_b + h * stride_h + r


def merge_f64(parts, B, H, rows, log2=False):
    """parts: a list of (O [X, d], lse [X], stride_b, stride_h), any float arrays -> (O [B, H, rows, d], lse [B, H, rows]) float64 by
    the rule.  A part's O row is READ only where its lse is finite.  log2=True is a WRONG merge: it takes lse for log2 units."""
    d = parts[0][0].shape[-1]
    lses = np.stack([np.asarray(l, np.float64).reshape(-1)[rows_of(sb, sh, B, H, rows)] for (_, l, sb, sh) in parts])   # [R,B,H,rows]
    M = lses.max(0)
    out = np.zeros((B, H, rows, d), np.float64)
    L = np.zeros((B, H, rows), np.float64)
    for (o, _, sb, sh), l in zip(parts, lses):
        live = np.isfinite(l)
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.where(live, (np.exp2 if log2 else np.exp)(np.where(live, l - M, 0.0)), 0.0)
        x = rows_of(sb, sh, B, H, rows)
        out[live] += w[live][:, None] * np.asarray(o, np.float64).reshape(-1, d)[x[live]]
        L += w
    some = L > 0
    out[some] /= L[some][:, None]
    with np.errstate(divide="ignore"):
        lse = np.where(some, M + (np.log2 if log2 else np.log)(np.where(some, L, 1.0)), -np.inf)
    return out, lse


# ---- the derived bound of the fp32 merge ---------------------------------------------------------------------------------------------
def f32_bound(R, vmax):
    """What the kernel may be off by on fp32 parts with fp32 output, against the float64 rule on the same parts, when every
    |lse_r - M| <= SPREAD.  Derived from what the kernel does (csrc/fa_merge_states.hip), u = 2^-24:
      weights   w_r = exp2(fl(fl(lse_r - M) * fl(log2 e))) with t_r = |lse_r - M|: the subtraction, the product and the constant are
                each off by a relative u, so the exponent is off by at most 3 u t_r (natural-log units), and the hardware exponential
                by one ulp, 2 u: w_r carries a relative error of at most 3 u t_r + 2 u.  The part with t_r = 0 has w_r = 1 exactly.
                What reaches the result is that error times the weight e^(-t_r): (3 u t_r + 2 u) e^(-t_r) <= (3 / e + 2) u < 3.11 u
                for ANY t_r (t e^-t <= 1 / e), which is why the restriction on the spread only has to keep w_r a normal number.
      sums      the numerator sum_r w_r O_r is R fused multiply-adds, the denominator L = sum_r w_r is R adds (a tree, which is no
                worse): each is off by at most R u times the sum of the magnitudes, and sum_r w_r |O_r| <= L max|O|.
      division  correctly rounded: u.
    With L >= 1 and |O| <= max|O|, numerator and denominator each contribute 3.11 (R - 1) u + R u, so
      |O_kernel - O| <= max|O| * u * (2 * (3.11 (R - 1) + R) + 1), times 1.05 for the second-order terms."""
    return 1.05 * vmax * U * (2.0 * (3.11 * (R - 1) + R) + 1.0)


def lse_bound(R, lse_abs_max):
    """The same for lse = M + log2(L) * ln 2: L carries the relative error (3.11 (R - 1) + R) u, the hardware logarithm one ulp of a
    value of at most log2(R), the product with fl(ln 2) two roundings, and the final sum one rounding of |lse|."""
    return 1.05 * U * (3.11 * (R - 1) + R + 4.0 * np.log2(max(R, 2)) + abs(lse_abs_max))


def out_bound(R, vmax, want, out_dtype):
    """f32_bound plus the ONE rounding to a 16-bit output: half an ulp of the output format at the value (fp16 results below the
    normal range are spaced 2^-24)"""
    b = f32_bound(R, vmax) + OUT_EPS[out_dtype] * np.abs(want)
    return b + (2.0 ** -25 if out_dtype == "f16" else 0.0)


# ---- the parts of the merge parity ----------------------------------------------------------------------------------------------------
MERGE_SHAPE = dict(B=2, H=2, rows=6)
MERGE_R = (1, 2, 3, 16)
LAYOUTS = ("contiguous", "hb", "padded")


def layout(name, B, H, rows):
    """-> (stride_b, stride_h, X): [B,H,rows] as a decode entry returns it; [H,B,rows] as the batch-folded prefix decode returns it;
    padded strides that leave gaps between heads and between batch entries"""
    if name == "contiguous":
        return H * rows, rows, B * H * rows
    if name == "hb":
        return rows, B * rows, B * H * rows
    assert name == "padded"
    sh = rows + 3
    sb = H * sh + 5
    return sb, sh, B * sb


def round_to(x, dtype, oracle):
    """fp32 values -> the fp32 values of their rounding to a state dtype"""
    x = np.asarray(x, np.float32)
    if dtype == "f32":
        return x
    fmt = 0 if dtype == "f16" else 1
    return oracle.decode16(oracle.encode16(x, fmt), fmt)


@functools.lru_cache(maxsize=None)
def merge_parts(oracle, R, d, dtype, lay, seed=9100):
    """R parts in one layout: O in [-4, 4) rounded to `dtype`, lse = a row base in [-30, 30) plus an offset in [-SPREAD, 0]: one part
    of every row at offset 0, half of the others within NEAR of it (weights that matter: a merge that is wrong shows) and half anywhere
    down to -SPREAD, and with R > 2 one part of every row at -SPREAD itself.  Rows the layout does not name hold NaN in O and in lse.
    -> tuple of (O [X, d] fp32, lse [X] fp32, stride_b, stride_h), read-only"""
    B, H, rows = (MERGE_SHAPE[k] for k in ("B", "H", "rows"))
    sb, sh, X = layout(lay, B, H, rows)
    rng = np.random.default_rng(seed + 31 * R + d + 7 * LAYOUTS.index(lay) + STATE_DTYPES.index(dtype))
    x = rows_of(sb, sh, B, H, rows)
    base = rng.uniform(-30.0, 30.0, (B, H, rows))
    near = rng.integers(0, 2, (R, B, H, rows)) == 1
    off = -np.where(near, rng.uniform(0.0, NEAR, (R, B, H, rows)), rng.uniform(0.0, SPREAD, (R, B, H, rows)))
    top = rng.integers(0, R, (B, H, rows))
    np.put_along_axis(off, top[None], 0.0, 0)
    if R > 2:
        np.put_along_axis(off, ((top + 1) % R)[None], -SPREAD, 0)
    parts = []
    for r in range(R):
        o = np.full((X, d), np.nan, np.float32)
        l = np.full(X, np.nan, np.float32)
        o[x] = round_to(rng.uniform(-4.0, 4.0, (B, H, rows, d)), dtype, oracle)
        l[x] = (base + off[r]).astype(np.float32)
        o.setflags(write=False), l.setflags(write=False)
        parts.append((o, l, sb, sh))
    lses = np.stack([p[1][x] for p in parts]).astype(np.float64)
    assert (lses.max(0) - lses.min(0) <= SPREAD + 1e-4).all()
    return tuple(parts)


# ---- the composed call ----------------------------------------------------------------------------------------------------------------
SHAPE = dict(B=3, Hkv=2, G=4, Pcap=200, P=130, Ncap=192, lens=(0, 1, 150), page=16, seed=9300)
LONG = dict(B=3, Hkv=2, G=4, Pcap=576, P=530, Ncap=192, lens=(0, 1, 150), page=16, seed=9400)   # the prefix decode splits (S = 2)
NQS = (1, 3)
VARIANTS = ("none",) + li.VARIANTS
K_MULT, V_MULT = (1.0, 6.0), (6.0, 1.0)   # fp8: per-head scales 6x apart, in opposite order for K and V


def suffix_limits(lens, Nq, Ncap, causal):
    """[B][Nq]: c_i, the suffix keys row i of sequence b sees"""
    return [cm.row_limits(cm.clamp(L, Ncap), Nq, Nq, causal)[1].tolist() for L in lens]


@functools.lru_cache(maxsize=None)
def inputs(oracle, shape_name, Nq, d, fmt, fp8=False):
    """q [B*Hq, Nq, d], prefix k, v [Hkv, Pcap, d], suffix k, v [B*Hkv, Ncap, d]: fp32 values (16-bit-rounded; with fp8 the K and V
    values are the dequantised codes) and what the device gets: 16-bit encodings, or with fp8 uint8 codes and the two scale vectors"""
    c = SHAPE if shape_name == "base" else LONG
    B, Hkv, G, Pcap, Ncap = (c[k] for k in ("B", "Hkv", "G", "Pcap", "Ncap"))
    (q, ks, vs), (qb, ksb, vsb) = di.inputs(oracle, B, Hkv, G, Nq, Ncap, d, fmt, c["seed"] + d + fmt)
    (_, kp, vp), (_, kpb, vpb) = di.inputs(oracle, 1, Hkv, 1, 1, Pcap, d, fmt, c["seed"] + 50 + d + fmt)
    out = dict(q=q, qb=qb, kp=kp, vp=vp, ks=ks, vs=vs, bits=(kpb, vpb, ksb, vsb), k_scale=None, v_scale=None)
    if fp8:
        vals, codes, scales = [], [], []
        for pre, suf, mult in ((kp, ks, K_MULT), (vp, vs, V_MULT)):
            amax = np.maximum(np.abs(pre).max((1, 2)), np.abs(suf.reshape(B, Hkv, Ncap, d)).max((0, 2, 3)))
            s = (amax / f8.MAX * np.array([mult[h % 2] for h in range(Hkv)])).astype(np.float32)
            scales.append(s)
            for x, sx in ((pre, s), (suf, np.tile(s, B))):
                code = f8.encode((x / sx[:, None, None]).astype(np.float32))
                assert not np.isin(code, f8.NAN_CODES).any()
                codes.append(code)
                vals.append((f8.decode(code) * sx[:, None, None]).astype(np.float32))
        out.update(kp=vals[0], ks=vals[1], vp=vals[2], vs=vals[3], bits=(codes[0], codes[2], codes[1], codes[3]),
                   k_scale=scales[0], v_scale=scales[1])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    for a in out["bits"]:
        a.setflags(write=False)
    return out


def vmax_of(x):
    return float(max(np.abs(x["vp"]).max(), np.abs(x["vs"]).max()))


def concatenated(x, c):
    """-> k, v [B*Hkv, P + Ncap, d]: the P live prefix keys of the K/V head followed by the sequence's own cache"""
    B, Hkv, P = c["B"], c["Hkv"], c["P"]
    return tuple(np.concatenate([np.tile(pre[:, :P], (B, 1, 1)), suf], axis=1) for pre, suf in ((x["kp"], x["ks"]), (x["vp"], x["vs"])))


@functools.lru_cache(maxsize=None)
def reference(oracle, shape_name, Nq, d, fmt, causal, variant, fp8=False):
    """(O [B*Hq, Nq, d], lse [B*Hq, Nq]) float64: common_inputs.expected_f64, W = 0, on the concatenated keys, row by row with the
    lengths P + c_i (see the module docstring)"""
    c = SHAPE if shape_name == "base" else LONG
    B, Hkv, G, P, Ncap = (c[k] for k in ("B", "Hkv", "G", "P", "Ncap"))
    x = inputs(oracle, shape_name, Nq, d, fmt, fp8)
    k, v = concatenated(x, c)
    sinks, softcap = li.options(variant, Hkv * G)
    lim = suffix_limits(c["lens"], Nq, Ncap, causal)
    out = np.zeros(x["q"].shape, np.float64)
    lse = np.zeros(x["q"].shape[:2], np.float64)
    for i in range(Nq):
        o1, l1 = cm.expected_f64(np.ascontiguousarray(x["q"][:, i:i + 1]), k, v, [P + lim[b][i] for b in range(B)], B, Hkv, G, 1, False,
                                 0, softcap=softcap, sinks=sinks)
        out[:, i], lse[:, i] = o1[:, 0], l1[:, 0]
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def folded_q(q, B, Hkv, G):
    """q [B*Hkv*G, Nq, d] -> [Hkv*B*G, Nq, d]: the permute of the front end, the batch folded into the rows of a K/V head"""
    Nq, d = q.shape[1:]
    return np.ascontiguousarray(q.reshape(B, Hkv, G, Nq, d).transpose(1, 0, 2, 3, 4)).reshape(Hkv * B * G, Nq, d)


@functools.lru_cache(maxsize=None)
def parts_f64(oracle, shape_name, Nq, d, fmt, causal, variant, fp8=False):
    """The two states of the composed call in float64, as the two decodes return them: the prefix part from the folded q (B = 1,
    G' = B*G, no mask, no sinks) laid out [Hkv, B, G*Nq], the suffix part (the caller's causal flag and sinks) laid out
    [B, Hkv, G*Nq].  -> ((O_p [X, d], lse_p [X], stride_b, stride_h), (O_s, lse_s, stride_b, stride_h))"""
    c = SHAPE if shape_name == "base" else LONG
    B, Hkv, G, P, Ncap = (c[k] for k in ("B", "Hkv", "G", "P", "Ncap"))
    x = inputs(oracle, shape_name, Nq, d, fmt, fp8)
    sinks, softcap = li.options(variant, Hkv * G)
    rows = G * Nq
    o_p, l_p = cm.expected_f64(folded_q(x["q"], B, Hkv, G), x["kp"], x["vp"], [P], 1, Hkv, B * G, Nq, False, 0, softcap=softcap)
    o_s, l_s = cm.expected_f64(x["q"], x["ks"], x["vs"], c["lens"], B, Hkv, G, Nq, causal, 0, softcap=softcap, sinks=sinks)
    return ((o_p.reshape(-1, d), l_p.reshape(-1), rows, B * rows), (o_s.reshape(-1, d), l_s.reshape(-1), Hkv * rows, rows))


CASES = [(Nq, causal, variant) for Nq in NQS for causal in (False, True) for variant in VARIANTS]


def misses(oracle, got, got_lse, want, want_lse, fmt, vmax):
    """True when (got, got_lse) fails a bound the GPU parity test applies: cm.peaked_tol(fmt, vmax, kernels=2) on max |O - want|,
    cm.REL_L2 on the relative L2 error, 2 * cm.P_EPS absolute on lse over the rows that see a key (or a sink), -inf elsewhere"""
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    got_lse = np.asarray(got_lse, np.float64).reshape(want_lse.shape)
    live = np.isfinite(want_lse)
    if not np.isfinite(got).all() or np.isnan(got_lse).any() or (np.isfinite(got_lse) != live).any():
        return True
    rl = float(np.sqrt(((got - want) ** 2).sum() / (want ** 2).sum()))
    return bool(np.abs(got - want).max() > cm.peaked_tol(fmt, vmax, kernels=2) or rl > cm.REL_L2[fmt]
                or np.abs(got_lse[live] - want_lse[live]).max() > 2 * cm.P_EPS[fmt])


WRONG = ("drops the prefix", "drops the suffix", "prefix twice", "lse as log2", "strides ignored")


def wrong_merge(kind, parts, B, Hkv, rows):
    """a float64 merge of the composed call's two parts with one mistake -> (O [B, Hkv, rows, d], lse)"""
    pre, suf = parts
    if kind == "drops the prefix":
        return merge_f64([suf], B, Hkv, rows)
    if kind == "drops the suffix":
        return merge_f64([pre], B, Hkv, rows)
    if kind == "prefix twice":
        return merge_f64([pre, pre, suf], B, Hkv, rows)
    if kind == "lse as log2":
        return merge_f64([pre, suf], B, Hkv, rows, log2=True)
    assert kind == "strides ignored"
    return merge_f64([(pre[0], pre[1], Hkv * rows, rows), suf], B, Hkv, rows)


# ---- the census ---------------------------------------------------------------------------------------------------------------------
def census_case(oracle, Nq, d, fmt, causal):
    """Family Z of tests/census_inputs.py on the composed call: K = 0 in prefix and suffix, V in the residue coding -- the suffix
    with m per (sequence, K/V head), the prefix with m per K/V head -- so O * cnt is the integer sum over the P prefix keys and the
    c_i suffix keys a row sees.  -> dict q, prefix and suffix encodings, S [B*Hq, Nq, d], cnt [B*Hq, Nq]"""
    c = SHAPE
    B, Hkv, G, Pcap, P, Ncap = (c[k] for k in ("B", "Hkv", "G", "Pcap", "P", "Ncap"))
    zs = ci.z_decode(oracle, B, Hkv, G, Nq, Ncap, d, fmt, "residue")
    zp = ci.z_decode(oracle, 1, Hkv, 1, 1, Pcap, d, fmt, "residue")
    lo, lim = ci.decode_limits(c["lens"], B, Hkv, G, Nq, Ncap, causal)
    S_s, _ = ci.decode_sums(zs["m"], lo, lim, G, Ncap, d, "residue")
    m_p = np.tile(np.repeat(zp["m"], G), B)                       # per query head: the prefix value of its K/V head
    S_p = ci.expected_sums(m_p, np.zeros_like(lim), np.full_like(lim, P), Pcap, d, "residue")
    assert (lim - lo == 0).any() or not causal                    # a causal row that sees no suffix key is included
    return dict(qb=zs["bits"][0], prefix=zp["bits"][1:], suffix=zs["bits"][1:], S=S_s + S_p, cnt=(lim - lo) + P,
                v=(zp["v"], zs["v"]), q=zs["q"])
