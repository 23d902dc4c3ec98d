"""Inputs, the float64 reference and the numpy kernels of the fp8 MLA entries fa_mla_decode_fp8 and fa_mla_append_fp8
(tests/test_gpu_mla_fp8.py, tests/test_mla_fp8_inputs.py).  Pure numpy plus the `oracle` fixture; nothing here touches a GPU.

The families, the packing, the check and the bounds are tests/mla_inputs.py's; the e4m3fn format is tests/fp8_inputs.py's.  A family's
cache is held as CODES: codes = encode(c / C_SCALE) with C_SCALE = float32(12 / 448), so the boosted key element (BOOST_K = 12, column
512) lands on the top code 0x7E and the N(0,1) elements lie far inside the range.  The float64 reference is mla_inputs.expected_f64 on
decode(codes) * C_SCALE: the device widens the codes exactly, so the fp8 cache adds no error the reference does not already contain and
the bounds are the 16-bit tier's, unchanged.
"""
import functools

import numpy as np

import common_inputs as cm
import decode_varlen_inputs as dv
import fp8_inputs as f8
import mla_inputs as mi

C_SCALE = np.float32(12.0 / 448.0)
NAN_CODE = f8.NAN_CODES[0]
ROW = mi.DQK   # bytes per cache row


@functools.lru_cache(maxsize=None)
def codes(oracle, name, fmt):
    """-> the family's cache [B, Ncap, 576] as uint8 e4m3fn codes of c / C_SCALE, read-only"""
    (_, c), _ = mi.inputs(oracle, name, fmt)
    out = f8.encode(c.astype(np.float32) / C_SCALE)
    f = mi.family(name)
    for b in range(f["B"]):   # the boosted element sits on the top code
        L = cm.clamp(f["lens"][b], f["Ncap"])
        assert (out[b, max(0, L - f["max_q"]):L, mi.DC] == 0x7E).all()
    out.setflags(write=False)
    return out


def values(code_array, c_scale=C_SCALE):
    """codes -> the float64 element values decode(code) * c_scale"""
    return f8.decode(code_array).astype(np.float64) * np.float64(c_scale)


@functools.lru_cache(maxsize=None)
def reference(oracle, name, fmt, causal):
    """mla_inputs.expected_f64 on the decoded cache (padded [B*Hq, max_q, ...]), computed once and read-only"""
    f, lay = mi.family(name), mi.layout(name)
    (q, _), _ = mi.inputs(oracle, name, fmt)
    out, lse = mi.expected_f64(q, values(codes(oracle, name, fmt)), f["lens"], lay.n, f["max_q"], f["Hq"], causal)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def poisoned_cache(oracle, name, fmt):
    """the family's codes [B, Ncap, 576] with the NaN code in every row at or past the clamped length"""
    return cm.poisoned(codes(oracle, name, fmt)[:, None], mi.family(name)["lens"], nan=NAN_CODE)[:, 0]


def paged_cache(oracle, name, fmt, ps, seed=5):
    """-> (pool [num_pages, ps, 576] uint8, table [B, max_pages] int32) by common_inputs.scatter: a shuffled table, garbage in the
    entries past the last live page, the NaN code in every pool row no key lies in"""
    cb = codes(oracle, name, fmt)[:, None]
    pool, _, table = cm.scatter(cb, cb, mi.family(name)["lens"], ps, seed, nan=NAN_CODE)
    return np.ascontiguousarray(pool[:, 0]), table


# ---- numpy kernels: the right one and the wrong ones the check must reject -----------------------------------------------------------
# wrong rule -> a family on which the check rejects it (tests/test_mla_fp8_inputs.py asserts each)
WRONG = {
    "scale_on_logits_only": "h16",    # 1. O is left in code units: 448 / 12 times too large
    "scale_on_o_only": "h16",         # 2. the logits are left in code units: a far too peaked softmax
    "scale_squared_on_logits": "h5",  # 3. c_scale twice on the logits: nearly uniform weights, the boost is lost
    "scale_on_512_only": "h48",       # 4. the rotary 64's share of the logit is left in code units
    "row_stride_1152": "h16",         # 5. the 16-bit row stride on byte rows: row p reads the bytes of row 2p
    "half_row_widened": "h128",       # 6. the first 288 bytes of a row are widened, the rest is zero
    "decoded_as_e5m2": "h5",          # 7. the codes are read as e5m2
    "pair_swapped": "h1",             # 8. the high and the low code of each widened pair change places
    "v_from_code_64": "h48",          # 9. V is taken from codes 64 .. 575
    "nan_code_as_448": "h5",          # 10. the split's end is rounded up to the 32-key tile, and the NaN code there reads as 448
}

E5M2 = np.array([(-1.0 if c & 0x80 else 1.0) * ((c & 3) / 4.0 * 2.0 ** -14 if (c >> 2) & 31 == 0 else (1.0 + (c & 3) / 4.0) * 2.0 ** (((c >> 2) & 31) - 15))
                 for c in range(256)], np.float64)   # exponent 31 (inf / NaN in e5m2) read as an ordinary binade: the result stays finite


def numpy_kernel(oracle, name, fmt, causal=True, wrong=None, S=2):
    """What a kernel would leave in pre-filled fp32 O [total_q, Hq, 512] and lse [Hq, total_q] on the family's POISONED codes: float64
    arithmetic rounded to fp32, with one of the WRONG rules in the place of the right one (None: the entry as specified, merged from S
    key splits)."""
    f, lay = mi.family(name), mi.layout(name)
    B, Hq, Nq, Ncap = f["B"], f["Hq"], f["max_q"], f["Ncap"]
    (q, _), _ = mi.inputs(oracle, name, fmt)
    cb = poisoned_cache(oracle, name, fmt)
    cs = np.float64(C_SCALE)
    o = np.zeros((B * Hq, Nq, mi.DC), np.float64)
    lse = np.full((B * Hq, Nq), -np.inf, np.float64)
    for b in range(B):
        n = lay.n[b]
        L = cm.clamp(f["lens"][b], Ncap)
        end = min(-(-L // 32) * 32, Ncap) if wrong == "nan_code_as_448" else L   # the rows that reach the arithmetic
        rows = cb[b, :end]
        if wrong == "row_stride_1152":
            flat = np.concatenate([cb[b].reshape(-1), np.zeros(Ncap * ROW, np.uint8)])
            rows = np.stack([flat[2 * p * ROW:2 * p * ROW + ROW] for p in range(end)]) if end else rows
            rows = np.where(np.isin(rows, f8.NAN_CODES), 0, rows).astype(np.uint8)   # a dead row's bytes: outside the descriptor
        if wrong == "pair_swapped":
            rows = rows.reshape(end, ROW // 2, 2)[:, :, ::-1].reshape(end, ROW)
        if wrong == "decoded_as_e5m2":
            code_vals = E5M2[rows]
        elif wrong == "nan_code_as_448":
            code_vals = np.where(np.isin(rows, f8.NAN_CODES), 448.0, f8.decode(np.where(np.isin(rows, f8.NAN_CODES), 0, rows))).astype(np.float64)
        else:
            code_vals = f8.decode(rows).astype(np.float64)
        assert np.isfinite(code_vals).all(), "a NaN code reached the arithmetic"
        if wrong == "half_row_widened":
            code_vals = code_vals.copy()
            code_vals[:, ROW // 2:] = 0.0
        for p in range(n * Hq):
            i, h = divmod(p, Hq)
            qq = q[b * Hq + h, i].astype(np.float64)
            lim = max(0, L - n + 1 + i) if causal else end
            if lim == 0:
                continue
            kk = code_vals[:lim]
            if wrong == "scale_on_o_only":
                s = (kk @ qq) * mi.SCALE
            elif wrong == "scale_squared_on_logits":
                s = (kk @ qq) * mi.SCALE * cs * cs
            elif wrong == "scale_on_512_only":
                s = ((kk[:, :mi.DC] @ qq[:mi.DC]) * cs + kk[:, mi.DC:] @ qq[mi.DC:]) * mi.SCALE
            else:
                s = (kk @ qq) * mi.SCALE * cs
            vv = kk[:, mi.DR:] if wrong == "v_from_code_64" else kk[:, :mi.DC]
            # S splits of the 64-key tiles, merged as the kernel merges them; c_scale joins 1 / l
            per = -(-(-(-lim // 64)) // S) * 64
            parts = [(s[a:a + per], vv[a:a + per]) for a in range(0, lim, per)]
            ms = [x.max() for x, _ in parts]
            M = max(ms)
            den = sum(np.exp(m - M) * np.exp(x - m).sum() for (x, _), m in zip(parts, ms))
            num = sum(np.exp(m - M) * (np.exp(x - m) @ v) for (x, v), m in zip(parts, ms))
            o[b * Hq + h, i] = num / den * (1.0 if wrong == "scale_on_logits_only" else cs)
            lse[b * Hq + h, i] = M + np.log(den)
    po = dv.pack_rows(lay, o.astype(np.float32), 0.0)
    po[~lay.owned] = np.array([dv.SENTINEL_O32], np.uint32).view(np.float32)[0]
    pl = dv.pack_lse(lay, lse.astype(np.float32), np.float32(dv.SENTINEL_LSE))
    return po, pl


# ---- the wide-logit-range inputs of tests/softmax_range_inputs.py on an fp8 cache ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_case(fmt):
    """softmax_range_inputs.mla_case(fmt) with its cache quantised: c_scale = amax / 448 makes the hostile rotary values (the largest
    elements by far) representable.  -> dict(q, codes [B, Ncap, 576] uint8, c_scale float32, c: the float64 values the codes stand for)"""
    import softmax_range_inputs as sr
    case = sr.mla_case(fmt)
    c_scale = np.float32(np.abs(case["c"]).max() / np.float32(448.0))
    cb = f8.encode(case["c"].astype(np.float32) / c_scale)
    c = values(cb, c_scale)
    for a in (cb, c):
        a.setflags(write=False)
    return dict(q=case["q"], qbits=case["bits"][0], codes=cb, c_scale=c_scale, c=c)


@functools.lru_cache(maxsize=None)
def range_reference(fmt, causal):
    """float64 on the decoded codes"""
    import softmax_range_inputs as sr
    case = range_case(fmt)
    out, lse = mi.expected_f64(case["q"], case["c"], sr.MLA["lens"], sr.mla_layout().n, sr.MLA["max_q"], sr.MLA["Hq"], causal)
    out.setflags(write=False), lse.setflags(write=False)
    return out, lse


def range_events(fmt, causal, S):
    """{(b, token, head): rises of the row's tiles, split after split} of the scheme's model (softmax_range_inputs.mla_model) on the
    decoded codes"""
    import softmax_range_inputs as sr
    case = range_case(fmt)
    ev = {}
    sr.mla_model(case["q"], case["c"].astype(np.float32), sr.MLA["lens"], sr.mla_layout(), sr.MLA["Hq"], fmt, causal, S, None, ev)
    return ev
