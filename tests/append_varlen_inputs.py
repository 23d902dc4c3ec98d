"""Inputs and expected bytes for the packed append fa_kvcache_append_varlen (tests/test_gpu_kvcache_append_varlen.py,
tests/test_append_varlen_inputs.py).  Pure numpy; nothing here touches a GPU.

The contract, from include/fa_mi355.h: Knew, Vnew (total_new, Hkv, d) and Q, Qout (total_new, Hkv*G, d) are cut by cu_seqlens_new:
s_b = clamp(cu[b], 0, total_new), e_b = clamp(cu[b+1], s_b, total_new), m_b = e_b - s_b; token row t with s_b <= t < e_b is token
i = t - s_b of sequence b and goes to p = L_b + i by fa_kvcache_append_ex's rules for m_b tokens; Q row t is rotated at p; rows of no
sequence are never used and their Qout rows are not written.  The expectation is COMPOSED from the pieces the other append tiers hold:
the rows are gathered into the padded head-major layout, rotated by rope_inputs, quantised by rope_inputs.fp8_codes and placed by
ragged_inputs.place -- the padded entry's result, which the packed one must equal byte for byte.

The shape.  Hkv 2, G 2; B = 5 with m = (37, 0, 1, 70, 12) behind cu[0] = 3 and 9 tail rows past cu[B]: total_new = 132.  Ncap = 96
with starting lengths (5, 40, 95, 30, 0): sequence 3 overflows (30 + 70 > 96: four tokens dropped), sequence 2 lands on the last row,
sequence 1 is empty between two live ones.  Pages of 16 behind a permuted table with spare pages.  At d = 64 a 256-thread workgroup
spans 32 (token, head) rows, so workgroups cross every sequence boundary.

WRONG names the kernels the CPU tier must tell apart from the right one (model(..., wrong=name) is what each would write).  The last
three concern the rotation or Q and exist in the rotary cases only.
"""
import functools

import numpy as np

import append_inputs as ai
import common_inputs as cm
import ragged_inputs as ri
import rope_inputs as rp

CASE = dict(B=5, Hkv=2, G=2, Ncap=96, ps=16, m=(37, 0, 1, 70, 12), first=3, tail=9, lens=(5, 40, 95, 30, 0), max_pos=80, seed=9100)
QOUT_NAN = 0x7FC1   # what a q_out of its own holds before the call: a NaN in fp16 and bf16 that is not the dead source rows' 0x7FFF
K_SCALE, V_SCALE = np.array([0.5, 1.75], np.float32), np.array([2.0, 0.37], np.float32)

WRONG = ("ignores_cu0", "padded_position", "boundary_to_empty", "rotates_at_i", "writes_dead_qout", "hkv_for_hq")
ROTARY_ONLY = WRONG[3:]

# every form: paged, fp8, rope (0 no rotation, 1 half-split pairs, 2 interleaved pairs)
FORMS = [(p, q, r) for p in (False, True) for q in (False, True) for r in (0, 1, 2)]


def form_id(paged, fp8, rope):
    return ("paged_" if paged else "") + ("fp8_" if fp8 else "") + ("plain", "rope", "rope_il")[rope]


def cu_of(case=CASE):
    """cu_seqlens_new, B + 1 entries"""
    return np.concatenate([[case["first"]], case["first"] + np.cumsum(case["m"])]).astype(np.int32)


def total_of(case=CASE):
    return case["first"] + sum(case["m"]) + case["tail"]


def bounds(cu, total):
    """[(s_b, e_b)]: the clamp of include/fa_mi355.h"""
    out = []
    for b in range(len(cu) - 1):
        s = cm.clamp(cu[b], total)
        out.append((s, min(max(int(cu[b + 1]), s), total)))
    return out


def owned(cu, total):
    """bool [total]: the rows that belong to a sequence"""
    own = np.zeros(total, bool)
    for s, e in bounds(cu, total):
        own[s:e] = True
    return own


def token_rows(cu, total, wrong=None):
    """[rows of sequence b]: the source row of token i of sequence b, for the right kernel or a wrong one"""
    bd = bounds(cu, total)
    if wrong == "ignores_cu0":
        bd[0] = (0, bd[0][1])
    rows = [list(range(s, e)) for s, e in bd]
    if wrong == "padded_position":   # the padded entry's source index, b * Nmax + i, held inside the tensor
        nmax = max(len(r) for r in rows)
        rows = [[min(b * nmax + i, total - 1) for i in range(len(r))] for b, r in enumerate(rows)]
    if wrong == "boundary_to_empty":   # the first row of the sequence behind an empty one goes to the empty one
        for b in range(len(rows) - 1):
            if not rows[b] and rows[b + 1] and bd[b][0] == bd[b + 1][0]:
                rows[b], rows[b + 1] = rows[b + 1][:1], rows[b + 1][1:]
    return rows


def gather(packed, rows, fill=0):
    """packed (total, H, d) -> the padded head-major [B, H, Nmax, d] the padded entry takes; padding holds `fill`"""
    nmax = max(1, max(len(r) for r in rows))
    out = np.full((len(rows), packed.shape[1], nmax, packed.shape[2]), fill, packed.dtype)
    for b, r in enumerate(rows):
        if r:
            out[b, :, :len(r)] = packed[r].transpose(1, 0, 2)
    return out


def make_table(case, cu, total, lens=None):
    """-> (table [B, max_pages] int32, num_pages): pages below the length after the append are the sequence's own, dealt out by a
    seeded permutation of a pool with three spare pages; every other entry holds garbage"""
    B, ps, ncap = len(cu) - 1, case["ps"], case["Ncap"]
    max_pages = ncap // ps
    m = [e - s for s, e in bounds(cu, total)]
    after = ri.lens_after(case["lens"] if lens is None else lens, m, B, max(1, max(m)), ncap)
    num_pages = B * max_pages + 3
    perm = np.random.default_rng(case["seed"]).permutation(num_pages)
    table = np.empty((B, max_pages), np.int32)
    nxt = 0
    for b in range(B):
        for pi in range(max_pages):
            if pi * ps < after[b]:
                table[b, pi] = perm[nxt]
                nxt += 1
            else:
                table[b, pi] = cm.GARBAGE[pi % 2]
    return table, num_pages


@functools.lru_cache(maxsize=None)
def inputs(fmt, d, paged, fp8, rope, split=None):
    """The sources, tables and starting caches of one form, read-only.  Rows of no sequence hold a NaN pattern in K, V and Q; caches
    and pools start as NaN patterns (0x7FFF, fp8: 0x7F); rot_dim = d / 2 and max_pos < Ncap, so the table clamp is on the path.
    split: None (the case's), or (cu, total_new, lens) as tuples: another cut of as many rows, B = len(cu) - 1."""
    c = CASE
    Hkv, G, ncap, ps = c["Hkv"], c["G"], c["Ncap"], c["ps"]
    cu, total, lens = (cu_of(c), total_of(c), c["lens"]) if split is None else (np.array(split[0], np.int32), split[1], tuple(split[2]))
    B = len(cu) - 1
    rng = np.random.default_rng(c["seed"] + 8 * d + fmt)
    own = owned(cu, total)
    if fp8 and not rope:
        knb = ai.fp8_new_rows(1, Hkv, total, d, K_SCALE, fmt, c["seed"] + 1)[0].transpose(1, 0, 2).copy()   # every code, every tie
    elif rope:   # a rotated NaN's payload is not promised, nor is inf - inf: K is rotated from finite rows
        knb = ai.round16_bits(rng.standard_normal((total, Hkv, d)).astype(np.float32), fmt)
    else:
        knb = ai.random_bytes((total, Hkv, d), 2, c["seed"] + 1)   # every pattern, NaN payloads included
    vnb = ai.fp8_new_rows(1, Hkv, total, d, V_SCALE, fmt, c["seed"] + 2)[0].transpose(1, 0, 2).copy() if fp8 \
        else ai.random_bytes((total, Hkv, d), 2, c["seed"] + 2)
    qsrc = ai.round16_bits(rng.standard_normal((total, Hkv * G, d)).astype(np.float32), fmt)
    for x in (knb, vnb, qsrc):
        x[~own] = cm.NAN16
    cos, sin = rp.scrambled_table(c["max_pos"], d // 4, c["seed"])
    table, num_pages = make_table(c, cu, total, lens) if paged else (None, 0)
    shape = (num_pages, Hkv, ps, d) if paged else (B, Hkv, ncap, d)
    cache0 = np.full(shape, 0x7F, np.uint8) if fp8 else np.full(shape, cm.NAN16, np.uint16)
    out = dict(knb=knb, vnb=vnb, qsrc=qsrc, cos=cos, sin=sin, table=table, num_pages=num_pages, kc0=cache0, vc0=cache0.copy(), cu=cu,
               total=total, lens=lens, ks=K_SCALE if fp8 else None, vs=V_SCALE if fp8 else None)
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def model(fmt, d, paged, fp8, rope, wrong=None, qout0=None, x=None):
    """What the call leaves behind -> dict(k, v: the whole cache or pool; lens: seqlens_out; qout: the whole Qout (rotary, else None)).
    qout0: what Qout held before (default: QOUT_NAN everywhere, a buffer of its own); x: other inputs than inputs(...) (another split)."""
    x = x or inputs(fmt, d, paged, fp8, rope)
    ncap, il = CASE["Ncap"], rope == 2
    cu, lens = x["cu"], x["lens"]
    total, cos, sin = x["total"], x["cos"], x["sin"]
    rows = token_rows(cu, total, wrong)
    m = [len(r) for r in rows]
    kpad, vpad = gather(x["knb"], rows), gather(x["vnb"], rows)
    rot_lens = None if wrong == "rotates_at_i" else lens
    if rope:
        krot = rp.rotated_rows_fp32(kpad, fmt, rot_lens, ncap, cos, sin, il)
        krows = rp.fp8_codes(krot, x["ks"]) if fp8 else rp.rotated_rows16(kpad, fmt, rot_lens, ncap, cos, sin, il)
    else:
        krows = rp.fp8_codes(ai.widen16(kpad, fmt), x["ks"]) if fp8 else kpad
    vrows = rp.fp8_codes(ai.widen16(vpad, fmt), x["vs"]) if fp8 else vpad
    out = dict(k=ri.place(x["kc0"], krows, lens, m, x["table"]), v=ri.place(x["vc0"], vrows, lens, m, x["table"]),
               lens=ri.lens_after(lens, m, len(rows), kpad.shape[2], ncap), qout=None)
    if rope:
        qsrc = x["qsrc"]
        qout = np.full(qsrc.shape, QOUT_NAN, np.uint16) if qout0 is None else np.array(qout0)
        qrot = rp.rotated_rows16(gather(qsrc, rows), fmt, rot_lens, ncap, cos, sin, il)
        heads = CASE["Hkv"] if wrong == "hkv_for_hq" else qsrc.shape[1]
        if wrong == "writes_dead_qout":
            dead = ~owned(cu, total)
            qout[dead] = qsrc[dead]
        for b, r in enumerate(rows):
            if r:
                qout[r, :heads] = qrot[b, :heads, :len(r)].transpose(1, 0, 2)
        out["qout"] = qout
    return out
