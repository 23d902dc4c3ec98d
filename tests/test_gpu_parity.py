"""GPU tier: the HIP path, called through the C ABI (libfa_mi355.so), against the CPU oracle on
identical seeded inputs and against the committed golden vectors.

Tolerance (BASELINE.json north_star): max-abs <= 1e-2 vs the naive fp32 CPU reference on the
same fp16/bf16-rounded Q/K/V.  Tighter per-dtype bounds on the relative L2 error the reference
prints (flashattn_streaming_16x16_mw.cu:383-391) are asserted as well.
"""
import glob
import os

import numpy as np
import pytest

import common_inputs as cm

pytestmark = pytest.mark.gpu

# The bounds of the docstring above -- MAX_ABS, REL_L2, P_EPS and peaked_tol -- are defined in tests/common_inputs.py, for every GPU tier.

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _tdtype(torch, fmt):
    return torch.float16 if fmt == 0 else torch.bfloat16


def _to_dev(torch, bits, fmt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(_tdtype(torch, fmt))


def _run(fa, torch, qb, kb, vb, fmt, algo=0, out_same=False, scale=None):
    q, k, v = (_to_dev(torch, x, fmt) for x in (qb, kb, vb))
    od = _tdtype(torch, fmt) if out_same else torch.float32
    o = fa.fa_forward(q, k, v, scale=scale, out_dtype=od, algo=algo)
    torch.cuda.synchronize()
    return o.float().cpu().numpy()


_EXPERIMENTAL = (21, 22, 25)   # A/B kernels: only in libfa_mi355_exp.so (FA_MI355_LIB=...)


def _have_exp():
    import flashattention_kernel_project_amd as fa_
    return fa_.lib().fa_mi355_has_experiments() == 1


def _present(algos):
    """The ids of `algos` the loaded library carries."""
    return tuple(a for a in algos if a not in _EXPERIMENTAL or _have_exp())


def _algos_for(d):
    return _present((0, 1, 2, 5, 6, 21, 22, 23, 24, 25, 26, 27, 29) if d == 64
                    else ((0, 1, 2, 21, 23, 24, 26, 28) if d == 128 else (0, 1)))


def _check(oracle, got, want, fmt, what, out_same=False, max_abs=cm.MAX_ABS, rel_l2=None):
    ma = oracle.max_abs(got, want)
    rl = oracle.rel_l2(got, want)
    assert np.isfinite(got).all(), what
    tol_rl = rel_l2 if rel_l2 is not None else cm.REL_L2[fmt] * (1.5 if out_same else 1.0)
    assert ma <= max_abs and rl <= tol_rl, f"{what}: max_abs={ma:.3e} rel_l2={rl:.3e}"


def test_golden_general(fa, oracle, torch_cuda, golden_dir):
    paths = sorted(p for p in glob.glob(os.path.join(golden_dir, "*.npz"))
                   if not os.path.basename(p).startswith("s16_"))
    assert paths
    for path in paths:
        z = np.load(path)
        fmt = int(z["fmt"])
        d = z["q"].shape[-1]
        for algo in _algos_for(d):
            for out_same in (False, True):
                got = _run(fa, torch_cuda, z["q"], z["k"], z["v"], fmt, algo, out_same)
                _check(oracle, got, z["expected"], fmt, f"{os.path.basename(path)} algo={algo} out_same={out_same}", out_same)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_shape_sweep_vs_oracle(fa, oracle, torch_cuda, fmt, d):
    ns = [1, 15, 16, 17, 63, 64, 65, 127, 255, 256, 257, 513]
    for i, n in enumerate(ns):
        bh = 3 if n < 300 else 2
        (q, k, v), (qb, kb, vb) = oracle.make_qkv(bh, n, d, fmt, seed=1000 + 13 * i + d)
        want = oracle.forward(q, k, v, accum=0, nthreads=8)
        for algo in _algos_for(d):
            got = _run(fa, torch_cuda, qb, kb, vb, fmt, algo)
            _check(oracle, got, want, fmt, f"n={n} d={d} fmt={fmt} algo={algo}")


def test_reference_wmma_entry_point(fa, oracle, torch_cuda):
    """(Q,K,V,O,BH,N,D,scale) exactly as flashattn_forward_wmma_kernel takes them, with the
    reference driver's deterministic fill (flashattn_forward_wmma.cu:368-373)."""
    torch = torch_cuda
    bh, n, d = 1, 128, 64
    i = np.arange(bh * n * d, dtype=np.int64)
    base = (i % 13).astype(np.float32) * np.float32(0.01)
    qb = oracle.encode16(base, 0).reshape(bh, n, d)
    kb = oracle.encode16(np.float32(0.5) * base, 0).reshape(bh, n, d)
    vb = oracle.encode16(np.float32(0.3) * base, 0).reshape(bh, n, d)
    Q, K, V = (_to_dev(torch, x, 0) for x in (qb, kb, vb))
    O = torch.full((bh, n, d), float("nan"), dtype=torch.float32, device="cuda")  # must be fully overwritten
    scale = 1.0 / np.sqrt(np.float32(d))
    fa.flashattn_forward_wmma(Q, K, V, O, bh, n, d, scale)
    torch.cuda.synchronize()
    want = oracle.forward(*(oracle.decode16(x, 0) for x in (qb, kb, vb)), scale=scale)
    _check(oracle, O.cpu().numpy(), want, 0, "wmma driver fill")


def test_scale_argument_and_stream(fa, oracle, torch_cuda):
    torch = torch_cuda
    (q, k, v), (qb, kb, vb) = oracle.make_qkv(2, 200, 64, 0, seed=77)
    want = oracle.forward(q, k, v, scale=0.3, nthreads=4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _run(fa, torch, qb, kb, vb, 0, scale=0.3)
    _check(oracle, got, want, 0, "scale=0.3 on a side stream")


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_forced_rescale_branch(fa, oracle, torch_cuda, fmt, d):
    """The lazy running-max update is a rare, data-dependent branch: force it.  Selected key rows
    in later tiles are made (anti-)parallel to selected query rows so the row max jumps by far
    more than the 2^8 threshold at chosen tiles -- upward several times, for some rows only, and
    for some rows in one half of the tile only."""
    n, bh = 448, 2
    (q, k, v), _ = oracle.make_qkv(bh, n, d, fmt, seed=4242 + d)
    rng = np.random.default_rng(5)
    big = 6.0
    for b in range(bh):
        for qi in rng.choice(n, 40, replace=False):
            for step, key in enumerate(sorted(rng.choice(np.arange(64, n), 3, replace=False))):
                k[b, key] = q[b, qi] * (big * (step + 1) / np.linalg.norm(q[b, qi])) * np.sqrt(d) / 4
        # a whole 32-row block of queries all spiking at the same late tile, and the first tile
        # all-negative for them
        k[b, 300] = 0
        q[b, 100:132] *= 0.05
        k[b, 300] = q[b, 100:132].mean(0) * 400
    q, k, v = (oracle.decode16(oracle.encode16(x, fmt), fmt) for x in (q, k, v))
    qb, kb, vb = (oracle.encode16(x, fmt) for x in (q, k, v))
    scores = np.einsum("bnd,bmd->bnm", q, k) / np.sqrt(d) * 1.4426950408889634
    run_max = np.maximum.accumulate(scores.reshape(bh, n, n // 64, 64).max(-1), axis=-1)
    jumps = (np.diff(run_max, axis=-1) > 8.0).sum()
    assert jumps > 50, "input does not force the rescale branch"
    want = oracle.forward(q, k, v, accum=1, nthreads=8)
    for algo in _algos_for(d):
        got = _run(fa, torch_cuda, qb, kb, vb, fmt, algo)
        _check(oracle, got, want, fmt, f"forced rescale d={d} fmt={fmt} algo={algo}")


def test_extreme_logits_stay_finite(fa, oracle, torch_cuda):
    """Large-magnitude scores (|s*scale| up to ~600): no overflow/NaN, still matches."""
    (q, k, v), _ = oracle.make_qkv(1, 256, 64, 0, seed=99)
    q *= 12.0
    k *= 12.0
    q, k = (oracle.decode16(oracle.encode16(x, 0), 0) for x in (q, k))
    qb, kb, vb = (oracle.encode16(x, 0) for x in (q, k, v))
    want = oracle.forward(q, k, v, accum=1, nthreads=8)
    for algo in (0, 1):
        got = _run(fa, torch_cuda, qb, kb, vb, 0, algo)
        assert np.isfinite(got).all()
        assert oracle.max_abs(got, want) <= cm.peaked_tol(0, np.abs(v).max())   # near-one-hot rows


def test_bit_reproducible_and_head_independent(fa, oracle, torch_cuda):
    _, (qb, kb, vb) = oracle.make_qkv(6, 300, 64, 1, seed=31)
    a = _run(fa, torch_cuda, qb, kb, vb, 1)
    b = _run(fa, torch_cuda, qb, kb, vb, 1)
    assert np.array_equal(a, b)
    sub = _run(fa, torch_cuda, qb[2:5], kb[2:5], vb[2:5], 1)
    assert np.array_equal(sub, a[2:5])   # a (b,h) slice never depends on its neighbours


def test_baseline_config_properties(fa, oracle, torch_cuda):
    """BASELINE cfg 4 size (B=8,H=16,N=4096,d=64): sampled rows against the oracle plus
    size-independent properties (convexity, constant-V, key-permutation invariance)."""
    torch = torch_cuda
    B, H, N, d = 8, 16, 4096, 64
    for fmt in (0, 1):
        dt = _tdtype(torch, fmt)
        g = torch.Generator(device="cuda").manual_seed(1234 + fmt)
        q = torch.randn(B, H, N, d, generator=g, device="cuda", dtype=torch.float32).to(dt)
        k = torch.randn(B, H, N, d, generator=g, device="cuda", dtype=torch.float32).to(dt)
        v = torch.randn(B, H, N, d, generator=g, device="cuda", dtype=torch.float32).to(dt)
        o = fa.fa_forward(q, k, v)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all()
        # sampled (b,h) slices, 64 rows each, full N keys, on the CPU oracle
        for (b, h, r0) in [(0, 0, 0), (3, 7, 1000), (7, 15, 4032), (5, 2, 2040)]:
            qs, ks, vs = (t[b, h].float().cpu().numpy()[None] for t in (q, k, v))
            want = oracle.forward(qs, ks, vs, accum=0, nthreads=8, row_range=(r0, r0 + 64))
            got = o[b, h, r0:r0 + 64].cpu().numpy()
            _check(oracle, got, want[0, r0:r0 + 64], fmt, f"cfg4 slice b={b} h={h} r0={r0} fmt={fmt}")
        # convexity: every output lies inside the per-column range of V
        vmin = v.float().amin(dim=2, keepdim=True)
        vmax = v.float().amax(dim=2, keepdim=True)
        assert bool(((o >= vmin - 1e-3) & (o <= vmax + 1e-3)).all())
        # key permutation invariance (same permutation applied to K and V)
        perm = torch.randperm(N, generator=g, device="cuda")
        o2 = fa.fa_forward(q[:2], k[:2, :, perm].contiguous(), v[:2, :, perm].contiguous())
        assert float((o2 - o[:2]).abs().max()) <= 5e-3
        # constant V -> constant output
        vc = torch.ones_like(v[:1]) * 0.5
        oc = fa.fa_forward(q[:1], k[:1], vc)
        assert float((oc - 0.5).abs().max()) <= 2e-3
        del q, k, v, o, o2, oc
        torch.cuda.empty_cache()


def test_d128_long_sequence_slice(fa, oracle, torch_cuda):
    """BASELINE cfg 5 per-head shape (N=8192, d=128), a few heads, sampled rows."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = (torch.randn(1, 4, 8192, 128, generator=g, device="cuda").half() for _ in range(3))
    o = fa.fa_forward(q, k, v)
    torch.cuda.synchronize()
    for (h, r0) in [(0, 0), (3, 8128), (2, 4000)]:
        qs, ks, vs = (t[0, h].float().cpu().numpy()[None] for t in (q, k, v))
        want = oracle.forward(qs, ks, vs, accum=0, nthreads=8, row_range=(r0, r0 + 32))
        _check(oracle, o[0, h, r0:r0 + 32].cpu().numpy(), want[0, r0:r0 + 32], 0, f"cfg5 slice h={h} r0={r0}")


# ---------------------------------------------------------------- 16x16 streaming family

def _s16_run(fa, torch, qb, kb, vb, kt=False):
    b, l = qb.shape[0], vb.shape[1]
    Q, K, V = (_to_dev(torch, x, 0) for x in (qb, kb, vb))
    O = torch.full((b, 16, 16), float("nan"), dtype=torch.float32, device="cuda")
    if kt:
        KT = K.transpose(1, 2).contiguous()   # host pre-transpose of the v8+ ABI
        fa.flashattn_streaming_16x16_mw_kt(Q, KT, V, O, b, l, 0.25)
    else:
        fa.flashattn_streaming_16x16_mw(Q, K, V, O, b, l, 0.25)
    torch.cuda.synchronize()
    return O.cpu().numpy()


def test_streaming16_golden(fa, oracle, torch_cuda, golden_dir):
    for path in sorted(glob.glob(os.path.join(golden_dir, "s16_*.npz"))):
        z = np.load(path)
        for kt in (False, True):
            got = _s16_run(fa, torch_cuda, z["q"], z["k"], z["v"], kt)
            _check(oracle, got, z["expected"], 0, f"{os.path.basename(path)} kt={kt}")


def test_streaming16_reference_driver_shape(fa, oracle, torch_cuda):
    """NUM_BATCH=1024, SEQ_LEN=128, N(0,1) seed 42, scale = 1/sqrt(16)
    (flashattn_streaming_16x16_mw.cu:322-349), plus ragged L and a batch count that does not
    fill the last workgroup."""
    for b, l in [(1024, 128), (1023, 128), (5, 16), (7, 200), (3, 24)]:
        nq, nk = b * 256, b * 16 * l
        qb = oracle.encode16(oracle.fill(nq, 42, 0), 0).reshape(b, 16, 16)
        kb = oracle.encode16(oracle.fill(nk, 42, nq), 0).reshape(b, 16, l)
        vb = oracle.encode16(oracle.fill(nk, 42, nq + nk), 0).reshape(b, l, 16)
        want = oracle.streaming_16x16(*(oracle.decode16(x, 0) for x in (qb, kb, vb)), scale=0.25)
        a = _s16_run(fa, torch_cuda, qb, kb, vb, False)
        c = _s16_run(fa, torch_cuda, qb, kb, vb, True)
        _check(oracle, a, want, 0, f"s16 b={b} l={l}")
        assert np.array_equal(a, c), "K and K_T entry points must agree bit for bit"


def test_device_rejects_bad_shapes(fa, torch_cuda):
    torch = torch_cuda
    q = torch.zeros(1, 128, 24, dtype=torch.float16, device="cuda")
    with pytest.raises(fa.FaError):
        fa.fa_forward(q, q, q)                       # D % 16 != 0
    q = torch.zeros(1, 128, 32, dtype=torch.float16, device="cuda")
    with pytest.raises(fa.FaError):
        fa.fa_forward(q, q, q, algo=2)               # tiled kernel needs D in {64,128}


@pytest.mark.parametrize("fmt", [0, 1])
def test_optimistic_pass_overflow_fallback(fa, oracle, torch_cuda, fmt):
    """The d=64 kernels first run without tracking the row max (reference = max of tile 0 + 2^4) and
    re-run a workgroup in tracking mode when a row sum comes out inf/NaN.  Force exactly that, in
    the corner cases: overflow in the very last tile only, for a single query row only, just above
    and just below the 16-bit overflow point, and a whole block whose first tile is far below the rest."""
    n, d, bh = 640, 64, 3
    (q, k, v), _ = oracle.make_qkv(bh, n, d, fmt, seed=777 + fmt)
    ln2 = float(np.log(2.0))

    def spike(b, qi, key, log2_above):
        # make score(qi,key)*log2e exceed that row's tile-0 max by ~log2_above
        s0 = (q[b, qi] @ k[b, :64].T) / np.sqrt(d)
        target = (s0.max() + log2_above * ln2) * np.sqrt(d)
        k[b, key] = q[b, qi] * (target / float(q[b, qi] @ q[b, qi]))

    spike(0, 5, n - 1, 40.0)        # one row, last key of the last tile, far beyond fp16 range
    spike(0, 300, 100, 19.0)        # below the overflow point (4 + 16 = 20): stays in the optimistic pass if alone
    spike(1, 77, 333, 21.5)         # just above it
    spike(1, 78, 334, 150.0 if fmt == 1 else 60.0)   # bf16 overflows only past 2^128
    k[2, 64:] *= 6.0                # rows of head 2: everything after tile 0 is much larger
    q, k, v = (oracle.decode16(oracle.encode16(x, fmt), fmt) for x in (q, k, v))
    qb, kb, vb = (oracle.encode16(x, fmt) for x in (q, k, v))
    want = oracle.forward(q, k, v, accum=1, nthreads=8)
    # A one-hot row reproduces |V| times the rounding error of its single packed weight when the row sum
    # is taken from the unrounded fp32 p: 2^-9 for bf16, |V| <= ~4.5.  The shipped kernels (AUTO, 5, 6)
    # sum the ROUNDED bf16 weights instead and meet the plain bar; the A/B variants do not.
    def tol(algo):
        return cm.MAX_ABS
    for algo in _present((0, 5, 6, 21, 22, 23, 24, 25, 26, 27, 29)):
        got = _run(fa, torch_cuda, qb, kb, vb, fmt, algo)
        _check(oracle, got, want, fmt, f"optimistic/fallback fmt={fmt} algo={algo}", max_abs=tol(algo))
    # ragged N with the overflow in the partial last tile
    n2 = 333
    (q2, k2, v2), _ = oracle.make_qkv(1, n2, d, fmt, seed=9)
    k2[0, n2 - 1] = q2[0, 200] * 40.0
    q2, k2, v2 = (oracle.decode16(oracle.encode16(x, fmt), fmt) for x in (q2, k2, v2))
    want2 = oracle.forward(q2, k2, v2, accum=1, nthreads=8)
    for algo in _present((0, 5, 6, 21, 22, 23, 24, 25, 26, 27, 29)):
        got2 = _run(fa, torch_cuda, *(oracle.encode16(x, fmt) for x in (q2, k2, v2)), fmt, algo)
        _check(oracle, got2, want2, fmt, f"optimistic/fallback ragged fmt={fmt} algo={algo}", max_abs=tol(algo))


# ---- causal variant (not a reference entry point) --------------------------------
def _run_causal(fa, torch, qb, kb, vb, fmt, algo=0, out_same=False):
    q, k, v = (_to_dev(torch, x, fmt) for x in (qb, kb, vb))
    od = _tdtype(torch, fmt) if out_same else torch.float32
    o = fa.fa_forward(q, k, v, out_dtype=od, algo=algo, causal=True)
    torch.cuda.synchronize()
    return o.float().cpu().numpy()


@pytest.mark.parametrize("fmt", [0, 1])
def test_causal_vs_oracle(fa, oracle, torch_cuda, fmt):
    """Every kernel that implements the mask, ragged N around the 32/64/256-row block edges."""
    for d in (16, 64, 128):
        for n in (1, 17, 64, 65, 255, 256, 257, 600):
            (q, k, v), (qb, kb, vb) = oracle.make_qkv(3, n, d, fmt=fmt, seed=900 + n + d)
            want = oracle.forward(q, k, v, causal=True, nthreads=8)
            for algo in (_present((0, 1, 2, 6, 24) + ((28,) if d == 128 else ())) if d in (64, 128) else (0, 1)):
                got = _run_causal(fa, torch_cuda, qb, kb, vb, fmt, algo=algo)
                _check(oracle, got, want, fmt, f"causal d={d} n={n} algo={algo} fmt={fmt}")
            got = _run_causal(fa, torch_cuda, qb, kb, vb, fmt, out_same=True)
            _check(oracle, got, want, fmt, f"causal d={d} n={n} out=same", out_same=True)


def test_causal_prefix_identity(fa, oracle, torch_cuda):
    """Row i of the causal forward == row i of the plain forward over the first i+1 keys, and the
    first row is exactly V[0]: properties that do not need the oracle."""
    n, d = 384, 64
    (q, k, v), (qb, kb, vb) = oracle.make_qkv(2, n, d, fmt=0, seed=77)
    got = _run_causal(fa, torch_cuda, qb, kb, vb, 0)
    np.testing.assert_allclose(got[:, 0], v[:, 0], atol=1e-6)
    for i in (1, 63, 64, 200, 383):
        plain = _run(fa, torch_cuda, qb[:, :i + 1], kb[:, :i + 1], vb[:, :i + 1], 0, algo=2)
        assert np.abs(got[:, i] - plain[:, i]).max() <= 2e-3, i


def test_causal_future_keys_do_not_matter(fa, oracle, torch_cuda):
    """Changing K/V rows j > i must not change output rows <= i, bit for bit."""
    n, d = 300, 128
    (_, _, _), (qb, kb, vb) = oracle.make_qkv(2, n, d, fmt=1, seed=5)
    a = _run_causal(fa, torch_cuda, qb, kb, vb, 1)
    kb2, vb2 = kb.copy(), vb.copy()
    kb2[:, 150:] = kb[:, 150:][:, ::-1]
    vb2[:, 150:] = 0x7BFF   # large finite bf16
    b = _run_causal(fa, torch_cuda, qb, kb2, vb2, 1)
    assert np.array_equal(a[:, :150], b[:, :150])


def test_causal_big(fa, oracle, torch_cuda):
    """B8 H16 N4096 d64 causal: sampled rows against the oracle."""
    fmt, bh, n, d = 0, 128, 4096, 64
    (q, k, v), (qb, kb, vb) = oracle.make_qkv(bh, n, d, fmt=fmt, seed=42)
    got = _run_causal(fa, torch_cuda, qb, kb, vb, fmt)
    assert np.isfinite(got).all()
    for b, r0 in ((0, 0), (17, 1000), (127, 4032)):
        want = oracle.forward(q, k, v, causal=True, nthreads=8, bh_range=(b, b + 1), row_range=(r0, r0 + 64))
        ma = np.abs(got[b, r0:r0 + 64] - want[b, r0:r0 + 64]).max()
        assert ma <= cm.MAX_ABS, (b, r0, ma)


# ---- second, independent oracle on the GPU box: PyTorch's own attention ----------
def _sdpa_fp32(torch, q, k, v, causal):
    """Plain fp32 softmax(QK^T/sqrt(d))V in torch ops, one head at a time (no fused kernel involved)."""
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    n, d = q.shape[-2:]
    mask = torch.ones(n, n, dtype=torch.bool, device=q.device).tril_() if causal else None
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            s = (q[b, h].float() @ k[b, h].float().T) * (1.0 / d ** 0.5)
            if causal:
                s = s.masked_fill(~mask, float("-inf"))
            out[b, h] = torch.softmax(s, dim=-1) @ v[b, h].float()
    return out


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fmt", [0, 1])
def test_full_size_against_torch_fp32(fa, torch_cuda, fmt, causal):
    """ALL rows of B8 H16 N4096 d64 (BASELINE's metric config) against fp32 torch ops on the GPU,
    through the registered custom op."""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import register
    register()
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(8, 16, 4096, 64, generator=g, device="cuda").to(_tdtype(torch, fmt)) for _ in range(3))
    got = torch.ops.fa_mi355.forward(q, k, v, 0.125, causal, True)
    want = _sdpa_fp32(torch, q, k, v, causal)
    torch.cuda.synchronize()
    err = (got - want).abs().max().item()
    assert err <= cm.MAX_ABS and torch.isfinite(got).all(), err
    rel = ((got - want).norm() / want.norm()).item()
    assert rel <= cm.REL_L2[fmt], rel


def test_sdpa_like_matches_torch_sdpa(fa, torch_cuda):
    """Drop-in call shape of F.scaled_dot_product_attention, 16-bit output, d=128."""
    torch = torch_cuda
    from flashattention_kernel_project_amd.torch_op import sdpa_like
    g = torch.Generator(device="cuda").manual_seed(3)
    q, k, v = (torch.randn(2, 4, 1000, 128, generator=g, device="cuda").half() for _ in range(3))
    for causal in (False, True):
        got = sdpa_like(q, k, v, is_causal=causal)
        want = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float(), is_causal=causal)
        assert got.dtype == torch.float16
        assert (got.float() - want).abs().max().item() <= cm.MAX_ABS


# ---- Nq != Nk with a split over the keys (not a reference entry point) -----------
def _run_splitkv(fa, torch, qb, kb, vb, fmt, out_same=False, scale=None):
    q, k, v = (_to_dev(torch, x[None], fmt) for x in (qb, kb, vb))   # B = 1, H = BH
    od = _tdtype(torch, fmt) if out_same else torch.float32
    o = fa.fa_forward_splitkv(q, k, v, scale=scale, out_dtype=od)
    torch.cuda.synchronize()
    return o[0].float().cpu().numpy()


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_splitkv_vs_oracle(fa, oracle, torch_cuda, fmt, d):
    """Few query rows against short, ragged and long K/V: the one-pass (S = 1) and the split + merge
    paths, both output types."""
    for bh, nq, nk in ((3, 1, 64), (2, 5, 100), (2, 16, 1000), (1, 130, 777), (4, 1, 8192 + 37), (16, 3, 4096)):
        (q, _, _), (qb, _, _) = oracle.make_qkv(bh, nq, d, fmt=fmt, seed=10 + nq)
        (_, k, v), (_, kb, vb) = oracle.make_qkv(bh, nk, d, fmt=fmt, seed=20 + nk)
        want = oracle.forward_cross(q, k, v, nthreads=8)
        got = _run_splitkv(fa, torch_cuda, qb, kb, vb, fmt)
        _check(oracle, got, want, fmt, f"splitkv d={d} bh={bh} nq={nq} nk={nk} fmt={fmt}")
        got = _run_splitkv(fa, torch_cuda, qb, kb, vb, fmt, out_same=True)
        _check(oracle, got, want, fmt, f"splitkv d={d} nq={nq} nk={nk} out=same", out_same=True)
    assert fa.splitkv_workspace_bytes(1, 4, 1, 8192 + 37, d) > 0      # that case really was split
    assert fa.splitkv_workspace_bytes(1, 3, 1, 64, d) == 0             # and that one was not


def test_splitkv_equals_plain_forward_on_square_shapes(fa, oracle, torch_cuda):
    """Nq == Nk: same answer as fa_forward (different kernels, so to rounding, not bit-exact), and a
    spiking key in the LAST chunk must win the merge (the per-chunk reference maxima differ by > 2^8)."""
    bh, n, d = 2, 2048, 64
    (q, k, v), _ = oracle.make_qkv(bh, n, d, fmt=0, seed=8)
    k[:, n - 3] = q[:, 7] * 9.0
    q, k = (oracle.decode16(oracle.encode16(x, 0), 0) for x in (q, k))
    qb, kb, vb = (oracle.encode16(x, 0) for x in (q, k, v))
    assert fa.splitkv_workspace_bytes(1, bh, n, n, d) > 0
    a = _run_splitkv(fa, torch_cuda, qb, kb, vb, 0)
    b = _run(fa, torch_cuda, qb, kb, vb, 0)
    assert np.abs(a - b).max() <= 2e-3
    want = oracle.forward_cross(q, k, v, nthreads=8)
    _check(oracle, a, want, 0, "splitkv square with a late spike")


def test_splitkv_rejects_a_short_workspace(fa, torch_cuda):
    torch = torch_cuda
    q = torch.zeros(1, 4, 1, 64, dtype=torch.float16, device="cuda")
    k = torch.zeros(1, 4, 8192, 64, dtype=torch.float16, device="cuda")
    need = fa.splitkv_workspace_bytes(1, 4, 1, 8192, 64)
    assert need > 0
    with pytest.raises(fa.FaError):
        fa.fa_forward_splitkv(q, k, k, workspace=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    fa.fa_forward_splitkv(q, k, k, workspace=torch.empty(need, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


# ---- stage-level debug kernels: each stage alone, against numpy ---------------
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_debug_stages(fa, oracle, torch_cuda, fmt, d):
    """QK^T-only, softmax-only and PV-only, each through the product kernels' LDS images and MFMA
    fragment maps: a layout bug shows up in exactly one of the three."""
    torch = torch_cuda
    bh, n = 2, 200   # ragged: 200 = 3 tiles + 8 keys, 1.56 query blocks
    (q, k, v), (qb, kb, vb) = oracle.make_qkv(bh, n, d, fmt=fmt, seed=321)
    dq, dk, dv = (_to_dev(torch, x, fmt) for x in (qb, kb, vb))
    L = fa.lib()
    st = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / np.sqrt(d)
    # stage 1
    s_dev = torch.full((bh, n, n), float("nan"), dtype=torch.float32, device="cuda")
    assert L.fa_debug_stage(1, dq.data_ptr(), dk.data_ptr(), s_dev.data_ptr(), bh, n, d, scale, fmt, st) == 0
    s_want = np.einsum("bid,bjd->bij", q.astype(np.float64), k.astype(np.float64)) * scale
    s_got = s_dev.cpu().numpy()
    assert np.abs(s_got - s_want).max() <= 2e-5 * max(1.0, np.abs(s_want).max())
    # stage 2 (from the exact S so that the stages are judged independently)
    s_in = torch.from_numpy(s_want.astype(np.float32)).cuda()
    p_dev = torch.zeros((bh, n, n), dtype=_tdtype(torch, fmt), device="cuda")
    assert L.fa_debug_stage(2, s_in.data_ptr(), None, p_dev.data_ptr(), bh, n, d, 0.0, fmt, st) == 0
    w = np.exp(s_want - s_want.max(-1, keepdims=True))
    p_want = w / w.sum(-1, keepdims=True)
    p_got = p_dev.float().cpu().numpy()
    assert np.abs(p_got - p_want).max() <= (2.0 ** -10 if fmt == 0 else 2.0 ** -7) * p_want.max()
    assert np.abs(p_got.sum(-1) - 1.0).max() <= (2e-3 if fmt == 0 else 1e-2)
    # stage 3 (from the rounded P the device produced)
    o_dev = torch.full((bh, n, d), float("nan"), dtype=torch.float32, device="cuda")
    assert L.fa_debug_stage(3, p_dev.data_ptr(), dv.data_ptr(), o_dev.data_ptr(), bh, n, d, 0.0, fmt, st) == 0
    torch.cuda.synchronize()
    o_want = np.einsum("bij,bjd->bid", p_got.astype(np.float64), v.astype(np.float64))
    assert np.abs(o_dev.cpu().numpy() - o_want).max() <= 2e-5
    # and the three chained agree with the fused kernel
    fused = _run(fa, torch, qb, kb, vb, fmt)
    assert np.abs(o_dev.cpu().numpy() - fused).max() <= (2e-3 if fmt == 0 else 1.5e-2)


def test_uniform_inputs_v12_drivers(fa, oracle, torch_cuda):
    """The reference's v12 drivers draw U(-1,1) with seed 123 (flashattn_streaming_16x16_mw_v12f.cu:26-29,305):
    the same distribution through the general-shape entry, every d=64 kernel, and the 16x16 family."""
    (q, k, v), (qb, kb, vb) = oracle.make_qkv(4, 320, 64, fmt=0, seed=123, dist=oracle.UNIFORM)
    want = oracle.forward(q, k, v, nthreads=8)
    for algo in _algos_for(64):
        _check(oracle, _run(fa, torch_cuda, qb, kb, vb, 0, algo), want, 0, f"uniform inputs algo={algo}")
    nb, L = 64, 128
    nq, nk = nb * 256, nb * 16 * L
    qb16 = oracle.encode16(oracle.fill(nq, 123, 0, oracle.UNIFORM), 0).reshape(nb, 16, 16)
    kb16 = oracle.encode16(oracle.fill(nk, 123, nq, oracle.UNIFORM), 0).reshape(nb, 16, L)
    vb16 = oracle.encode16(oracle.fill(nk, 123, nq + nk, oracle.UNIFORM), 0).reshape(nb, L, 16)
    want16 = oracle.streaming_16x16(*(oracle.decode16(x, 0) for x in (qb16, kb16, vb16)), scale=0.25)
    _check(oracle, _s16_run(fa, torch_cuda, qb16, kb16, vb16, False), want16, 0, "s16 uniform inputs")


def test_launchers_are_graph_capturable(fa, torch_cuda):
    """The launchers only enqueue kernels on the caller's stream (no allocation, no sync), so a HIP
    graph captured around them replays to the same bits -- plain, causal and split-KV paths."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = (torch.randn(2, 4, 700, 64, generator=g, device="cuda").half() for _ in range(3))
    q1 = q[:, :, :3].contiguous()
    ws = torch.empty(max(fa.splitkv_workspace_bytes(2, 4, 3, 700, 64), 1), dtype=torch.uint8, device="cuda")
    o = torch.empty(q.shape, dtype=torch.float32, device="cuda")
    oc = torch.empty_like(o)
    eager = (fa.fa_forward(q, k, v).clone(), fa.fa_forward(q, k, v, causal=True).clone(),
             fa.fa_forward_splitkv(q1, k, v, workspace=ws).clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.fa_forward(q, k, v, out=o)
        fa.fa_forward(q, k, v, out=oc, causal=True)
        os_ = fa.fa_forward_splitkv(q1, k, v, workspace=ws)
    o.zero_(), oc.zero_(), os_.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, eager[0]) and torch.equal(oc, eager[1]) and torch.equal(os_, eager[2])


def test_splitkv_grouped_query_heads(fa, oracle, torch_cuda):
    """Hq = G * Hkv: each group of G query heads shares one K/V head (passed to the C ABI as one head
    with G*Nq rows).  Against the oracle run with K/V repeated per query head."""
    torch = torch_cuda
    b, hq, hkv, nq, nk, d = 2, 8, 2, 1, 3000, 128
    g = hq // hkv
    (q, _, _), (qb, _, _) = oracle.make_qkv(b * hq, nq, d, fmt=0, seed=61)
    (_, k, v), (_, kb, vb) = oracle.make_qkv(b * hkv, nk, d, fmt=0, seed=62)
    want = oracle.forward_cross(q, np.repeat(k, g, axis=0), np.repeat(v, g, axis=0), nthreads=8)
    dq = _to_dev(torch, qb, 0).view(b, hq, nq, d)
    dk, dv = (_to_dev(torch, x, 0).view(b, hkv, nk, d) for x in (kb, vb))
    got = fa.fa_forward_splitkv(dq, dk, dv)
    torch.cuda.synchronize()
    _check(oracle, got.view(b * hq, nq, d).float().cpu().numpy(), want, 0, "splitkv GQA")
    nq = 5   # several rows per head: row r of the merged head = (head r // nq, row r % nq)
    (q, _, _), (qb, _, _) = oracle.make_qkv(b * hq, nq, d, fmt=0, seed=63)
    want = oracle.forward_cross(q, np.repeat(k, g, axis=0), np.repeat(v, g, axis=0), nthreads=8)
    got = fa.fa_forward_splitkv(_to_dev(torch, qb, 0).view(b, hq, nq, d), dk, dv)
    torch.cuda.synchronize()
    _check(oracle, got.view(b * hq, nq, d).float().cpu().numpy(), want, 0, "splitkv GQA nq=5")


# ---------------------------------------------------------------- round 2: configs at their stated shapes, AUTO edges, the folded pass

def _sampled_rows_check(fa, oracle, torch, q, k, v, o, fmt, rows, what, max_abs=cm.MAX_ABS, rel_l2=None):
    """q,k,v,o: [B,H,N,d] device tensors; rows: list of (b, h, r0, n) row ranges checked against the oracle."""
    for (b, h, r0, n) in rows:
        qs, ks, vs = (t[b, h].float().cpu().numpy()[None] for t in (q, k, v))
        want = oracle.forward(qs, ks, vs, accum=0, nthreads=8, row_range=(r0, r0 + n))
        _check(oracle, o[b, h, r0:r0 + n].float().cpu().numpy(), want[0, r0:r0 + n], fmt, f"{what} b={b} h={h} rows {r0}..{r0 + n}",
               max_abs=max_abs, rel_l2=rel_l2)


def test_cfg3_exact_shape_through_auto(fa, oracle, torch_cuda):
    """BASELINE config 3 at its stated shape, B=4 H=8 N=1024 d=64 fp16, through FA_ALGO_AUTO (the small-grid branch),
    every row of every head against the oracle (8.6 GFLOP on the CPU)."""
    torch = torch_cuda
    (q, k, v), (qb, kb, vb) = oracle.make_qkv(32, 1024, 64, 0, seed=303)
    sel = fa.lib().fa_selected_algo(4, 8, 1024, 64, 0)
    assert sel == 27, sel   # 256 workgroups of 128 rows: the pipeline on 16-row waves
    Q, K, V = (_to_dev(torch, x, 0).view(4, 8, 1024, 64) for x in (qb, kb, vb))
    o = fa.fa_forward(Q, K, V)
    torch.cuda.synchronize()
    want = oracle.forward(q, k, v, accum=0, nthreads=16)
    _check(oracle, o.view(32, 1024, 64).cpu().numpy(), want, 0, "cfg3 B4 H8 N1024 d64 fp16 AUTO")


@pytest.mark.parametrize("fmt", [0, 1])
def test_cfg5_per_gpu_full_size(fa, oracle, torch_cuda, fmt):
    """BASELINE config 5, one GPU's shard at full size: B=8 H=16 N=8192 d=128.  Sampled row blocks against the oracle,
    plus the size-independent properties: every output inside its head's V range (convexity), constant V -> constant O."""
    torch = torch_cuda
    dt = _tdtype(torch, fmt)
    g = torch.Generator(device="cuda").manual_seed(55 + fmt)
    q, k, v = (torch.randn(8, 16, 8192, 128, generator=g, device="cuda").to(dt) for _ in range(3))
    o = fa.fa_forward(q, k, v)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all())
    _sampled_rows_check(fa, oracle, torch, q, k, v, o, fmt, [(0, 0, 0, 16), (7, 15, 8176, 16), (3, 9, 4090, 16), (5, 2, 6000, 8)], "cfg5")
    vmin = v.float().amin(dim=2, keepdim=True)
    vmax = v.float().amax(dim=2, keepdim=True)
    assert bool(((o >= vmin - 2e-3) & (o <= vmax + 2e-3)).all())
    vc = torch.full_like(v[:1], 0.5)
    oc = fa.fa_forward(q[:1], k[:1], vc)
    assert float((oc - 0.5).abs().max()) <= 4e-3
    del q, k, v, o, oc
    torch.cuda.empty_cache()


@pytest.mark.parametrize("fmt", [0, 1])
def test_auto_dispatch_boundaries(fa, oracle, torch_cuda, fmt):
    """FA_ALGO_AUTO at d=64: N <= 256 keeps the interleaved kernels (256-row workgroups from two per CU upwards); longer
    sequences take the rolling pipeline on the widest waves whose grid still covers the device (512 / 256 / 128-row
    workgroups by rounds x rows / efficiency).  Shapes on each side of the switches, through algo 0, against the oracle."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = fa.lib()
    big = 24
    for (bh, n, want_algo) in [(cus - 1, 512, big), (cus, 512, big), (2 * cus - 1, 256, 6), (2 * cus, 256, 5), (cus, 500, big), (cus // 2, 513, big), (4 * cus, 250, 5),
                               (cus // 8, 1024, 27), (cus // 4, 1024, 26), (cus // 8, 700, 27), (3 * cus // 2, 512, 26),
                               (cus // 16, 2048, 29), (cus // 16, 2000, 27)]:   # 128-row workgroups on long sequences: the key split, where N allows it
        sel = L.fa_selected_algo(bh, 1, n, 64, fmt)
        if want_algo is not None:
            assert sel == want_algo, (bh, n, sel)
        assert L.fa_selected_kernel(bh, 1, n, 64, fmt, 0).decode().startswith("fa::fa_fwd_")
        (q, k, v), (qb, kb, vb) = oracle.make_qkv(bh, n, 64, fmt, seed=900 + bh + n)
        got = _run(fa, torch, qb, kb, vb, fmt)
        heads = sorted({0, bh // 2, bh - 1})
        want = oracle.forward(q[heads], k[heads], v[heads], accum=0, nthreads=16)
        _check(oracle, got[heads], want, fmt, f"AUTO boundary bh={bh} n={n} fmt={fmt} -> algo {sel}")
    # d = 128: one wave per SIMD (28) from N = 4096 wherever the 256-row workgroups are chosen
    for (bh, n, want_algo) in [(cus // 8, 8192, 28), (cus // 32, 8192, 28), (cus // 4, 4096, 28), (cus // 4, 4096 - 64, 24), (cus // 16, 16384, 28), (cus, 2048, 24)]:
        assert L.fa_selected_algo(bh, 1, n, 128, fmt) == want_algo, (bh, n)


def test_bf16_overflow_window_below_inf(fa, oracle, torch_cuda):
    """bf16 keeps p finite up to 2^127, so a late score 120..127 log2 units above the reference leaves the row SUM finite
    while sum(p*v) overflows fp32 at |V| ~ 4: the optimistic pass must still be rejected (finite limit 2^96)."""
    n, d, bh, fmt = 640, 64, 2, 1
    (q, k, v), _ = oracle.make_qkv(bh, n, d, fmt, seed=4321)
    v *= 4.0
    ln2 = float(np.log(2.0))
    for (b, qi, key, lift) in [(0, 9, 500, 122.0), (0, 200, 639, 126.5), (1, 64, 70, 110.0), (1, 300, 300, 97.0)]:
        s0 = (q[b, qi] @ k[b, :64].T) / np.sqrt(d)
        target = (s0.max() + lift * ln2) * np.sqrt(d)
        k[b, key] = q[b, qi] * (target / float(q[b, qi] @ q[b, qi]))
    q, k, v = (oracle.decode16(oracle.encode16(x, fmt), fmt) for x in (q, k, v))
    qb, kb, vb = (oracle.encode16(x, fmt) for x in (q, k, v))
    want = oracle.forward(q, k, v, accum=1, nthreads=8)
    for algo in _present((0, 5, 6, 21, 23, 24, 26, 27)):
        got = _run(fa, torch_cuda, qb, kb, vb, fmt, algo)
        _check(oracle, got, want, fmt, f"bf16 window algo={algo}", max_abs=4 * cm.MAX_ABS)   # |V| = 4 x the N(0,1) bar


@pytest.mark.parametrize("fmt", [0, 1])
def test_folded_pass_gates(fa, oracle, torch_cuda, fmt):
    """The fast pass of FA_ALGO_RP16_FOLD / FA_ALGO_RP_FOLD (scale folded into a rounded Q, one reference maximum per wave) must hand a
    workgroup to the exact pass whenever its assumptions fail, and agree with the exact kernel where they hold."""
    d = 64
    cases = []
    # (a) rows of one wave with very different maxima: the wave reference sits far above some rows' scores
    (q, k, v), _ = oracle.make_qkv(2, 576, d, fmt, seed=61)
    q[0, 0:32] *= 8.0
    q[0, 32:64] *= 0.02
    k[0, 5] = q[0, 3] * 3.0
    cases.append(("mixed row maxima", q, k, v, None))
    # (b) large logits everywhere (reference max beyond kFoldMax)
    (q, k, v), _ = oracle.make_qkv(2, 320, d, fmt, seed=62)
    cases.append(("large logits", q * 6.0, k * 6.0, v, None))
    # (c) Q*scale below fp16's normal range, K large enough that the logits still matter
    (q, k, v), _ = oracle.make_qkv(1, 256, d, fmt, seed=63)
    cases.append(("tiny folded Q", q * 1e-3, k * 50.0, v, 0.02))
    # (d) Q*scale overflowing fp16
    (q, k, v), _ = oracle.make_qkv(1, 256, d, fmt, seed=64)
    cases.append(("overflowing folded Q", q * 200.0, k * 1e-2, v, 300.0))
    # (e) negative scale, ragged N, one key only
    (q, k, v), _ = oracle.make_qkv(3, 333, d, fmt, seed=65)
    cases.append(("negative scale", q, k, v, -0.2))
    (q, k, v), _ = oracle.make_qkv(2, 1, d, fmt, seed=66)
    cases.append(("one key", q, k, v, None))
    # (f) all scores far below zero against a few near it (row sums below the lower gate)
    (q, k, v), _ = oracle.make_qkv(1, 2048, d, fmt, seed=67)
    k[0, 64:] = -np.abs(k[0, 64:]) * 3.0
    q[0] = np.abs(q[0])
    cases.append(("late keys all far below", q, k, v, None))
    # (g) one row hundreds of log2 units below its wave's reference (its weights vanish in fp32), single key
    (q, k, v), _ = oracle.make_qkv(1, 1, d, fmt, seed=68)
    q[0, 0] = -np.abs(k[0, 0]) * 6.0
    cases.append(("row far below the wave reference", q, k * 6.0, v, 1.0))
    # (h) K beyond fp16's range (bf16 inputs: the converted K overflows; fp16 inputs cannot hold it)
    if fmt == 1:
        (q, k, v), _ = oracle.make_qkv(1, 192, d, fmt, seed=69)
        k[0, 100] *= 1e5
        cases.append(("K beyond fp16 range", q * 1e-4, k, v, None))
    # (i) two comparable dominant LATE keys ~60 log2 units above the first-32-key maximum, with different V rows: every gate known
    # before the first tile passes; the folded Q' would move their weight ratio by |logit| 2^-11 -- the row-sum gate must refuse
    (q, k, v), _ = oracle.make_qkv(1, 640, d, fmt, seed=70)
    q[0] *= 0.25
    k[0] *= 0.25
    unit = q[0, 7] / np.linalg.norm(q[0, 7])
    lift = 60.0 / 1.4426950408889634 / (1.0 / np.sqrt(d)) / np.linalg.norm(q[0, 7])   # q.k * scale * log2e = 60
    k[0, 500] = unit * lift
    k[0, 600] = unit * lift * 0.995
    v[0, 500] = 3.0
    v[0, 600] = -3.0
    cases.append(("two dominant late keys 60 log2 units up", q, k, v, None))
    for (name, q, k, v, scale) in cases:
        q, k, v = (oracle.decode16(oracle.encode16(x, fmt), fmt) for x in (q, k, v))
        qb, kb, vb = (oracle.encode16(x, fmt) for x in (q, k, v))
        want = oracle.forward(q, k, v, accum=1, nthreads=8, **({} if scale is None else {"scale": scale}))
        for algo in _present((24, 26, 27, 29, 23, 22, 21, 0)):
            got = _run(fa, torch_cuda, qb, kb, vb, fmt, algo, scale=scale)
            # (case (i): O = 3 (w1 - w2) with w1 ~ w2 -- the row's output nearly cancels, so a relative measure over the tensor says
            # little; the max-abs bar is what holds there)
            _check(oracle, got, want, fmt, f"folded-pass gate: {name} algo={algo} fmt={fmt}",
                   max_abs=cm.MAX_ABS if fmt == 0 else cm.peaked_tol(fmt, np.abs(v).max()),
                   rel_l2=5.0 * cm.REL_L2[fmt] if name.startswith("two dominant") else None)


def _pass_ids(torch, q, k, v, algo):
    """Which pass produced each 512-row block (libfa_mi355_exp.so only: fa_lab_rp16_pass_ids): 0 folded fast pass, 1 exact
    optimistic pass, 2 running-max pass in the kernel, 3 left to the redo kernel."""
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "flashattention_kernel_project_amd", "libfa_mi355_exp.so")
    assert os.path.exists(path), "make -C flashattention_kernel_project_amd/csrc experimental (build() does it)"
    from flashattention_kernel_project_amd import capi
    capi._share_torch_hip_runtime()
    L = C.CDLL(path)
    L.fa_forward_ex.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] + [C.c_int] * 3 + [C.c_void_p]
    L.fa_lab_rp16_pass_ids.argtypes = [C.c_void_p]
    B, H, N, d = q.shape
    ids = torch.full((B * H * ((N + 511) // 512),), 255, dtype=torch.int32, device="cuda")
    out = torch.empty(q.shape, dtype=torch.float32, device="cuda")
    assert L.fa_lab_rp16_pass_ids(ids.data_ptr()) == 0
    try:
        rc = L.fa_forward_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, N, d, 1.0 / d ** 0.5,
                             0 if q.dtype == torch.float16 else 1, 0, algo, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
    finally:
        assert L.fa_lab_rp16_pass_ids(None) == 0
    return ids.cpu().numpy(), out


@pytest.mark.parametrize("fmt", [0, 1])
def test_folded_pass_matches_exact_on_bench_data(fa, oracle, torch_cuda, fmt):
    """N(0,1) inputs at the bench shape: the folded pass IS the pass that runs (asserted through the experimental build's
    per-block pass ids: at least 99 % of the blocks, no block left to the redo kernel) and its output stays within the
    tolerance of the exact pass on every element."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.randn(2, 16, 4096, 64, generator=g, device="cuda").to(_tdtype(torch, fmt)) for _ in range(3))
    ids, a_exp = _pass_ids(torch, q, k, v, 24)
    assert (ids == 0).mean() >= 0.99 and (ids <= 1).all(), np.bincount(ids, minlength=4)
    ids23, _ = _pass_ids(torch, q, k, v, 23)
    assert (ids23 == 1).all(), np.bincount(ids23, minlength=4)   # the exact kernel: its optimistic pass, never the running max, on this data
    a = fa.fa_forward(q, k, v, algo=24)
    b = fa.fa_forward(q, k, v, algo=23)
    torch.cuda.synchronize()
    assert torch.equal(a, a_exp)   # the experimental build's kernel is the product's
    tol = 2e-3 if fmt == 0 else 6e-3
    assert float((a - b).abs().max()) <= tol
    if _have_exp():
        c = fa.fa_forward(q, k, v, algo=22)
        assert float((c - b).abs().max()) <= tol
    _sampled_rows_check(fa, oracle, torch, q, k, v, a, fmt, [(0, 0, 0, 32), (1, 15, 4064, 32), (1, 7, 2000, 16)], "folded pass")


def test_redo_kernel_takes_the_blocks_the_fast_passes_refuse(fa, oracle, torch_cuda):
    """fp16 inputs spread x2 (logits of +-40 log2 units) at the full width: every 512-row block is refused by the folded pass
    before its first tile and left to the redo kernel (pass id 3: the running-max pass on half-width waves, launched behind
    the forward); the result is checked against the oracle on sampled rows and against the exact kernel on all rows.
    bf16 at the same spread stays in the forward (its exact optimistic pass cannot overflow there)."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(2, 8, 4096, 64, generator=g, device="cuda") for _ in range(3))
    for fmt, want_redo in ((0, True), (1, False)):
        dt = _tdtype(torch, fmt)
        qq, kk, vv = (q * 2.0).to(dt), (k * 2.0).to(dt), v.to(dt)
        ids, o_exp = _pass_ids(torch, qq, kk, vv, 24)
        if want_redo:
            assert (ids == 3).all(), np.bincount(ids, minlength=4)
        else:
            assert (ids <= 1).all(), np.bincount(ids, minlength=4)
        o = fa.fa_forward(qq, kk, vv, algo=24)
        torch.cuda.synchronize()
        assert torch.equal(o, o_exp)
        vmax = float(vv.float().abs().max())
        exact = fa.fa_forward(qq, kk, vv, algo=23)
        assert float((o - exact).abs().max()) <= cm.peaked_tol(fmt, vmax, kernels=2) - cm.MAX_ABS + 1e-3
        _sampled_rows_check(fa, oracle, torch, qq, kk, vv, o, fmt, [(0, 0, 0, 16), (1, 7, 4080, 16), (1, 3, 2047, 8)],
                            f"redo kernel fmt={fmt}", max_abs=cm.MAX_ABS if fmt == 0 else cm.peaked_tol(fmt, vmax), rel_l2=None if fmt == 0 else 3e-2)


@pytest.mark.parametrize("fmt", [0, 1])
def test_folded_pass_spread_inputs_all_widths(fa, oracle, torch_cuda, fmt):
    """Q and K spread x1.5 / x2 / x3 (logits x2.25 / x4 / x9): where the wave reference is placed, the gates and the
    fallback chain (folded -> exact optimistic -> tracked) decide the path per workgroup; every width of the pipeline
    (algos 24, 26, 27; d=128: 24, 26) against the oracle on sampled rows and against the exact kernel on all rows."""
    torch = torch_cuda
    dt = _tdtype(torch, fmt)
    for d, algos in ((64, (24, 26, 27, 29)), (128, (24, 26, 28))):
        for spread in (1.5, 2.0, 3.0):
            g = torch.Generator(device="cuda").manual_seed(int(100 * spread) + d + fmt)
            q, k, v = (torch.randn(2, 3, 1152, d, generator=g, device="cuda") for _ in range(3))   # (9 x 128: the key split runs as such)
            q, k, v = (q * spread).to(dt), (k * spread).to(dt), v.to(dt)
            exact = fa.fa_forward(q, k, v, algo=23)
            for algo in algos:
                o = fa.fa_forward(q, k, v, algo=algo)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(o).all()), (d, spread, algo)
                # two of our kernels against each other: each rounds its weights once (the bar itself does not enter)
                vmax = float(v.float().abs().max())
                assert float((o - exact).abs().max()) <= cm.peaked_tol(fmt, vmax, kernels=2) - cm.MAX_ABS + 1e-3, (d, spread, algo)
                _sampled_rows_check(fa, oracle, torch, q, k, v, o, fmt, [(0, 0, 0, 16), (1, 2, 1136, 16), (1, 1, 500, 8)],
                                    f"spread {spread} d={d} algo={algo}", max_abs=cm.MAX_ABS if fmt == 0 else cm.peaked_tol(fmt, vmax),
                                    rel_l2=None if fmt == 0 else 3e-2)


def test_bench_two_rank_rehearsal():
    """bench.py's N > 1 path on ONE device: two ranks started by torch.distributed.run, gloo for the barrier and the
    max-reduction (the driver's own runs use RCCL), exactly one JSON line with n_gpus = 2."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FA_BENCH_BACKEND="gloo", FA_BENCH_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--sustained", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["scaling"] == "weak" and rec["value"] > 0
    # "per-GPU and aggregate" (north_star, config 5): every rank's own figure and the sum, for the metric shape and for config 5's shard
    assert len(rec["per_rank_tflops"]) == 2 and all(x > 0 for x in rec["per_rank_tflops"])
    c5 = rec["cfg5_per_gpu"]
    assert len(c5["per_rank_tflops"]) == 2 and c5["tflops_all_gpus"] > c5["tflops_per_gpu"] > 0 and c5["launches"] >= 30


def test_native_harness_check_step():
    """bench/fa_bench --check: the reference driver's sequence in the native harness (CPU reference, one check launch,
    rel-L2 and max-abs print, then the timed loop) for both families; the error figures are parsed from its output."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bench", "fa_bench")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "bench")])
    subprocess.check_call(["make", "-C", os.path.join(root, "oracle"), "liboracle_cpu.so"], stdout=subprocess.DEVNULL)
    for args, tol_abs, tol_rel in ((["--family", "s16", "--B", "1024", "--N", "128", "--check", "--iters", "5", "--warmup", "2"], 1e-2, 2e-3),
                                   (["--B", "2", "--H", "4", "--N", "512", "--d", "64", "--check", "--iters", "5", "--warmup", "2"], 1e-2, 2e-3),
                                   (["--B", "1", "--H", "2", "--N", "300", "--d", "128", "--dtype", "bf16", "--out", "same", "--check", "--iters", "3", "--warmup", "1"], 3e-2, 1.5e-2)):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        m = re.search(r"rel_l2 = ([0-9.eE+-]+)\s+max_abs = ([0-9.eE+-]+)", out.stdout)
        assert m, out.stdout
        rel, mab = float(m.group(1)), float(m.group(2))
        assert rel <= tol_rel and mab <= tol_abs, (args, rel, mab)
        assert "TFLOPS" in out.stdout


def test_native_harness_two_shard_rehearsal():
    """bench/fa_bench --gpus 2 --one-device: the native driver's multi-GPU mode (contiguous (b,h) shards, one host thread and
    stream per shard, per-shard and aggregate TFLOP/s) rehearsed on ONE device; the shards tile the batch exactly."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bench", "fa_bench")
    subprocess.check_call(["make", "-C", os.path.join(root, "bench")], stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, "--B", "3", "--H", "5", "--N", "512", "--d", "64", "--gpus", "2", "--one-device", "--iters", "5", "--warmup", "2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    shards = re.findall(r"shard (\d) on gpu (\d): \(b,h\) \[(\d+),(\d+)\)\s+avg ([0-9.]+) ms\s+([0-9.]+) TFLOPS", out.stdout)
    assert [(int(a), int(b), int(c), int(d)) for (a, b, c, d, _, _) in shards] == [(0, 0, 0, 8), (1, 0, 8, 15)], out.stdout
    assert all(float(t) > 0 for (*_, t) in shards) and re.search(r"gpus=2\s+[0-9.]+ ms\s+[0-9.]+ TFLOPS aggregate", out.stdout), out.stdout


@pytest.mark.parametrize("fmt", [0, 1])
def test_causal_large_grid_item_order(fa, oracle, torch_cuda, fmt):
    """The causal pipeline alternates the direction of the query blocks between rounds of its persistent grid: with more
    items than CUs every (head, query block) must still be computed exactly once (found by the randomised sweep: a
    direction that depended on the round of the ITEM computed some blocks twice and others never)."""
    torch = torch_cuda
    for (bh, n, d) in ((300, 1000, 64), (300, 1000, 128), (700, 600, 64)):
        g = torch.Generator(device="cuda").manual_seed(3 + bh + d)
        q, k, v = (torch.randn(bh, n, d, generator=g, device="cuda").to(_tdtype(torch, fmt)) for _ in range(3))
        for algo in (0, 24):
            o = fa.fa_forward(q, k, v, algo=algo, causal=True)
            s = (q.float() @ k.float().transpose(1, 2)) * (1.0 / d ** 0.5)
            s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device="cuda").tril_(), float("-inf"))
            want = torch.softmax(s, dim=-1) @ v.float()
            err = float((o - want).abs().max())
            # (bf16 under the mask: the first rows have two or three keys -- peaked by construction)
            assert err <= (cm.MAX_ABS if fmt == 0 else cm.peaked_tol(fmt, float(v.float().abs().max()))), (bh, n, d, algo, err)
            del s, want, o
        del q, k, v
        torch.cuda.empty_cache()


def test_microbenchmarks():
    """the CDNA4 profiling micro-benchmarks build (make -C tools/microbench) and report sane figures --
    matrix-only slots keep the pipe >= 95 % busy, the vector issue costs sit where the kernel's issue model puts them, the
    sustained fp16 MFMA rate is a plausible fraction of the 2.5 PF peak, and the K/V stream alone (staging + barrier, no
    matrix or vector work: the counterpart of flashattn_forward_cp_async_stall.cu:93-206) moves several TB/s into LDS."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mb = os.path.join(root, "tools", "microbench")
    subprocess.check_call(["make", "-C", mb], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(*cmd):
        out = subprocess.run([os.path.join(mb, cmd[0])] + list(cmd[1:]), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout

    import time
    # matrix-only slots: >= 95 % of the pipe.  The chip throttles the ISSUE of matrix instructions when it comes hot out of a
    # power-capped stretch (seen right behind the full test run: 69 % for the same loop), so: settle, and look up to three times
    for attempt in range(3):
        time.sleep(2.0)
        slot = run("slot_model")
        got = []
        for shape in ("MFMA 32x32x16 only", "2 x MFMA 16x16x32 only"):
            m = re.search(re.escape(shape) + r"[^\n]*?2w:\s+([0-9.]+) cyc/slot \(\s*([0-9]+)% MFMA\)", slot)
            assert m, slot[:2000]
            got.append((shape, float(m.group(1)), int(m.group(2))))
        if all(31.0 <= c <= 34.5 and pct >= 95 for (_, c, pct) in got):
            break
    else:
        raise AssertionError(got)
    m = re.search(r"2 x 16x16x32 \+ folded\s+1w:\s+([0-9.]+) cyc/slot.*?2w:\s+([0-9.]+) cyc/slot", slot)
    assert m and 36.0 <= float(m.group(2)) <= 60.0, slot[:3000]   # the loop's floor: matrix issue + vector issue, serialised
    valu = run("valu_rate")
    # (cycles per wave-instruction, one wave alone on its SIMD; 8.9 / 8.3 / 5.4 on a cool chip, up to a quarter more measured
    # on a device that had just left the power cap: sanity ranges, not a calibration)
    for name, lo, hi in (("v_exp_f32", 7.0, 13.5), ("v_cvt_pk_f16_f32", 6.0, 12.5), ("v_fma_f32 (3 VGPR)", 3.5, 8.5)):
        m = re.search(re.escape(name) + r"\s+1 waves/SIMD:\s+([0-9.]+) ticks", valu)
        assert m and lo <= float(m.group(1)) <= hi, (name, m and m.group(1))
    mf = run("mfma_power", "0.5")
    rates = [float(x) for x in re.findall(r"mfma \d+x\d+: ([0-9.]+) TFLOP/s", mf)]
    assert len(rates) == 4 and all(900.0 <= r <= 2600.0 for r in rates), mf
    kv = run("kv_stream")
    m0 = re.search(r"mode 0 .*?staged ([0-9.]+) TB/s", kv)
    m1 = re.search(r"mode 1 .*?staged ([0-9.]+) TB/s", kv)
    ml = re.search(r"LDS fragment reads ([0-9.]+) TB/s", kv)
    assert m0 and m1 and ml, kv
    assert float(m0.group(1)) >= 4.0, kv          # L2 -> LDS, staging + barrier only
    assert float(ml.group(1)) >= 8.0 * float(m1.group(1)) * 0.99, kv
