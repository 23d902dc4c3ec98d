#!/usr/bin/env python3
"""Quick GPU sanity sweep of explicit algo ids against fp32 torch ops (development aid; the parity tests are
tests/test_gpu_parity.py against the CPU oracle).

    python tools/quick_check.py --algos 24,23 [--exp]     (--exp: the experimental library, for 21, 22, 25)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ref(q, k, v, scale):
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    return torch.softmax(s, dim=-1) @ v.float()


ap = argparse.ArgumentParser()
ap.add_argument("--algos", default="24,23")
ap.add_argument("--exp", action="store_true")
args = ap.parse_args()
if args.exp:
    os.environ["FA_MI355_LIB"] = os.path.join(ROOT, "flashattention_kernel_project_amd", "libfa_mi355_exp.so")
import torch  # noqa: E402
import flashattention_kernel_project_amd as fa  # noqa: E402

algos = [int(a) for a in args.algos.split(",")]
g = torch.Generator(device="cuda").manual_seed(1)
worst = {a: 0.0 for a in algos}
fails = 0
cases = []
for dt in (torch.float16, torch.bfloat16):
    for (bh, n) in ((1, 1), (2, 17), (3, 64), (2, 65), (1, 127), (2, 128), (1, 129), (3, 513), (2, 1000), (1, 2048), (64, 1024)):
        for (spread, scale) in ((1.0, None), (2.5, None), (1.0, -0.125), (1.0, 1.0), (6.0, 1.0), (1e-3, 0.125), (300.0, 1e-5)):
            cases.append((dt, bh, n, spread, scale))
for (dt, bh, n, spread, scale) in cases:
    q, k, v = (torch.randn(bh, n, 64, generator=g, device="cuda") * spread for _ in range(3))
    q, k, v = q.to(dt), k.to(dt), (v / spread).to(dt)
    sc = scale if scale is not None else 0.125
    want = ref(q, k, v, sc)
    for a in algos:
        for od in (torch.float32, dt):
            got = fa.fa_forward(q, k, v, scale=sc, algo=a, out_dtype=od).float()
            err = float((got - want).abs().max())
            tol = 1e-2 * (1.0 if dt == torch.float16 else 2.5) + (float(want.abs().max()) * 2 ** -8 if od != torch.float32 and dt == torch.bfloat16 else 0.0)
            ok = bool(torch.isfinite(got).all()) and err <= tol
            worst[a] = max(worst[a], err)
            if not ok:
                fails += 1
                print(f"FAIL algo {a} dt {dt} out {od} bh {bh} n {n} spread {spread} scale {scale}: max_abs {err:.3e} (tol {tol:.1e}) finite {bool(torch.isfinite(got).all())}")
# spikes: one key far above the rest in a late tile (overflow of the optimistic pass), |V| ~ 4
for dt in (torch.float16, torch.bfloat16):
    for lift in (10.0, 30.0, 80.0, 125.0, 160.0):
        q, k, v = (torch.randn(2, 640, 64, generator=g, device="cuda") for _ in range(3))
        v = v * 4
        k[:, 600] = q[:, 5] * (lift * 8.0 / 0.6931 / float((q[0, 5] ** 2).sum())) * 0.6931   # logit of (row 5, key 600) ~ lift / log2e-ish
        q, k, v = q.to(dt), k.to(dt), v.to(dt)
        want = ref(q, k, v, 0.125)
        for a in algos:
            got = fa.fa_forward(q, k, v, scale=0.125, algo=a).float()
            err = float((got - want).abs().max())
            tol = 1e-2 if dt == torch.float16 else 4e-2
            ok = bool(torch.isfinite(got).all()) and err <= tol
            worst[a] = max(worst[a], err)
            if not ok:
                fails += 1
                print(f"FAIL spike algo {a} dt {dt} lift {lift}: max_abs {err:.3e} finite {bool(torch.isfinite(got).all())}")
print("worst max-abs per algo:", {a: f"{w:.3e}" for a, w in worst.items()}, "failures:", fails)
sys.exit(1 if fails else 0)
