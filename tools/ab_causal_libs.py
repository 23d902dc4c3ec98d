"""tools/ab_libs.py for the causal entry point: interleaved rounds of fa_forward_causal (algo 24, fp16, B8 H16 N4096 at d = 64 and
d = 128), several builds of the library in one process:  python tools/ab_causal_libs.py lib_a.so,lib_b.so"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from flashattention_kernel_project_amd import capi
capi._share_torch_hip_runtime()
libs = []
for path in sys.argv[1].split(","):
    L = C.CDLL(os.path.abspath(path))
    L.fa_forward_causal.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] + [C.c_int] * 3 + [C.c_void_p]
    L.fa_forward_causal.restype = C.c_int
    libs.append((os.path.basename(path), L))
st = torch.cuda.current_stream().cuda_stream
for (B, H, N, d) in ((8, 16, 4096, 64), (8, 16, 4096, 128)):
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(B, H, N, d, generator=g, device="cuda").half() for _ in range(3))
    outs = [torch.empty(q.shape, device="cuda", dtype=torch.float32) for _ in libs]
    def run(i):
        rc = libs[i][1].fa_forward_causal(q.data_ptr(), k.data_ptr(), v.data_ptr(), outs[i].data_ptr(), B, H, N, d, 1.0 / d ** 0.5, 0, 0, 24, st)
        assert rc == 0, rc
    for i in range(len(libs)):
        for _ in range(3):
            run(i)
    torch.cuda.synchronize()
    times = [[] for _ in libs]
    for _ in range(24):
        for i in range(len(libs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                run(i)
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / 20)
    print(f"causal B{B} H{H} N{N} d{d} fp16, algo 24, 24 rounds x 20 launches")
    for i, (name, _) in enumerate(libs):
        print(f"{name:24s} median {statistics.median(times[i]):.4f} ms  min {min(times[i]):.4f} ms  max|d| vs first {float((outs[i] - outs[0]).abs().max()):.1e}", flush=True)
