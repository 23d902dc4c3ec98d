"""The flat C entries of include/fa_mi355.h, called through fa.lib() as they are.

The Python front end reaches the KV-cache kernels through the descriptor entries alone (fa_kvcache_decode, fa_kvcache_append_ex), so
a bit tie between a flat entry and its descriptor form takes its flat side from here.  The argument lists follow the rule that
flashattention_kernel_project_amd/capi.py states: each suffix of the name inserts its arguments.
"""
import math


def _ptr(t):
    return None if t is None else t.data_ptr()


def decode(fa, torch, q, k, v, seqlens, causal, fmt, workspace, table=None, scales=None, window=None):
    """fa_forward_kvcache[_paged][_fp8][_window]: _paged with a block table, _fp8 with scales = (k_scale, v_scale), _window with a
    window that is not None (0 included).  q [B,Hq,Nq,d], k/v a cache [B,Hkv,Ncap,d] or a pool [num_pages,Hkv,page_size,d], fmt the
    input dtype id, scale 1/sqrt(d), fp32 output.  -> O, lse, NaN wherever the entry did not write"""
    paged, fp8, windowed = table is not None, scales is not None, window is not None
    B, Hq, Nq, d = q.shape
    Hkv = k.shape[1]
    o = torch.full(q.shape, float("nan"), dtype=torch.float32, device=q.device)
    lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=q.device)
    args = [_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(seqlens)]
    args += [_ptr(table)] if paged else []
    args += [_ptr(scales[0]), _ptr(scales[1])] if fp8 else []
    args += [B, Hkv, Hq // Hkv, Nq]
    args += [k.shape[0], k.shape[2], table.shape[1]] if paged else [k.shape[2]]
    args += [d, 1.0 / math.sqrt(d), 1 if causal else 0]
    args += [window] if windowed else []
    args += [fmt, fa.capi.OUT_F32, _ptr(workspace), workspace.numel(), torch.cuda.current_stream().cuda_stream]
    torch.cuda.synchronize()
    assert getattr(fa.lib(), "fa_forward_kvcache" + "_paged" * paged + "_fp8" * fp8 + "_window" * windowed)(*args) == 0
    torch.cuda.synchronize()
    return o, lse


def append(fa, torch, k_new, v_new, k, v, seqlens, seqlens_out, fmt, table=None, scales=None, rope=None):
    """fa_kvcache_append[_paged][_fp8][_rope]: _paged with a block table, _fp8 with scales = (k_scale, v_scale), _rope with
    rope = (q or None, q_out or None, cos, sin, interleaved).  k_new/v_new [B,Hkv,Nnew,d], k/v a cache or a pool as in decode, fmt
    the dtype id of the new rows.  The caches, seqlens_out and q_out are written in place."""
    paged, fp8, rotary = table is not None, scales is not None, rope is not None
    B, Hkv, Nnew, d = k_new.shape
    args = [_ptr(k_new), _ptr(v_new), _ptr(k), _ptr(v), _ptr(seqlens), _ptr(seqlens_out)]
    args += [_ptr(table)] if paged else []
    args += [_ptr(scales[0]), _ptr(scales[1])] if fp8 else []
    if rotary:
        q, q_out, cos, sin, interleaved = rope
        args += [_ptr(q), _ptr(q_out), _ptr(cos), _ptr(sin)]
    args += [B, Hkv, Nnew]
    args += [k.shape[0], k.shape[2], table.shape[1]] if paged else [k.shape[2]]
    args += [d]
    args += [1 if q is None else q.shape[1] // Hkv, 2 * cos.shape[1], cos.shape[0], 1 if interleaved else 0] if rotary else []
    args += [fmt, torch.cuda.current_stream().cuda_stream]
    assert getattr(fa.lib(), "fa_kvcache_append" + "_paged" * paged + "_fp8" * fp8 + "_rope" * rotary)(*args) == 0
    torch.cuda.synchronize()
