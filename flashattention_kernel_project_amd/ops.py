"""torch-tensor front end over the C ABI, keeping the reference's argument lists.

PyTorch is plumbing only (device memory + streams); every op goes through libfa_mi355.so.
"""
from __future__ import annotations

import math

from . import capi


def attention_flops(bh: int, n: int, d: int) -> float:
    """4*BH*N^2*D (QK^T + PV, non-causal) -- the reference's own count,
    FlashAttention/flashattn_forward_memory_bound/flashattn_forward_wmma_memprofile.cu:508."""
    return 4.0 * bh * n * n * d


def attention_min_bytes(bh: int, n: int, d: int, in_bytes: int = 2, out_bytes: int = 4) -> float:
    """3*BH*N*D*sizeof(in) + BH*N*D*sizeof(out): memprofile.cu:518-520."""
    return 3.0 * bh * n * d * in_bytes + 1.0 * bh * n * d * out_bytes


def _stream_ptr(stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return getattr(stream, "cuda_stream", stream)


def _one_device(*tensors):
    """All tensors on one GPU; returns it.  The C side launches on (and reads the CU count / sets the LDS
    attribute of) the CURRENT device, so every entry point below makes the tensors' device current."""
    dev = tensors[0].device
    for t in tensors[1:]:
        if t is not None and t.device != dev:
            raise ValueError("all tensors of one call must live on one device")
    return dev


def _dev_ptr(t, name: str, dtypes):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} has dtype {t.dtype}, expected one of {dtypes}")
    return t.data_ptr()


def _in_dt(dtype) -> int:
    """the C ABI's id of a 16-bit input dtype that has been checked"""
    import torch
    return capi.F16 if dtype == torch.float16 else capi.BF16


def _out_dt(out_dtype, in_dtype) -> int:
    """the C ABI's id of an output dtype, which is float32 or the input's"""
    import torch
    if out_dtype not in (torch.float32, in_dtype):
        raise ValueError("out_dtype must be torch.float32 or the input dtype")
    return capi.OUT_F32 if out_dtype == torch.float32 else capi.OUT_SAME


def _scale_or_default(scale, d: int):
    return 1.0 / math.sqrt(d) if scale is None else scale


def flashattn_forward_wmma(Q, K, V, O, BH: int, N: int, D: int, scale: float, stream=None) -> None:
    """(Q,K,V,O,BH,N,D,scale) of flashattn_forward_wmma_kernel
    (FlashAttention/flashattn_forward_wmma/flashattn_forward_wmma.cu:49-58).
    Q,K,V: fp16 [BH,N,D]; O: fp32 [BH,N,D], fully overwritten."""
    import torch
    for name, t in (("Q", Q), ("K", K), ("V", V)):
        if t.numel() != BH * N * D:
            raise ValueError(f"{name} has {t.numel()} elements, expected BH*N*D = {BH * N * D}")
    if O.numel() != BH * N * D:
        raise ValueError("O has the wrong number of elements")
    ptrs = (_dev_ptr(Q, "Q", (torch.float16,)), _dev_ptr(K, "K", (torch.float16,)),
            _dev_ptr(V, "V", (torch.float16,)), _dev_ptr(O, "O", (torch.float32,)))
    with torch.cuda.device(_one_device(Q, K, V, O)):
        code = capi.lib().flashattn_forward_wmma(*ptrs, BH, N, D, float(scale), _stream_ptr(stream))
    capi.check("flashattn_forward_wmma", code)


def fa_forward(q, k, v, scale: float | None = None, out_dtype=None, algo: int = capi.ALGO_AUTO,
               out=None, stream=None, causal: bool = False):
    """Attention forward on [B,H,N,d] (or [BH,N,d]) fp16/bf16 device tensors.
    out_dtype: torch.float32 (the reference's output type, default) or the input dtype.
    causal: query row i attends to keys 0..i (fa_forward_causal; algo AUTO / GENERIC / TILED / RP16_FOLD, RP16_FOLD_1W at d=128)."""
    import torch
    if q.dim() == 3:
        B, (H, N, d) = 1, q.shape
    elif q.dim() == 4:
        B, H, N, d = q.shape
    else:
        raise ValueError("q must be [B,H,N,d] or [BH,N,d]")
    if k.shape != q.shape or v.shape != q.shape:
        raise ValueError("q, k, v must have identical shapes (self-attention, Nq == Nk)")
    if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("q, k, v must all be fp16 or all bf16")
    in_dt = _in_dt(q.dtype)
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    out_dt = _out_dt(out_dtype, q.dtype)
    if out is None:
        out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != out_dtype:
        raise ValueError("out has the wrong shape or dtype")
    scale = _scale_or_default(scale, d)
    dts = (torch.float16, torch.bfloat16)
    fn_name = "fa_forward_causal" if causal else "fa_forward_ex"
    with torch.cuda.device(_one_device(q, k, v, out)):   # the launch goes to the CURRENT device: make that the tensors' device
        code = getattr(capi.lib(), fn_name)(
            _dev_ptr(q, "q", dts), _dev_ptr(k, "k", dts), _dev_ptr(v, "v", dts),
            _dev_ptr(out, "out", (out_dtype,)), B, H, N, d, float(scale), in_dt, out_dt, algo,
            _stream_ptr(stream))
    capi.check(fn_name, code)
    return out


def fa_forward_splitkv(q, k, v, scale: float | None = None, out_dtype=None, workspace=None, stream=None):
    """q [B,Hq,Nq,d], k/v [B,Hkv,Nk,d] fp16/bf16 device tensors, no mask, d in {64,128}: the key axis is
    cut into chunks that run in parallel and are merged (fa_forward_splitkv, "flash-decoding").
    Hq may be a multiple of Hkv (grouped-query attention): the G = Hq/Hkv query heads of a group are
    contiguous in q, so the group is passed to the C ABI as ONE head with G*Nq query rows and its K/V is
    streamed once for all of them -- no copy, same kernel.
    workspace: optional uint8 device tensor of at least splitkv_workspace_bytes(B, Hkv, G*Nq, Nk, d)."""
    import torch
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise ValueError("q must be [B,Hq,Nq,d] and k, v [B,Hkv,Nk,d]")
    B, Hq, Nq, d = q.shape
    H, Nk = k.shape[1], k.shape[2]
    if Hq % H != 0:
        raise ValueError("the number of query heads must be a multiple of the number of K/V heads")
    rows = (Hq // H) * Nq   # query rows that share one K/V head
    if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("q, k, v must all be fp16 or all bf16")
    in_dt = _in_dt(q.dtype)
    out_dtype = out_dtype or torch.float32
    out_dt = _out_dt(out_dtype, q.dtype)
    out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    need = splitkv_workspace_bytes(B, H, rows, Nk, d)   # from the shape alone: the split count reads no device property
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_ptr, ws_len = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    scale = _scale_or_default(scale, d)
    dts = (torch.float16, torch.bfloat16)
    ptrs = (_dev_ptr(q, "q", dts), _dev_ptr(k, "k", dts), _dev_ptr(v, "v", dts), _dev_ptr(out, "out", (out_dtype,)))
    with torch.cuda.device(_one_device(q, k, v, out, workspace)):
        code = capi.lib().fa_forward_splitkv(*ptrs, B, H, rows, Nk, d, float(scale), in_dt, out_dt, ws_ptr, ws_len, _stream_ptr(stream))
    capi.check("fa_forward_splitkv", code)
    return out


def splitkv_workspace_bytes(B: int, H: int, Nq: int, Nk: int, d: int) -> int:
    return int(capi.lib().fa_forward_splitkv_workspace_bytes(B, H, Nq, Nk, d))


def _decode(q, k, v, k_name, v_name, cache_seqlens, causal, scale, out_dtype, return_lse, workspace, stream, window, paged=False,
            block_table=None, scales=None, sinks=None, softcap=0.0, seqlens_q=None):
    """The four decode front ends: k, v (named k_name, v_name in messages) are a cache [B,Hkv,Ncap,d] or, with `paged`, a pool
    [num_pages,Hkv,page_size,d] behind block_table; scales is None (a 16-bit cache) or (k_scale, v_scale) of an fp8 one.  Every call
    is fa_kvcache_decode, whose descriptor names each field; without sinks, softcap and seqlens_q that IS the flat entry
    fa_forward_kvcache + _paged + _fp8 + _window of the same layout (include/fa_mi355.h)."""
    import torch
    fp8 = scales is not None
    table_ptr = ks_ptr = vs_ptr = None
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape or q.shape[3] != k.shape[3] or (not paged and q.shape[0] != k.shape[0]):
        raise ValueError(f"q must be [B,Hq,Nq,d] and {k_name}, {v_name} " + ("[num_pages,Hkv,page_size,d]" if paged else "[B,Hkv,Ncap,d]"))
    B, Hq, Nq, d = q.shape
    Hkv = k.shape[1]
    dts = (torch.float16, torch.bfloat16)
    if fp8:   # the cache format is judged first, then (paged) the table: before q and before anything that needs a device
        if k.dtype != torch.float8_e4m3fn or v.dtype != torch.float8_e4m3fn:
            raise ValueError(f"{k_name}, {v_name}: {_FP8_CACHE} (got {k.dtype}, {v.dtype})")
        if paged:
            table_ptr = _table_ptr(block_table, B)
        if q.dtype not in dts:
            raise ValueError("q must be fp16 or bf16")
    if Hq % Hkv != 0:
        raise ValueError("the number of query heads must be a multiple of the number of K/V heads")
    G = Hq // Hkv
    if not fp8 and (q.dtype not in dts or k.dtype != q.dtype or v.dtype != q.dtype):
        raise ValueError(f"q, {k_name}, {v_name} must all be fp16 or all bf16")
    out_dtype = out_dtype or torch.float32
    out_dt = _out_dt(out_dtype, q.dtype)
    if fp8:
        ks_ptr, vs_ptr = _scale_ptrs(scales[0], scales[1], Hkv)
    elif paged:
        table_ptr = _table_ptr(block_table, B)
    cache_dts = (torch.float8_e4m3fn,) if fp8 else dts
    len_ptr = None
    if cache_seqlens is not None:
        if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dim() != 1 or cache_seqlens.shape[0] != B:
            raise ValueError("cache_seqlens must be an int32 device tensor of shape [B]")
        len_ptr = _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    q_ptr, k_ptr, v_ptr = (_dev_ptr(q, "q", dts), _dev_ptr(k, "k cache" if fp8 else k_name, cache_dts),
                           _dev_ptr(v, "v cache" if fp8 else v_name, cache_dts))
    out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    lse = torch.empty((B, Hq, Nq), dtype=torch.float32, device=q.device) if return_lse else None
    window = _window(window)
    softcap = _softcap(softcap)
    sink_ptr = _sinks_ptr(sinks, Hq, q.device)
    nq_ptr = _counts_ptr(seqlens_q, "seqlens_q", B, q.device)
    # a cache has Ncap, a pool (num_pages, page_size, max_pages); the fields of the other layout are 0
    Ncap, num_pages, page_size, max_pages = (0, k.shape[0], k.shape[2], block_table.shape[1]) if paged else (k.shape[2], 0, 0, 0)
    if workspace is None:
        # from the shape and the window alone (the split count reads no device property); the 16-bit entry's for an fp8 cache
        need = kvcache_paged_window_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d, window) if paged \
            else kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, window)
        if need:
            workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_ptr, ws_len = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    desc = capi.new_desc(capi.KvDecodeDesc)
    capi.fill(
        desc, Q=q_ptr, K=k_ptr, V=v_ptr, O=out.data_ptr(), lse=lse.data_ptr() if return_lse else None, seqlens_k=len_ptr,
        block_table=table_ptr, k_scale=ks_ptr, v_scale=vs_ptr, sinks=sink_ptr, kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT,
        B=B, Hkv=Hkv, G=G, Nq=Nq, d=d, Ncap=Ncap, num_pages=num_pages, page_size=page_size, max_pages=max_pages,
        scale=float(_scale_or_default(scale, d)), causal=1 if causal else 0, window=window, softcap=softcap, in_dtype=_in_dt(q.dtype),
        out_dtype=out_dt, workspace=ws_ptr, workspace_bytes=ws_len, stream=_stream_ptr(stream), seqlens_q=nq_ptr)
    with torch.cuda.device(_one_device(q, k, v, block_table, *(scales or ()), cache_seqlens, workspace, sinks, seqlens_q)):
        code = capi.lib().fa_kvcache_decode(desc)
    capi.check("fa_kvcache_decode", code)
    return (out, lse) if return_lse else out


def fa_forward_kvcache(q, k_cache, v_cache, cache_seqlens=None, causal: bool = False, scale: float | None = None,
                       out_dtype=None, return_lse: bool = False, workspace=None, stream=None, window: int = 0, sinks=None,
                       softcap: float = 0.0, seqlens_q=None):
    """Decode against a pre-allocated cache (fa_forward_kvcache): q [B,Hq,Nq,d], k_cache/v_cache [B,Hkv,Ncap,d]
    fp16/bf16 device tensors, d in {64,128}, Hq a multiple of Hkv (the group's K/V is streamed once, as in
    fa_forward_splitkv).
    cache_seqlens: int32 contiguous device tensor [B], the keys each sequence holds (None: Ncap for all).  It is read on
    the device only, so a call captured into a graph follows lengths that are later changed in place.
    causal: row i sees the keys [0, L_b - Nq + 1 + i) -- the last query row sees the whole sequence.
    A row that sees no key returns zeros (and lse = -inf).
    return_lse: also return the fp32 [B,Hq,Nq] natural-log sum of exponentials, for merging results over key ranges.
    workspace: optional uint8 device tensor of at least kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d).
    window: 0 (no window), or W >= 1: row i sees only the keys [max(0, L_b - Nq + 1 + i - W), its upper limit) -- with causal its own
    position and the W - 1 before it (fa_forward_kvcache_window).  Keys below row 0's lower limit are never used.  The window is a host
    integer (baked into a captured call); the workspace is then sized by kvcache_window_workspace_bytes.
    softcap: 0 (off), or a finite float > 0: every logit s becomes softcap * tanh(s / softcap) before the masks and the softmax
    (flash-attn's softcap; baked into a captured call).
    sinks: None, or a float32 contiguous device tensor of Hq values: head h gets one extra key with the natural-log logit sinks[h]
    (not scaled, not capped) and a zero V row, which every row sees under any mask or window -- lse includes it; -inf: no sink for
    that head.  Read on the device only.  When merging over key ranges, pass sinks to exactly one range.
    seqlens_q: None, or an int32 contiguous device tensor [B]: Nq is then the PADDED row count and sequence b has
    n_b = min(max(seqlens_q[b], 0), Nq) live rows per head, rows i < n_b, with n_b in the place of Nq in the causal and window limits.
    Dead rows return O = 0 and lse = -inf exactly and their q rows are never used; n_b = 0 is an idle slot that reads nothing of the
    sequence.  Read on the device only: a captured call follows counts rewritten in place; grid, splits and workspace follow the padded Nq.
    The C call is always the descriptor entry fa_kvcache_decode; without the last three it is, bit for bit, the flat entry named above
    (fa_forward_kvcache, with a window fa_forward_kvcache_window).  Workspace sizes do not depend on the three."""
    return _decode(q, k_cache, v_cache, "k_cache", "v_cache", cache_seqlens, causal, scale, out_dtype, return_lse, workspace, stream,
                   window, sinks=sinks, softcap=softcap, seqlens_q=seqlens_q)


def kvcache_workspace_bytes(B: int, Hkv: int, G: int, Nq: int, Ncap: int, d: int) -> int:
    return int(capi.lib().fa_forward_kvcache_workspace_bytes(B, Hkv, G, Nq, Ncap, d))


def kvcache_window_workspace_bytes(B: int, Hkv: int, G: int, Nq: int, Ncap: int, d: int, window: int) -> int:
    """Workspace of the windowed contiguous entries (16 bit and fp8): the split count follows the window, not the capacity."""
    return int(capi.lib().fa_forward_kvcache_window_workspace_bytes(B, Hkv, G, Nq, Ncap, d, window))


def _softcap(softcap) -> float:
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)) or not (0.0 <= softcap < math.inf):
        raise ValueError("softcap must be a finite float >= 0 (0: no soft-cap)")
    return float(softcap)


def _sinks_ptr(sinks, Hq: int, device):
    """None, or the device pointer of a checked sink vector: one fp32 natural-log logit per query head."""
    if sinks is None:
        return None
    import torch
    if not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32:
        raise ValueError("sinks must be a float32 device tensor")
    if sinks.numel() != Hq:
        raise ValueError(f"sinks must hold one value per query head ({Hq}), got {sinks.numel()}")
    if not sinks.is_contiguous():
        raise ValueError("sinks must be contiguous")
    if sinks.device != device:
        raise ValueError(f"sinks is on {sinks.device}, q on {device}")
    return _dev_ptr(sinks, "sinks", (torch.float32,))


def _counts_ptr(counts, name: str, B: int, device):
    """None, or the device pointer of a checked per-sequence count vector (seqlens_q, seqlens_new): one int32 per sequence."""
    if counts is None:
        return None
    import torch
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32:
        raise ValueError(f"{name} must be an int32 device tensor")
    if counts.numel() != B or counts.dim() != 1:
        raise ValueError(f"{name} must hold one value per sequence (shape [{B}]), got {tuple(counts.shape)}")
    if not counts.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if counts.device != device:
        raise ValueError(f"{name} is on {counts.device}, the call's tensors on {device}")
    return _dev_ptr(counts, name, (torch.int32,))


def _window(window) -> int:
    if isinstance(window, bool) or not isinstance(window, int) or window < 0:
        raise ValueError("window must be an int >= 0 (0: no window)")
    return window


def fa_forward_kvcache_paged(q, k_pool, v_pool, block_table, cache_seqlens=None, causal: bool = False, scale: float | None = None,
                             out_dtype=None, return_lse: bool = False, workspace=None, stream=None, window: int = 0, sinks=None,
                             softcap: float = 0.0, seqlens_q=None):
    """fa_forward_kvcache against a paged cache (fa_forward_kvcache_paged): q [B,Hq,Nq,d], k_pool/v_pool
    [num_pages,Hkv,page_size,d] fp16/bf16 contiguous device tensors (a contiguous slice of a larger pool, pool[2:6], is a pool),
    d in {64,128}, page_size a power of two >= 16, Hq a multiple of Hkv.
    block_table: int32 contiguous device tensor [B, max_pages]; key j of sequence b is row j % page_size of page
    block_table[b, j // page_size].  The capacity is max_pages * page_size.  Entries past a sequence's last live page are not read;
    a live entry outside [0, num_pages) reads as a page of zeros.
    cache_seqlens, causal, scale, out_dtype, return_lse: as in fa_forward_kvcache.  Table and lengths are read on the device only,
    so a call captured into a graph follows both when they are later rewritten in place.
    workspace: optional uint8 device tensor of at least kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d).
    window: 0 (no window), or W >= 1: row i sees only the keys [max(0, L_b - Nq + 1 + i - W), its upper limit) -- with causal its own
    position and the W - 1 before it (fa_forward_kvcache_paged_window).  Keys below row 0's lower limit are never used.  The window is a host
    integer (baked into a captured call); the workspace is then sized by kvcache_paged_window_workspace_bytes.
    Under a window a page wholly below row 0's lower limit is not dereferenced and its table entry is not read.
    sinks, softcap, seqlens_q: as in fa_forward_kvcache."""
    return _decode(q, k_pool, v_pool, "k_pool", "v_pool", cache_seqlens, causal, scale, out_dtype, return_lse, workspace, stream,
                   window, paged=True, block_table=block_table, sinks=sinks, softcap=softcap, seqlens_q=seqlens_q)


def kvcache_paged_workspace_bytes(B: int, Hkv: int, G: int, Nq: int, max_pages: int, page_size: int, d: int) -> int:
    return int(capi.lib().fa_forward_kvcache_paged_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d))


def kvcache_paged_window_workspace_bytes(B: int, Hkv: int, G: int, Nq: int, max_pages: int, page_size: int, d: int, window: int) -> int:
    """Workspace of the windowed paged entries (16 bit and fp8): kvcache_window_workspace_bytes for Ncap = max_pages * page_size."""
    return int(capi.lib().fa_forward_kvcache_paged_window_workspace_bytes(B, Hkv, G, Nq, max_pages, page_size, d, window))


_FP8_CACHE = "an fp8 cache must be torch.float8_e4m3fn (OCP e4m3fn, the gfx950 format); float8_e4m3fnuz, float8_e5m2 and " \
             "16-bit caches are not accepted here"


def fa_forward_kvcache_fp8(q, k_cache, v_cache, k_scale=None, v_scale=None, cache_seqlens=None, causal: bool = False,
                           scale: float | None = None, out_dtype=None, return_lse: bool = False, workspace=None, stream=None,
                           window: int = 0, sinks=None, softcap: float = 0.0, seqlens_q=None):
    """fa_forward_kvcache against an fp8 cache (fa_forward_kvcache_fp8): q [B,Hq,Nq,d] fp16/bf16, k_cache/v_cache [B,Hkv,Ncap,d]
    torch.float8_e4m3fn (OCP e4m3fn; fnuz and e5m2 are refused) device tensors, d in {64,128}.  K and V are widened to q's type
    on the way into the kernel, exactly.
    k_scale, v_scale: float32 contiguous device tensors [Hkv], or None (1.0): the logits are scale * k_scale[h] * q.k8, the output
    is v_scale[h] * softmax.v8, lse is that of the scaled logits.  Scales must be finite and > 0; they are read on the device only,
    like cache_seqlens, so a captured call follows all three when they are rewritten in place.  quantize_kv_fp8() makes a cache
    and its scales from a 16-bit or fp32 tensor.
    Everything else -- cache_seqlens, causal, rows without a key, return_lse, the workspace (kvcache_workspace_bytes), window (what
    fa_forward_kvcache_fp8_window computes, on kvcache_window_workspace_bytes), sinks and softcap (the sinks take neither scale),
    seqlens_q, the descriptor call -- is fa_forward_kvcache's."""
    return _decode(q, k_cache, v_cache, "k_cache", "v_cache", cache_seqlens, causal, scale, out_dtype, return_lse, workspace, stream,
                   window, scales=(k_scale, v_scale), sinks=sinks, softcap=softcap, seqlens_q=seqlens_q)


def fa_forward_kvcache_paged_fp8(q, k_pool, v_pool, block_table, k_scale=None, v_scale=None, cache_seqlens=None,
                                 causal: bool = False, scale: float | None = None, out_dtype=None, return_lse: bool = False,
                                 workspace=None, stream=None, window: int = 0, sinks=None, softcap: float = 0.0, seqlens_q=None):
    """fa_forward_kvcache_paged against fp8 pools (fa_forward_kvcache_paged_fp8): k_pool/v_pool [num_pages,Hkv,page_size,d]
    torch.float8_e4m3fn, block_table as in fa_forward_kvcache_paged, k_scale / v_scale and everything else as in
    fa_forward_kvcache_fp8.  Workspace: kvcache_paged_workspace_bytes; with a window (fa_forward_kvcache_paged_fp8_window)
    kvcache_paged_window_workspace_bytes.  sinks, softcap, seqlens_q: as in fa_forward_kvcache."""
    return _decode(q, k_pool, v_pool, "k_pool", "v_pool", cache_seqlens, causal, scale, out_dtype, return_lse, workspace, stream,
                   window, paged=True, block_table=block_table, scales=(k_scale, v_scale), sinks=sinks, softcap=softcap, seqlens_q=seqlens_q)


def _state_dtype(dtype):
    import torch
    ids = {torch.float16: capi.STATE_F16, torch.bfloat16: capi.STATE_BF16, torch.float32: capi.STATE_F32}
    if dtype not in ids:
        raise ValueError(f"an attention state is float32, float16 or bfloat16 (got {dtype})")
    return ids[dtype]


def _merge_call(parts, B, H, rows, d, part_dtype, out, lse, tensors, stream):
    """fa_merge_states: parts is a list of (O pointer, lse pointer, stride_b, stride_h), strides in rows; out [B,H,rows,d]
    contiguous, lse [B,H,rows] fp32 or None."""
    import torch
    desc = capi.MergeDesc(parts=parts, R=len(parts), B=B, H=H, rows=rows, d=d, part_dtype=_state_dtype(part_dtype), O=out.data_ptr(),
                          lse=None if lse is None else lse.data_ptr(), out_dtype=_state_dtype(out.dtype), stream=_stream_ptr(stream))
    with torch.cuda.device(_one_device(*tensors)):
        code = capi.lib().fa_merge_states(desc)
    capi.check("fa_merge_states", code)


def fa_merge_states(outs, lses, out_dtype=None, return_lse: bool = True, stream=None):
    """Merge R attention states over disjoint key ranges (fa_merge_states): outs a list of R tensors [B,Hq,Nq,d], all float32 or all
    float16 or all bfloat16, lses a list of R float32 tensors [B,Hq,Nq] -- what R decode calls with return_lse=True return, each
    over its own keys.  1 <= R <= 16, d in {64,128}, contiguous device tensors on one device.
    -> (O [B,Hq,Nq,d] of out_dtype, lse [B,Hq,Nq] float32), or O alone with return_lse=False:
    lse = ln sum_r exp(lse_r), O = sum_r O_r exp(lse_r - lse), evaluated in fp32 against the largest lse_r and rounded once.
    out_dtype: torch.float32 (None), torch.float16 or torch.bfloat16.
    A part with lse_r = -inf (a range without a visible key) is neutral and its O row is never used; if every part is -inf the row is
    O = 0, lse = -inf.  With one part, or one finite part, the result is that part's bits (rounded once if the dtypes differ).
    Sinks are part of the lse of the range they were passed to: pass `sinks` to exactly one of the decode calls.
    One kernel, no workspace, nothing read on the host: a captured call follows parts that are rewritten in place."""
    import torch
    outs, lses = list(outs), list(lses)
    if not 1 <= len(outs) <= capi.MERGE_MAX_PARTS or len(lses) != len(outs):
        raise ValueError(f"outs and lses must be lists of the same length R, 1 <= R <= {capi.MERGE_MAX_PARTS}")
    first = outs[0]
    if not isinstance(first, torch.Tensor) or first.dim() != 4:
        raise ValueError("every out must be a tensor [B,Hq,Nq,d]")
    B, Hq, Nq, d = first.shape
    states = (torch.float32, torch.float16, torch.bfloat16)
    out_dtype = out_dtype or torch.float32
    if out_dtype not in states:
        raise ValueError("out_dtype must be torch.float32, torch.float16 or torch.bfloat16")
    parts = []
    for i, (o, l) in enumerate(zip(outs, lses)):
        if not isinstance(o, torch.Tensor) or o.shape != first.shape or o.dtype != first.dtype:
            raise ValueError(f"outs[{i}] must have the shape and dtype of outs[0] ({tuple(first.shape)}, {first.dtype})")
        if not isinstance(l, torch.Tensor) or l.shape != first.shape[:3]:
            raise ValueError(f"lses[{i}] must be a float32 tensor [B,Hq,Nq] = {tuple(first.shape[:3])}")
        parts.append((_dev_ptr(o, f"outs[{i}]", states), _dev_ptr(l, f"lses[{i}]", (torch.float32,)), Hq * Nq, Nq))
    dev = _one_device(*outs, *lses)
    out = torch.empty(first.shape, dtype=out_dtype, device=dev)
    lse = torch.empty(first.shape[:3], dtype=torch.float32, device=dev) if return_lse else None
    _merge_call(parts, B, Hq, Nq, d, first.dtype, out, lse, outs + lses, stream)
    return (out, lse) if return_lse else out


def _packed_strides(t, name: str):
    """(stride_t, stride_h) in elements of a packed (total, H, d) tensor as it lies; the last dimension must be contiguous"""
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{name} must be contiguous in its last dimension (any token and head strides are taken as they are)")
    # the stride of a dimension of size 1 addresses nothing and may hold anything
    return (t.stride(0) if t.shape[0] > 1 else t.shape[2]), (t.stride(1) if t.shape[1] > 1 else 0)


def fa_forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k=None, causal: bool = False, scale: float | None = None, out_dtype=None,
                      return_lse: bool = False, out=None, stream=None, lse=None, window: int = 0, softcap: float = 0.0, sinks=None):
    """Variable-length packed prefill (fa_forward_varlen, fa_forward_varlen_ex): B sequences of different lengths in one launch.
    q (total_q, Hq, d), k and v (total_k, Hkv, d) fp16/bf16 device tensors, packed along the token axis; d in {64,128};
    Hq = G * Hkv (grouped-query: query head hq reads K/V head hq // G, no expanded copy).  Any token and head strides are accepted as
    long as the last dimension is contiguous (strides multiples of 8 elements, 16-byte aligned storage), so a (H, total, d) tensor
    passed through .transpose(0, 1) is taken as it lies.
    cu_seqlens_q, cu_seqlens_k: int32 device tensors [B+1], read on the device only; sequence b owns the rows [cu[b], cu[b+1]),
    clamped into the tensor.  cu_seqlens_k=None means cu_seqlens_q (self-attention).
    causal: row i of a sequence sees the keys [0, Lk - Lq + 1 + i) -- aligned to the END of the keys, as in fa_forward_kvcache.  A row
    that sees no key is O = 0 and lse = -inf.
    -> o (total_q, Hq, d) of out_dtype (torch.float32, the default, or the input dtype), or (o, lse) with return_lse, lse (Hq, total_q)
    float32 in natural-log units, as fa_merge_states takes it.  Rows that belong to no sequence are NOT written: in a fresh result they
    are uninitialised; pass `out` (and `lse`, which implies return_lse) to keep what they held.
    window: 0 (no window), or W >= 1: row i sees only the keys [max(0, Lk - Lq + 1 + i - W), its upper limit) -- with causal its own
    position and the W - 1 before it, the limits fa_forward_kvcache has.  K/V tiles below a query block's first visible key are not read.
    softcap: 0 (off), or a finite float > 0: every logit s becomes softcap * tanh(s / softcap) before the masks and the softmax.
    sinks: None, or a float32 contiguous device tensor of Hq values: head h gets one extra key with the natural-log logit sinks[h]
    (not scaled, not capped) and a zero V row, which every row of a sequence sees under any mask or window -- lse includes it, and a
    row without a key is O = 0, lse = sinks[h]; -inf: no sink for that head.  Read on the device only.
    window and softcap are host values (baked into a captured call).  With all three unset the call is fa_forward_varlen itself;
    otherwise fa_forward_varlen_ex, whose kernels compute a prompt by the arithmetic fa_forward_kvcache decodes its tokens with.
    One kernel, no workspace, nothing read on the host: a captured call follows vectors that are rewritten in place."""
    import torch
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{name} must be a packed tensor (total, H, d)")
    if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("q, k, v must all be fp16 or all bf16")
    total_q, Hq, d = q.shape
    total_k, Hkv = k.shape[0], k.shape[1]
    if v.shape != k.shape or k.shape[2] != d:
        raise ValueError("k and v must both be (total_k, Hkv, d) with q's d")
    if d not in (64, 128):
        raise ValueError("d must be 64 or 128")
    if total_q <= 0 or total_k <= 0 or Hkv <= 0 or Hq <= 0 or Hq % Hkv != 0:
        raise ValueError("the number of query heads must be a positive multiple of the number of K/V heads, and no tensor empty")
    window = _window(window)
    softcap = _softcap(softcap)
    sink_ptr = _sinks_ptr(sinks, Hq, q.device)
    if cu_seqlens_k is None:
        cu_seqlens_k = cu_seqlens_q
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32:
            raise ValueError(f"{name} must be an int32 tensor (the kernel reads 32-bit entries)")
        if cu.dim() != 1 or cu.numel() < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-d tensor of B+1 entries")
    if cu_seqlens_k.numel() != cu_seqlens_q.numel():
        raise ValueError("cu_seqlens_q and cu_seqlens_k must both have B+1 entries")
    B = cu_seqlens_q.numel() - 1
    (qt, qh), (kt, kh), (vt, vh) = (_packed_strides(t, name) for name, t in (("q", q), ("k", k), ("v", v)))
    for name, t in (("q", q), ("k", k), ("v", v), ("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    out_dt = _out_dt(out_dtype, q.dtype)
    if out is None:
        out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.shape != q.shape or out.dtype != out_dtype:
        raise ValueError("out must be a device tensor of q's shape and of out_dtype")
    if lse is not None:
        if not isinstance(lse, torch.Tensor) or lse.shape != (Hq, total_q):
            raise ValueError("lse must be a float32 tensor (Hq, total_q)")
        _dev_ptr(lse, "lse", (torch.float32,))
        return_lse = True
    elif return_lse:
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=q.device)
    ot, oh = _packed_strides(out, "out")
    desc = capi.VarlenDesc(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=out.data_ptr(), lse=None if lse is None else lse.data_ptr(),
                           cu_seqlens_q=cu_seqlens_q.data_ptr(), cu_seqlens_k=cu_seqlens_k.data_ptr(), B=B, Hkv=Hkv, G=Hq // Hkv, d=d,
                           total_q=total_q, total_k=total_k, q_stride_t=qt, q_stride_h=qh, k_stride_t=kt, k_stride_h=kh, v_stride_t=vt,
                           v_stride_h=vh, o_stride_t=ot, o_stride_h=oh, scale=float(_scale_or_default(scale, d)), causal=int(bool(causal)),
                           in_dtype=_in_dt(q.dtype), out_dtype=out_dt, stream=_stream_ptr(stream))
    plain = window == 0 and softcap == 0.0 and sinks is None   # then the old symbol, as before the options existed
    with torch.cuda.device(_one_device(q, k, v, out, cu_seqlens_q, cu_seqlens_k, lse, sinks)):
        if plain:
            code = capi.lib().fa_forward_varlen(desc)
        else:
            code = capi.lib().fa_forward_varlen_ex(desc, capi.VarlenOpts(sinks=sink_ptr, window=window, softcap=softcap))
    capi.check("fa_forward_varlen" if plain else "fa_forward_varlen_ex", code)
    return (out, lse) if return_lse else out


def fa_forward_varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table=None, causal: bool = False,
                              scale: float | None = None, out_dtype=None, return_lse: bool = False, out=None, stream=None, lse=None,
                              window: int = 0, softcap: float = 0.0, sinks=None):
    """fa_forward_varlen with the keys taken from the KV cache (fa_forward_varlen_kvcache): chunked prefill, prefix caching and a window
    across the cache boundary in one launch.  q (total_q, Hq, d) fp16/bf16 packed along the token axis and cut by cu_seqlens_q (int32
    device [B+1]), exactly as in fa_forward_varlen; d in {64,128}; Hq = G * Hkv.
    k_cache, v_cache: contiguous device tensors of q's dtype: [B,Hkv,Ncap,d], or with block_table (int32 contiguous device tensor
    [B, max_pages]) the pools [num_pages,Hkv,page_size,d], page_size a power of two >= 16; key j of sequence b is then row
    j % page_size of page block_table[b, j // page_size], and the capacity is max_pages * page_size.
    cache_seqlens: int32 contiguous device tensor [B]: the keys of sequence b in the cache, the chunk's own tokens INCLUDED -- the
    lengths after fa_kvcache_append* -- clamped to [0, capacity].  With Lk = cache_seqlens[b] and Lq from cu_seqlens_q, row i sees the
    keys [lo_i, c_i): c_i = Lk, or max(0, Lk - Lq + 1 + i) with causal; lo_i = max(0, Lk - Lq + 1 + i - window) with a window, else 0.
    So append the chunk, then call this with causal=True: row i sees the cached prefix and the chunk up to itself.
    scale, out_dtype, return_lse, out, lse, window, softcap, sinks and the result: as in fa_forward_varlen, whose bits the call returns
    on the same finite keys; the paged form returns the bits of the contiguous form.
    Table, lengths and sinks are read on the device only: one kernel, no workspace, and a captured call follows all of them when they
    are rewritten in place.  Table entries past a sequence's last live page are not read; a live entry outside [0, num_pages) reads
    as a page of zeros; under a window the pages wholly below max(0, Lk - Lq + 1 - window) are not read and may be freed.
    An fp8 cache is fa_forward_varlen_kvcache_fp8's."""
    return _varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, causal, scale, out_dtype, return_lse, out,
                           stream, lse, window, softcap, sinks)


def fa_forward_varlen_kvcache_fp8(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table=None, k_scale=None, v_scale=None,
                                  causal: bool = False, scale: float | None = None, out_dtype=None, return_lse: bool = False, out=None,
                                  stream=None, lse=None, window: int = 0, softcap: float = 0.0, sinks=None):
    """fa_forward_varlen_kvcache against an fp8 cache (fa_forward_varlen_kvcache_fp8): the cache fa_kvcache_append_fp8 / _paged_fp8
    write and the fp8 decode entries read.  k_cache, v_cache: contiguous torch.float8_e4m3fn device tensors (OCP e4m3fn; fnuz, e5m2
    and 16-bit caches are refused), [B,Hkv,Ncap,d] or with block_table the pools [num_pages,Hkv,page_size,d].  q stays fp16/bf16: the
    codes are widened to its type, exactly, on the way into LDS.  k_scale, v_scale: float32 device tensors [Hkv], finite and > 0, or
    None for 1.0, read on the device only: the logits are scale * k_scale[hkv] * q.k8 and O = v_scale[hkv] * softmax.v8; the sinks take
    neither scale, and lse is that of the scaled logits.  Everything else -- lengths, limits, options, what is read and what a captured
    call follows -- as in fa_forward_varlen_kvcache, whose bits the call returns on the widened cache when both scales are None."""
    return _varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, causal, scale, out_dtype, return_lse, out,
                           stream, lse, window, softcap, sinks, scales=(k_scale, v_scale))


def _varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, causal, scale, out_dtype, return_lse, out, stream,
                    lse, window, softcap, sinks, scales=None):
    """The two varlen front ends against the KV cache: scales is None (a 16-bit cache of q's type) or (k_scale, v_scale) of an fp8 one."""
    import torch
    fp8 = scales is not None
    name8 = "fa_forward_varlen_kvcache" + "_fp8" * fp8
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if fp8 and (k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn):   # judged first, as in _decode
        raise ValueError(f"k_cache, v_cache: {_FP8_CACHE} (got {k_cache.dtype}, {v_cache.dtype})")
    if q.dim() != 3:
        raise ValueError("q must be a packed tensor (total_q, Hq, d)")
    if fp8:
        if q.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("q must be fp16 or bf16")
    elif q.dtype not in (torch.float16, torch.bfloat16) or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise ValueError("q, k_cache, v_cache must all be fp16 or all bf16")
    total_q, Hq, d = q.shape
    paged = block_table is not None
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape or k_cache.shape[3] != d:
        raise ValueError("k_cache and v_cache must both be [B,Hkv,Ncap,d], or with block_table [num_pages,Hkv,page_size,d], with q's d")
    Hkv = k_cache.shape[1]
    if d not in (64, 128):
        raise ValueError("d must be 64 or 128")
    if total_q <= 0 or Hkv <= 0 or Hq <= 0 or Hq % Hkv != 0 or k_cache.numel() == 0:
        raise ValueError("the number of query heads must be a positive multiple of the number of K/V heads, and no tensor empty")
    window = _window(window)
    softcap = _softcap(softcap)
    sink_ptr = _sinks_ptr(sinks, Hq, q.device)
    ks_ptr, vs_ptr = _scale_ptrs(scales[0], scales[1], Hkv) if fp8 else (None, None)
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32:
        raise ValueError("cu_seqlens_q must be an int32 tensor (the kernel reads 32-bit entries)")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or not cu_seqlens_q.is_contiguous():
        raise ValueError("cu_seqlens_q must be a contiguous 1-d tensor of B+1 entries")
    B = cu_seqlens_q.numel() - 1
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (B,):
        raise ValueError("cache_seqlens must be an int32 device tensor of B entries")
    qt, qh = _packed_strides(q, "q")
    if paged:
        num_pages, page_size, Ncap = k_cache.shape[0], k_cache.shape[2], 0
        if page_size < 16 or page_size & (page_size - 1):
            raise ValueError("page_size must be a power of two >= 16")
        table_ptr = _table_ptr(block_table, B)
        max_pages = block_table.shape[1]
        if max_pages <= 0:
            raise ValueError("block_table must have at least one column")
    else:
        table_ptr, num_pages, page_size, max_pages, Ncap = None, 0, 0, 0, k_cache.shape[2]
        if k_cache.shape[0] != B:
            raise ValueError(f"k_cache holds {k_cache.shape[0]} sequences, cu_seqlens_q {B}")
    for name, t in (("q", q), ("cu_seqlens_q", cu_seqlens_q)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    cache_dts = (torch.float8_e4m3fn if fp8 else q.dtype,)
    k_ptr, v_ptr = _dev_ptr(k_cache, "k_cache", cache_dts), _dev_ptr(v_cache, "v_cache", cache_dts)
    lens_ptr = _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    out_dt = _out_dt(out_dtype, q.dtype)
    if out is None:
        out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.shape != q.shape or out.dtype != out_dtype:
        raise ValueError("out must be a device tensor of q's shape and of out_dtype")
    if lse is not None:
        if not isinstance(lse, torch.Tensor) or lse.shape != (Hq, total_q):
            raise ValueError("lse must be a float32 tensor (Hq, total_q)")
        _dev_ptr(lse, "lse", (torch.float32,))
        return_lse = True
    elif return_lse:
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=q.device)
    ot, oh = _packed_strides(out, "out")
    desc = capi.VarlenKvcacheDesc(Q=q.data_ptr(), O=out.data_ptr(), lse=None if lse is None else lse.data_ptr(), K=k_ptr, V=v_ptr,
                                  cu_seqlens_q=cu_seqlens_q.data_ptr(), seqlens_k=lens_ptr, block_table=table_ptr, B=B, Hkv=Hkv,
                                  G=Hq // Hkv, d=d, total_q=total_q, Ncap=Ncap, num_pages=num_pages, page_size=page_size,
                                  max_pages=max_pages, q_stride_t=qt, q_stride_h=qh, o_stride_t=ot, o_stride_h=oh,
                                  scale=float(_scale_or_default(scale, d)), causal=int(bool(causal)), in_dtype=_in_dt(q.dtype),
                                  out_dtype=out_dt, sinks=sink_ptr, window=window, softcap=softcap, stream=_stream_ptr(stream))
    with torch.cuda.device(_one_device(q, k_cache, v_cache, out, cu_seqlens_q, cache_seqlens, block_table, lse, sinks, *(scales or ()))):
        if fp8:
            code = capi.lib().fa_forward_varlen_kvcache_fp8(desc, ks_ptr, vs_ptr)
        else:
            code = capi.lib().fa_forward_varlen_kvcache(desc)
    capi.check(name8, code)
    return (out, lse) if return_lse else out


def fa_kvcache_decode_varlen(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=None, block_table=None, causal: bool = False,
                             scale: float | None = None, out_dtype=None, return_lse: bool = False, out=None, workspace=None, stream=None,
                             window=None, softcap: float = 0.0, sinks=None, lse=None, tree_mask=None):
    """Split-KV decode on a token-packed batch (fa_kvcache_decode_varlen): the read half of fa_kvcache_append_varlen for a step whose
    sequences bring few rows each (one token per sequence, speculative tokens, a short chunk beside decode tokens).  It is
    fa_forward_kvcache(seqlens_q=...) -- the split-KV stream with the G heads of a group folded into the rows -- with q, the result and
    lse in the packed layout of fa_forward_varlen_kvcache.
    q: (total_q, Hq, d) fp16/bf16 device tensor, taken as it lies: any token and head strides with a contiguous last dimension (strides
    multiples of 8 elements, 16-byte aligned storage), so the Q view of a fused (total, Hq + 2*Hkv, d) projection buffer, rotated in
    place by the append, goes in without a copy.  d in {64,128}; Hq = G * Hkv.
    cu_seqlens_q: int32 contiguous device tensor [B+1], read on the device only; sequence b owns the tokens [cu[b], cu[b+1]), clamped
    into the tensor as in fa_forward_varlen.  max_seqlen_q: a host int >= 1, the most rows a sequence may have: sequence b has
    n_b = min(cu[b+1] - cu[b], max_seqlen_q) rows, its first n_b tokens.  Grid, split count and workspace follow max_seqlen_q, not the
    vector: size it to the step.
    k_cache, v_cache: [B,Hkv,Ncap,d] of q's dtype, or with block_table (int32 [B, max_pages]) the pools [num_pages,Hkv,page_size,d].
    cache_seqlens: int32 [B], the keys of sequence b in the cache, its own new tokens INCLUDED (the lengths after the append), or None
    (the capacity for all).  With L_b and n_b, row i sees the keys [lo_i, c_i): c_i = L_b, or max(0, L_b - n_b + 1 + i) with causal;
    lo_i = max(0, L_b - n_b + 1 + i - window) with a window, else 0.
    window (None or 0: none), softcap, sinks, scale, out_dtype: as in fa_forward_kvcache.
    -> o (total_q, Hq, d) of out_dtype (torch.float32, the default, or q's dtype), or (o, lse) with return_lse, lse (Hq, total_q)
    float32.  On the live rows the bits are those of fa_forward_kvcache(seqlens_q=n, Nq=max_seqlen_q) on the padded copy of the same
    rows.  Tokens that are no live row of any sequence are NOT written: a fresh result holds O = 0 and lse = -inf there ("no key");
    with `out` (a tensor of q's shape and of out_dtype, any token and head strides) and `lse` (a contiguous float32 (Hq, total_q) tensor,
    which implies return_lse) they keep what they held.  The fills of a fresh result are torch's, on the current stream.
    workspace: optional uint8 device tensor of at least kvcache_decode_varlen_workspace_bytes(...).
    Nothing is read on the host: append_varlen(seqlens_out=lens, q=q) then this call with cu_seqlens_q = cu_seqlens_new and
    cache_seqlens = lens, captured once, serves every step of the same total_q; the replay follows the vectors, the table and the sinks.
    tree_mask (fa_kvcache_decode_varlen_ex): None, or an int64 tensor (total_q,) on q's device, one word per token row, for the verify
    step of tree speculation.  It takes the causal triangle's place (causal must be True, max_seqlen_q <= 64): with base = L_b - n_b,
    row i sees every key below base and key base + j iff bit j of (tree_mask[s_b + i] & low n_b bits) | 1 << i is set; under a window
    lo_i = max(0, base + popcount - window).  tree_from_parents() makes the words from parent indices; with (1 << (i + 1)) - 1 the
    result has the bits of causal=True.  Words of tokens of no sequence are not read; a captured call follows the tensor in place.
    An fp8 cache is fa_kvcache_decode_varlen_fp8's."""
    return _decode_varlen(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, scale, out_dtype,
                          return_lse, out, workspace, stream, window, softcap, sinks, lse, tree_mask=tree_mask)


def fa_kvcache_decode_varlen_fp8(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=None, block_table=None, k_scale=None,
                                 v_scale=None, causal: bool = False, scale: float | None = None, out_dtype=None, return_lse: bool = False,
                                 out=None, workspace=None, stream=None, window=None, softcap: float = 0.0, sinks=None, lse=None,
                                 tree_mask=None):
    """fa_kvcache_decode_varlen against an fp8 cache: k_cache, v_cache (or the pools) contiguous torch.float8_e4m3fn (OCP e4m3fn; fnuz,
    e5m2 and 16-bit caches are refused), k_scale, v_scale float32 [Hkv] or None (1.0), read on the device only; scales, logits and lse
    as in fa_forward_kvcache_fp8, everything else as in fa_kvcache_decode_varlen, tree_mask included."""
    return _decode_varlen(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, scale, out_dtype,
                          return_lse, out, workspace, stream, window, softcap, sinks, lse, scales=(k_scale, v_scale), tree_mask=tree_mask)


def fa_kvcache_attend_varlen(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table=None, split_rows: int = 128,
                             scale: float | None = None, out_dtype=None, return_lse: bool = False, out=None, workspace=None, window=None,
                             softcap: float = 0.0, sinks=None, parts: int = 3, stream=None, lse=None):
    """The mixed prefill + decode step (fa_kvcache_attend_varlen): one causal attention call for a token-packed batch that holds prompt
    chunks beside one-token decodes, each sequence routed on the device to the kernel that suits its row count.  With span_b the rows
    cu_seqlens_q gives sequence b (clamped into the tensor as in fa_forward_varlen): 1 <= span_b <= split_rows runs on the split-KV
    stream and returns the bits of fa_kvcache_decode_varlen(..., max_seqlen_q=split_rows, causal=True); span_b > split_rows runs on the
    tiled kernel and returns the bits of fa_forward_varlen_kvcache(..., causal=True).  Every token of every sequence is computed --
    nothing is cut at split_rows -- and row i sees the keys [lo_i, c_i) with c_i = max(0, L_b - span_b + 1 + i),
    lo_i = max(0, L_b - span_b + 1 + i - window) under a window, else 0: append the step, then call this.
    q, k_cache, v_cache, cu_seqlens_q, block_table, window, softcap, sinks, scale, out_dtype, out, lse: as in fa_kvcache_decode_varlen.
    cache_seqlens: int32 [B], required: the keys of sequence b, its new tokens INCLUDED.  split_rows: a host int >= 1 (default 128, the
    measured crossover of the two entries); the split count, the grid of the split-KV half and the workspace follow it, so
    kvcache_decode_varlen_workspace_bytes(B, Hkv, G, max_seqlen_q=split_rows, ...) sizes `workspace`.
    parts: 3 (both halves, the default), 1 (only the sequences of at most split_rows rows are computed and written) or 2 (only the
    longer ones); the other class keeps its rows in `out` and `lse` and nothing of it is read -- for a caller who runs the
    bandwidth-bound half and the compute-bound half on two streams.
    -> o (total_q, Hq, d), or (o, lse) with return_lse; a fresh o holds zeros and a fresh lse -inf where nothing was written.
    Nothing is read on the host: captured once, the call follows cu_seqlens_q, cache_seqlens, the table and the sinks rewritten in
    place, sequences that change class included.  An fp8 cache is fa_kvcache_attend_varlen_fp8's."""
    return _decode_varlen(q, k_cache, v_cache, cu_seqlens_q, split_rows, cache_seqlens, block_table, True, scale, out_dtype, return_lse,
                          out, workspace, stream, window, softcap, sinks, lse, attend=True, parts=parts)


def fa_kvcache_attend_varlen_fp8(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table=None, k_scale=None, v_scale=None,
                                 split_rows: int = 128, scale: float | None = None, out_dtype=None, return_lse: bool = False, out=None,
                                 workspace=None, window=None, softcap: float = 0.0, sinks=None, parts: int = 3, stream=None, lse=None):
    """fa_kvcache_attend_varlen against an fp8 cache: k_cache, v_cache (or the pools) contiguous torch.float8_e4m3fn, k_scale, v_scale
    float32 [Hkv] or None (1.0), read on the device only.  The short sequences return the bits of fa_kvcache_decode_varlen_fp8, the long
    ones those of fa_forward_varlen_kvcache_fp8; everything else as in fa_kvcache_attend_varlen."""
    return _decode_varlen(q, k_cache, v_cache, cu_seqlens_q, split_rows, cache_seqlens, block_table, True, scale, out_dtype, return_lse,
                          out, workspace, stream, window, softcap, sinks, lse, scales=(k_scale, v_scale), attend=True, parts=parts)


def kvcache_decode_varlen_workspace_bytes(B: int, Hkv: int, G: int, max_seqlen_q: int, d: int, Ncap: int = 0, max_pages: int = 0,
                                          page_size: int = 0, window: int = 0) -> int:
    """Workspace of fa_kvcache_decode_varlen and _fp8: a contiguous cache gives Ncap, a paged one max_pages and page_size.  It is what
    the padded decode entry needs with Nq = max_seqlen_q (kvcache_window_workspace_bytes, kvcache_paged_window_workspace_bytes)."""
    desc = capi.new_desc(capi.KvDecodeVarlenDesc)
    capi.fill(desc, block_table=1 if max_pages or page_size else None, B=B, Hkv=Hkv, G=G, d=d, max_q=max_seqlen_q, Ncap=Ncap,
              max_pages=max_pages, page_size=page_size, window=window)
    return int(capi.lib().fa_kvcache_decode_varlen_workspace_bytes(desc))


def _decode_varlen(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, scale, out_dtype, return_lse,
                   out, workspace, stream, window, softcap, sinks, lse, scales=None, tree_mask=None, attend=False, parts=3):
    """The two packed decode front ends: scales is None (a 16-bit cache of q's type) or (k_scale, v_scale) of an fp8 one; tree_mask is
    None (fa_kvcache_decode_varlen) or the words of fa_kvcache_decode_varlen_ex.  Shapes and dtypes are judged before anything needs a
    device.  attend: the call is fa_kvcache_attend_varlen_part(desc, parts) on the same descriptor, max_seqlen_q its threshold."""
    import torch
    fp8 = scales is not None
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if fp8 and (k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn):   # judged first, as in _decode
        raise ValueError(f"k_cache, v_cache: {_FP8_CACHE} (got {k_cache.dtype}, {v_cache.dtype})")
    if q.dim() != 3:
        raise ValueError("q must be a packed tensor (total_q, Hq, d)")
    dts = (torch.float16, torch.bfloat16)
    if fp8:
        if q.dtype not in dts:
            raise ValueError("q must be fp16 or bf16")
    elif q.dtype not in dts or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise ValueError("q, k_cache, v_cache must all be fp16 or all bf16")
    total_q, Hq, d = q.shape
    paged = block_table is not None
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape or k_cache.shape[3] != d:
        raise ValueError("k_cache and v_cache must both be [B,Hkv,Ncap,d], or with block_table [num_pages,Hkv,page_size,d], with q's d")
    Hkv = k_cache.shape[1]
    if d not in (64, 128):
        raise ValueError("d must be 64 or 128")
    if total_q <= 0 or Hkv <= 0 or Hq <= 0 or Hq % Hkv != 0 or k_cache.numel() == 0:
        raise ValueError("the number of query heads must be a positive multiple of the number of K/V heads, and no tensor empty")
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 1:
        raise ValueError("split_rows must be an int >= 1: the most rows of a sequence that runs on the split-KV stream"
                         if attend else "max_seqlen_q must be an int >= 1: the most rows a sequence may have")
    if attend:
        if type(parts) is not int or parts not in (1, 2, 3):
            raise ValueError("parts must be 1 (the split-KV half), 2 (the tiled half) or 3 (both)")
        if cache_seqlens is None:
            raise ValueError("cache_seqlens must be an int32 device tensor of B entries (the mixed step has no default lengths)")
    if tree_mask is not None:
        if not isinstance(tree_mask, torch.Tensor) or tree_mask.dtype != torch.int64:
            raise ValueError("tree_mask must be an int64 tensor: one 64-bit word per token row")
        if tree_mask.shape != (total_q,) or not tree_mask.is_contiguous():
            raise ValueError("tree_mask must be a contiguous tensor (total_q,)")
        if tree_mask.device != q.device:
            raise ValueError("tree_mask must live on q's device")
        if not causal:
            raise ValueError("tree_mask takes the causal triangle's place: causal must be True")
        if max_seqlen_q > 64:
            raise ValueError("tree_mask holds one bit per token of a sequence's step: max_seqlen_q must be <= 64")
    window = _window(0 if window is None else window)
    softcap = _softcap(softcap)
    sink_ptr = _sinks_ptr(sinks, Hq, q.device)
    ks_ptr, vs_ptr = _scale_ptrs(scales[0], scales[1], Hkv) if fp8 else (None, None)
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32:
        raise ValueError("cu_seqlens_q must be an int32 tensor (the kernel reads 32-bit entries)")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or not cu_seqlens_q.is_contiguous():
        raise ValueError("cu_seqlens_q must be a contiguous 1-d tensor of B+1 entries")
    B = cu_seqlens_q.numel() - 1
    if cache_seqlens is not None and (not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32
                                      or cache_seqlens.shape != (B,)):
        raise ValueError("cache_seqlens must be an int32 device tensor of B entries")
    qt, qh = _packed_strides(q, "q")
    if paged:
        num_pages, page_size, Ncap = k_cache.shape[0], k_cache.shape[2], 0
        if page_size < 16 or page_size & (page_size - 1):
            raise ValueError("page_size must be a power of two >= 16")
        table_ptr = _table_ptr(block_table, B)
        max_pages = block_table.shape[1]
        if max_pages <= 0:
            raise ValueError("block_table must have at least one column")
    else:
        table_ptr, num_pages, page_size, max_pages, Ncap = None, 0, 0, 0, k_cache.shape[2]
        if k_cache.shape[0] != B:
            raise ValueError(f"k_cache holds {k_cache.shape[0]} sequences, cu_seqlens_q {B}")
    for name, t in (("q", q), ("cu_seqlens_q", cu_seqlens_q)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    cache_dts = (torch.float8_e4m3fn if fp8 else q.dtype,)
    k_ptr, v_ptr = _dev_ptr(k_cache, "k_cache", cache_dts), _dev_ptr(v_cache, "v_cache", cache_dts)
    lens_ptr = None if cache_seqlens is None else _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    out_dt = _out_dt(out_dtype, q.dtype)
    if out is None:   # tokens of no sequence then read as "no key"
        out = torch.zeros(q.shape, dtype=out_dtype, device=q.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.shape != q.shape or out.dtype != out_dtype:
        raise ValueError("out must be a device tensor of q's shape and of out_dtype")
    if lse is not None:
        if not isinstance(lse, torch.Tensor) or lse.shape != (Hq, total_q):
            raise ValueError("lse must be a float32 tensor (Hq, total_q)")
        _dev_ptr(lse, "lse", (torch.float32,))
        return_lse = True
    elif return_lse:
        lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    ot, oh = _packed_strides(out, "out")
    G = Hq // Hkv
    if workspace is None:
        need = kvcache_decode_varlen_workspace_bytes(B, Hkv, G, max_seqlen_q, d, Ncap, max_pages, page_size, window)
        if need:
            workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_ptr, ws_len = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    desc = capi.new_desc(capi.KvDecodeVarlenDesc)
    capi.fill(
        desc, Q=q.data_ptr(), O=out.data_ptr(), lse=None if lse is None else lse.data_ptr(), K=k_ptr, V=v_ptr,
        cu_seqlens_q=cu_seqlens_q.data_ptr(), seqlens_k=lens_ptr, block_table=table_ptr, k_scale=ks_ptr, v_scale=vs_ptr, sinks=sink_ptr,
        kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT, B=B, Hkv=Hkv, G=G, d=d, total_q=total_q, max_q=max_seqlen_q, Ncap=Ncap,
        num_pages=num_pages, page_size=page_size, max_pages=max_pages, q_stride_t=qt, q_stride_h=qh, o_stride_t=ot, o_stride_h=oh,
        scale=float(_scale_or_default(scale, d)), causal=int(bool(causal)), window=window, softcap=softcap, in_dtype=_in_dt(q.dtype),
        out_dtype=out_dt, workspace=ws_ptr, workspace_bytes=ws_len, stream=_stream_ptr(stream))
    with torch.cuda.device(_one_device(q, k_cache, v_cache, out, cu_seqlens_q, cache_seqlens, block_table, lse, sinks, workspace,
                                       tree_mask, *(scales or ()))):
        if attend:
            code = capi.lib().fa_kvcache_attend_varlen_part(desc, parts)
        elif tree_mask is None:
            code = capi.lib().fa_kvcache_decode_varlen(desc)
        else:
            opts = capi.new_desc(capi.KvDecodeTreeOpts)
            opts.tree_mask = tree_mask.data_ptr()
            code = capi.lib().fa_kvcache_decode_varlen_ex(desc, opts)
    capi.check("fa_kvcache_attend_varlen_part" if attend else
               "fa_kvcache_decode_varlen" if tree_mask is None else "fa_kvcache_decode_varlen_ex", code)
    return (out, lse) if return_lse else out


def fa_forward_kvcache_shared_prefix(q, k_prefix, v_prefix, k_cache, v_cache, prefix_len=None, cache_seqlens=None, block_table=None,
                                     k_scale=None, v_scale=None, causal: bool = False, scale: float | None = None, out_dtype=None,
                                     return_lse: bool = False, sinks=None, softcap: float = 0.0, stream=None):
    """Decode for B sequences that share one prefix: sequence b holds the keys of the prefix [0, P) followed by its own [0, L_b).
    q [B,Hq,Nq,d] fp16/bf16; k_prefix, v_prefix [1,Hkv,Pcap,d], one copy for the whole batch; the suffix is k_cache, v_cache
    [B,Hkv,Ncap,d] or, with block_table [B,max_pages], pools [num_pages,Hkv,page_size,d].  Suffix and prefix have ONE element type:
    q's 16-bit type, or torch.float8_e4m3fn with k_scale, v_scale ([Hkv] float32 or None) that apply to both.
    prefix_len: int32 device tensor [1], P = its value clamped to [0, Pcap], or None (P = Pcap).  cache_seqlens: as in
    fa_forward_kvcache.  Both are read on the device only.
    causal: the mask is aligned to the end of the suffix, as in fa_forward_kvcache -- row i sees the suffix keys
    [0, L_b - Nq + 1 + i) -- and every row sees the whole prefix.  sinks, softcap, scale, out_dtype, return_lse: as there; the sinks
    count once.
    The batch is folded into the rows of ONE stream over the prefix, as the G heads of a group are folded everywhere in the decode
    family, so the prefix K/V is read once and not B times.  Three launches and one small copy: q permuted to [1,Hkv*(B*G),Nq,d] (the
    copy) and fa_forward_kvcache on the prefix with B = 1 and G' = B*G; the suffix's own decode entry; fa_merge_states over the two
    (fp32) results, the prefix part read in place through its [Hkv,B,G*Nq] strides.  Workspaces are allocated here, sized by
    kvcache_workspace_bytes(1, Hkv, B*G, Nq, Pcap, d) and the suffix form's function.  The whole call can be captured into one graph
    (after a warm-up call), and the replay follows prefix_len, cache_seqlens, block_table, the scales and the sinks.
    With P = 0 the result is the plain entry's, bit for bit; a sequence with L_b = 0 gets the prefix part's rows.
    A short prefix does not pay for the copy and the two extra launches (DESIGN.md 7.11 has the measured crossover): below it,
    keep the prefix in every sequence's own cache and call fa_forward_kvcache.
    `window` and `seqlens_q` are NOT keywords of this function: a window would cross the boundary between prefix and suffix, and a
    dead row's q would reach the prefix decode.  Not supported either: a prefix of another element type than the suffix, a paged
    prefix, more than one prefix level (fa_merge_states takes 16 parts; compose them yourself).
    stream: a torch.cuda.Stream, or None for the current one (the permute copy and the allocations are torch's)."""
    import contextlib
    import torch
    paged = block_table is not None
    dts = (torch.float16, torch.bfloat16)
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or q.shape[3] != k_cache.shape[3]:
        raise ValueError("q must be [B,Hq,Nq,d] and k_cache, v_cache " + ("[num_pages,Hkv,page_size,d]" if paged else "[B,Hkv,Ncap,d]"))
    B, Hq, Nq, d = q.shape
    Hkv = k_cache.shape[1]
    if k_prefix.dim() != 4 or v_prefix.shape != k_prefix.shape or k_prefix.shape[0] != 1 or k_prefix.shape[1] != Hkv \
            or k_prefix.shape[3] != d or k_prefix.shape[2] < 1:
        raise ValueError(f"k_prefix, v_prefix must be [1,Hkv,Pcap,d] = [1,{Hkv},Pcap,{d}]: one prefix for the whole batch")
    if k_prefix.dtype != k_cache.dtype or v_prefix.dtype != v_cache.dtype:
        raise ValueError(f"the prefix must have the suffix's element type ({k_cache.dtype}; got {k_prefix.dtype}, {v_prefix.dtype})")
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError("k_scale, v_scale belong to an fp8 cache (torch.float8_e4m3fn)")
    if Hkv == 0 or Hq % Hkv != 0:
        raise ValueError("the number of query heads must be a multiple of the number of K/V heads")
    G = Hq // Hkv
    if prefix_len is not None and (not isinstance(prefix_len, torch.Tensor) or prefix_len.dim() != 1 or prefix_len.shape[0] != 1):
        raise ValueError("prefix_len must be an int32 device tensor of shape [1]")
    _dev_ptr(q, "q", dts)
    out_dtype = out_dtype or torch.float32
    _out_dt(out_dtype, q.dtype)
    if isinstance(stream, torch.cuda.Stream):
        on_stream = torch.cuda.stream(stream)
    elif stream is None:
        on_stream = contextlib.nullcontext()
    else:
        raise ValueError("stream must be a torch.cuda.Stream or None: the permute copy is torch's")
    scales = (k_scale, v_scale) if fp8 else None
    with on_stream:
        # row (hkv, b*G*Nq + g*Nq + i) of the folded stream is row (b, hkv*G + g, i) of q
        qp = q.view(B, Hkv, G, Nq, d).permute(1, 0, 2, 3, 4).reshape(1, Hkv * B * G, Nq, d).contiguous()
        o_p, lse_p = _decode(qp, k_prefix, v_prefix, "k_prefix", "v_prefix", prefix_len, False, scale, torch.float32, True, None, stream,
                             0, scales=scales, softcap=softcap)
        o_s, lse_s = _decode(q, k_cache, v_cache, "k_pool" if paged else "k_cache", "v_pool" if paged else "v_cache", cache_seqlens,
                             causal, scale, torch.float32, True, None, stream, 0, paged=paged, block_table=block_table, scales=scales,
                             sinks=sinks, softcap=softcap)
        out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
        lse = torch.empty((B, Hq, Nq), dtype=torch.float32, device=q.device) if return_lse else None
        rows = G * Nq
        parts = [(o_p.data_ptr(), lse_p.data_ptr(), rows, B * rows), (o_s.data_ptr(), lse_s.data_ptr(), Hkv * rows, rows)]
        _merge_call(parts, B, Hkv, rows, d, torch.float32, out, lse, (o_p, o_s), stream)
    return (out, lse) if return_lse else out


FP8_E4M3_MAX = 448.0   # largest finite e4m3fn value


def quantize_kv_fp8(x, scale=None):
    """x [*, Hkv, N, d] (head axis at dim 1: a cache [B,Hkv,Ncap,d] or a pool [num_pages,Hkv,page_size,d]), any float type, CPU or
    GPU -> (x8 torch.float8_e4m3fn of x's shape, scale float32 [Hkv]) with x ~= x8 * scale[h].
    scale[h] = amax over head h / 448 (1.0 for a head of zeros), so each head's largest magnitude lands on +-448; or the given
    `scale` (float32 [Hkv], finite and > 0: scales calibrated elsewhere), returned as it is.  The quotient is clamped to +-448
    before the conversion: torch's conversion to float8_e4m3fn does not saturate (a value that rounds past 448 becomes NaN)."""
    import torch
    if x.dim() != 4:
        raise ValueError("x must be [*, Hkv, N, d]")
    xf = x.float()
    if scale is None:
        amax = xf.abs().amax(dim=(0, 2, 3))
        scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    elif scale.shape != (x.shape[1],) or scale.dtype != torch.float32 or scale.device != x.device:
        raise ValueError("scale must be a float32 tensor of shape [Hkv] on x's device")
    x8 = (xf / scale.view(1, -1, 1, 1)).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return x8, scale.contiguous()


def _append(k_new, v_new, k_dst, v_dst, what, cache_seqlens, seqlens_out, stream, rope, seqlens_new, paged=False, block_table=None,
            scales=None):
    """The four append front ends: k_dst, v_dst (named `what` in messages) are a cache [B,Hkv,Ncap,d] or, with `paged`, a pool
    [num_pages,Hkv,page_size,d] behind block_table; scales is None (a 16-bit cache) or (k_scale, v_scale) of an fp8 one; rope is
    (q, q_out, rotary_cos, rotary_sin, rotary_interleaved).  Every call is fa_kvcache_append_ex, whose descriptor names each field;
    without seqlens_new that IS the flat entry fa_kvcache_append + _paged + _fp8 + _rope of the same layout (include/fa_mi355.h)."""
    import torch
    fp8 = scales is not None
    if k_dst.dim() != 4 or v_dst.shape != k_dst.shape or k_new.dim() != 4 or (not paged and k_new.shape[0] != k_dst.shape[0]):
        raise ValueError(f"k_new, v_new must be [B,Hkv,Nnew,d] and {what} " + ("[num_pages,Hkv,page_size,d]" if paged else "[B,Hkv,Ncap,d]"))
    if fp8 and (k_dst.dtype != torch.float8_e4m3fn or v_dst.dtype != torch.float8_e4m3fn):   # judged first, as in the decode front end
        raise ValueError(f"{what}: {_FP8_CACHE} (got {k_dst.dtype}, {v_dst.dtype})")
    table_ptr = _table_ptr(block_table, k_new.shape[0]) if paged else None
    ks_ptr, vs_ptr = _scale_ptrs(scales[0], scales[1], k_new.shape[1]) if fp8 else (None, None)
    if v_new.shape != k_new.shape or k_new.shape[1] != k_dst.shape[1] or k_new.shape[3] != k_dst.shape[3]:
        raise ValueError(f"k_new, v_new must be [B,Hkv,Nnew,d] with the Hkv and d of {what}")
    B, Hkv, Nnew, d = k_new.shape
    dts = (torch.float16, torch.bfloat16)
    if k_new.dtype not in dts or v_new.dtype != k_new.dtype:
        raise ValueError("k_new, v_new must both be fp16 or both bf16")
    if not fp8 and (k_dst.dtype != k_new.dtype or v_dst.dtype != k_new.dtype):
        raise ValueError(f"{what} must have the dtype of k_new ({k_new.dtype}; got {k_dst.dtype}, {v_dst.dtype}); an fp8 cache "
                         "goes through fa_kvcache_append_fp8 / fa_kvcache_append_paged_fp8")
    cache_dts = (torch.float8_e4m3fn,) if fp8 else dts
    rot = _rope_shapes(k_new, *rope)
    len_ptrs = []
    for name, t in (("cache_seqlens", cache_seqlens), ("seqlens_out", seqlens_out)):
        if t is None:
            len_ptrs.append(None)
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] != B:
            raise ValueError(f"{name} must be an int32 device tensor of shape [B]")
        len_ptrs.append(_dev_ptr(t, name, (torch.int32,)))
    knew_ptr, vnew_ptr = _dev_ptr(k_new, "k_new", dts), _dev_ptr(v_new, "v_new", dts)
    k_ptr, v_ptr = _dev_ptr(k_dst, "k cache", cache_dts), _dev_ptr(v_dst, "v cache", cache_dts)
    rope_fields, rope_tensors = {}, ()   # without rotary_cos the rotary fields stay as new_desc leaves them: 0 and NULL
    if rot is not None:
        q, q_out, cos, sin, (G, rot_dim, max_pos, interleaved) = rot
        q_ptr, qout_ptr = (None, None) if q is None else (_dev_ptr(q, "q", dts), _dev_ptr(q_out, "q_out", dts))
        rope_fields = dict(Q=q_ptr, Qout=qout_ptr, rope_cos=_dev_ptr(cos, "rotary_cos", (torch.float32,)),
                           rope_sin=_dev_ptr(sin, "rotary_sin", (torch.float32,)), G=G, rot_dim=rot_dim, max_pos=max_pos,
                           interleaved=interleaved)
        rope_tensors = (q, q_out, cos, sin)
    cnt_ptr = _counts_ptr(seqlens_new, "seqlens_new", B, k_new.device)
    # a cache has Ncap, a pool (num_pages, page_size, max_pages); the fields of the other layout are 0
    Ncap, num_pages, page_size, max_pages = (0, k_dst.shape[0], k_dst.shape[2], block_table.shape[1]) if paged else (k_dst.shape[2], 0, 0, 0)
    desc = capi.new_desc(capi.KvAppendDesc)
    capi.fill(
        desc, Knew=knew_ptr, Vnew=vnew_ptr, K=k_ptr, V=v_ptr, seqlens_k=len_ptrs[0], seqlens_out=len_ptrs[1], seqlens_new=cnt_ptr,
        block_table=table_ptr, k_scale=ks_ptr, v_scale=vs_ptr, kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT, B=B, Hkv=Hkv,
        Nnew=Nnew, d=d, Ncap=Ncap, num_pages=num_pages, page_size=page_size, max_pages=max_pages, dtype=_in_dt(k_new.dtype),
        stream=_stream_ptr(stream), **rope_fields)
    with torch.cuda.device(_one_device(k_new, v_new, k_dst, v_dst, block_table, *(scales or ()), cache_seqlens, seqlens_out, *rope_tensors,
                                       seqlens_new)):
        code = capi.lib().fa_kvcache_append_ex(desc)
    capi.check("fa_kvcache_append_ex", code)


def _rope_shapes(k_new, q, q_out, cos, sin, interleaved):
    """The rotary keywords of the append front ends against k_new [B,Hkv,Nnew,d], by shape and dtype alone (nothing here needs a
    device).  -> None without rotary_cos, else (q, q_out or q, cos, sin, (G, rot_dim, max_pos, interleaved))"""
    import torch
    if cos is None:
        if q is not None or q_out is not None or sin is not None:
            raise ValueError("q, q_out and rotary_sin are arguments of the rotary append: they need rotary_cos")
        return None
    B, Hkv, Nnew, d = k_new.shape
    max_pos, rot_dim = _rope_tables(cos, sin, d)
    G = 1
    if q is None:
        if q_out is not None:
            raise ValueError("q_out needs q")
    else:
        if not isinstance(q, torch.Tensor) or q.dim() != 4 or q.shape[0] != B or q.shape[2] != Nnew or q.shape[3] != d \
                or q.shape[1] % Hkv != 0 or q.shape[1] == 0 or q.dtype != k_new.dtype:
            raise ValueError(f"q must be [B,Hq,Nnew,d] = [{B},Hq,{Nnew},{d}] with Hq a multiple of Hkv = {Hkv}, of k_new's dtype")
        G = q.shape[1] // Hkv
        if q_out is None:
            q_out = q   # in place
        elif not isinstance(q_out, torch.Tensor) or q_out.shape != q.shape or q_out.dtype != q.dtype:
            raise ValueError("q_out must have q's shape and dtype")
    return q, q_out, cos, sin, (G, rot_dim, max_pos, 1 if interleaved else 0)


def _rope_tables(cos, sin, d):
    """rotary_cos, rotary_sin of an append against rows of d elements, by shape and dtype alone -> (max_pos, rot_dim)"""
    import torch
    for name, t in (("rotary_cos", cos), ("rotary_sin", sin)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 device tensor of shape [max_pos, rot_dim/2]")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if sin.shape != cos.shape:
        raise ValueError(f"rotary_cos and rotary_sin must have one shape (got {tuple(cos.shape)}, {tuple(sin.shape)})")
    max_pos, rot_dim = cos.shape[0], 2 * cos.shape[1]
    if max_pos < 1 or rot_dim % 16 != 0 or not 16 <= rot_dim <= d:
        raise ValueError(f"rotary_cos must be [max_pos >= 1, rot_dim/2] with rot_dim a multiple of 16 in [16, d = {d}] (got "
                         f"{tuple(cos.shape)})")
    return max_pos, rot_dim


def _scale_ptrs(k_scale, v_scale, Hkv):
    import torch
    out = []
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is None:
            out.append(None)
            continue
        if not isinstance(s, torch.Tensor) or s.dim() != 1 or s.shape[0] != Hkv or s.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 device tensor of shape [Hkv] = [{Hkv}]")
        out.append(_dev_ptr(s, name, (torch.float32,)))
    return out


def _table_ptr(block_table, B):
    import torch
    if not isinstance(block_table, torch.Tensor) or block_table.dim() != 2 or block_table.shape[0] != B:
        raise ValueError("block_table must be an int32 device tensor of shape [B, max_pages]")
    return _dev_ptr(block_table, "block_table", (torch.int32,))


def fa_kvcache_append(k_new, v_new, k_cache, v_cache, cache_seqlens=None, seqlens_out=None, stream=None, *, q=None, q_out=None,
                      rotary_cos=None, rotary_sin=None, rotary_interleaved=False, seqlens_new=None) -> None:
    """Write k_new/v_new [B,Hkv,Nnew,d] behind each sequence's length into k_cache/v_cache [B,Hkv,Ncap,d] (fa_kvcache_append): fp16 or
    bf16 device tensors of ONE dtype, d in {64,128}.  Token t of sequence b goes to row L_b + t, L_b = cache_seqlens[b] clamped to
    [0, Ncap]; a token at or past Ncap is dropped; nothing else in the cache changes.  The caches are mutated, None is returned.
    cache_seqlens: int32 contiguous device tensor [B], or None: every sequence is EMPTY (a prefill into a fresh cache) -- not "full",
    which is what None means to fa_forward_kvcache.
    seqlens_out: int32 contiguous device tensor [B] that receives min(L_b + Nnew, Ncap), or None (the caller updates the lengths).  It
    may be cache_seqlens itself (in place) or a tensor that does not overlap it.
    Lengths are read on the device only: append(seqlens_out=lens) followed by fa_forward_kvcache(lens), captured once into a graph,
    serves every step of a growing cache.
    rotary_cos, rotary_sin: float32 contiguous device tensors [max_pos, rot_dim/2] (rot_dim a multiple of 16 in [16, d]), or None.  With
    them the call is what fa_kvcache_append_rope computes: K is rotated at its position p = L_b + t (table row min(p, max_pos - 1)) on its way into
    the cache, elements [rot_dim, d) pass through, V is written as without them.  rotary_interleaved: False pairs (x[i], x[i+rot_dim/2])
    (NeoX / HF), True pairs (x[2i], x[2i+1]) (GPT-J).  The arithmetic is stepwise fp32 without fused multiply-add (include/fa_mi355.h).
    q: [B,Hq,Nnew,d] of k_new's dtype, Hq a multiple of Hkv, or None: rotated by the same positions in the same launch, into q_out
    (same shape and dtype, not overlapping q) or, with q_out=None, in place.  Without rotary_cos, q and q_out must be None.
    seqlens_new: None, or an int32 contiguous device tensor [B] that does not overlap seqlens_out: Nnew is then the PADDED token count,
    sequence b appends its first m_b = min(max(seqlens_new[b], 0), Nnew) tokens and grows by m_b; a token t >= m_b is not written (no
    table entry is read for it) and its q row reaches q_out unchanged.  Read on the device only.
    fa_forward_kvcache(seqlens_q=the same tensor) is its read half.
    The C call is always the descriptor entry fa_kvcache_append_ex; without seqlens_new it is, byte for byte, the flat entry of the
    form (fa_kvcache_append, fa_kvcache_append_rope)."""
    _append(k_new, v_new, k_cache, v_cache, "k_cache, v_cache", cache_seqlens, seqlens_out, stream,
            (q, q_out, rotary_cos, rotary_sin, rotary_interleaved), seqlens_new)


def fa_kvcache_append_paged(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens=None, seqlens_out=None, stream=None, *, q=None,
                            q_out=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, seqlens_new=None) -> None:
    """fa_kvcache_append into a paged cache (fa_kvcache_append_paged): k_pool/v_pool [num_pages,Hkv,page_size,d] of k_new's dtype,
    block_table int32 [B, max_pages] as in fa_forward_kvcache_paged; position p is row p % page_size of page
    block_table[b, p // page_size], the capacity is max_pages * page_size.  A table entry outside [0, num_pages) drops the tokens of
    that page; entries of pages that receive no token are not read.  The pages a sequence appends into must be its own: a page shared
    between sequences may only be written by the caller's copy-on-write (not checked).
    q, q_out, rotary_cos, rotary_sin, rotary_interleaved: as in fa_kvcache_append (fa_kvcache_append_paged_rope); the q row of a
    dropped token is still rotated.  seqlens_new: as in fa_kvcache_append."""
    _append(k_new, v_new, k_pool, v_pool, "k_pool, v_pool", cache_seqlens, seqlens_out, stream,
            (q, q_out, rotary_cos, rotary_sin, rotary_interleaved), seqlens_new, paged=True, block_table=block_table)


def fa_kvcache_append_fp8(k_new, v_new, k_cache, v_cache, k_scale=None, v_scale=None, cache_seqlens=None, seqlens_out=None,
                          stream=None, *, q=None, q_out=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, seqlens_new=None) -> None:
    """fa_kvcache_append into an fp8 cache (fa_kvcache_append_fp8): k_new/v_new fp16 or bf16, k_cache/v_cache [B,Hkv,Ncap,d]
    torch.float8_e4m3fn (fnuz and e5m2 are refused).  The stored code is quantize_kv_fp8(x, scale) bit for bit: x / scale[h] in fp32,
    clamped to +-448, rounded to nearest even; +-inf becomes +-448, NaN a NaN code.
    k_scale, v_scale: float32 contiguous device tensors [Hkv], finite and > 0, or None (1.0); read on the device only.
    q, q_out, rotary_cos, rotary_sin, rotary_interleaved: as in fa_kvcache_append (fa_kvcache_append_fp8_rope).  The fp32 rotated K is
    quantised directly, without a 16-bit rounding in between; q stays 16 bit.  seqlens_new: as in fa_kvcache_append."""
    _append(k_new, v_new, k_cache, v_cache, "k_cache, v_cache", cache_seqlens, seqlens_out, stream,
            (q, q_out, rotary_cos, rotary_sin, rotary_interleaved), seqlens_new, scales=(k_scale, v_scale))


def fa_kvcache_append_paged_fp8(k_new, v_new, k_pool, v_pool, block_table, k_scale=None, v_scale=None, cache_seqlens=None,
                                seqlens_out=None, stream=None, *, q=None, q_out=None, rotary_cos=None, rotary_sin=None,
                                rotary_interleaved=False, seqlens_new=None) -> None:
    """fa_kvcache_append_paged into fp8 pools (fa_kvcache_append_paged_fp8): k_pool/v_pool [num_pages,Hkv,page_size,d]
    torch.float8_e4m3fn, block_table as in fa_kvcache_append_paged, scales and codes as in fa_kvcache_append_fp8; the rotary keywords
    as there (fa_kvcache_append_paged_fp8_rope); seqlens_new as in fa_kvcache_append."""
    _append(k_new, v_new, k_pool, v_pool, "k_pool, v_pool", cache_seqlens, seqlens_out, stream,
            (q, q_out, rotary_cos, rotary_sin, rotary_interleaved), seqlens_new, paged=True, block_table=block_table, scales=(k_scale, v_scale))


def fa_kvcache_append_varlen(k_new, v_new, k_cache, v_cache, cu_seqlens_new, cache_seqlens=None, seqlens_out=None, block_table=None,
                             stream=None, *, q=None, q_out=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False,
                             positions=None) -> None:
    """The append of a token-packed batch (fa_kvcache_append_varlen): the write half of fa_forward_varlen_kvcache.  k_new, v_new
    (total_new, Hkv, d) fp16 or bf16 device tensors of ONE dtype, d in {64,128}, taken as they lie: any token and head strides with a
    contiguous last dimension (strides multiples of 8 elements, 16-byte aligned storage), so the K and V views of a fused
    (total_new, Hq + 2*Hkv, d) projection buffer go in without a copy.
    cu_seqlens_new: int32 contiguous device tensor [B+1], read on the device only; sequence b owns the rows [cu[b], cu[b+1]), clamped
    into the tensor as in fa_forward_varlen.  Rows of no sequence are never used.
    k_cache, v_cache: [B,Hkv,Ncap,d] of k_new's dtype, or with block_table (int32 [B, max_pages]) the pools
    [num_pages,Hkv,page_size,d].  Token i of sequence b goes to p = L_b + i, L_b = cache_seqlens[b] clamped to [0, capacity] (None:
    every sequence EMPTY); the drops at the capacity and at a bad table entry are fa_kvcache_append's.
    seqlens_out: int32 [B] that receives min(L_b + m_b, capacity), or None; cache_seqlens itself or disjoint from it; it must not
    overlap cu_seqlens_new.
    rotary_cos, rotary_sin, rotary_interleaved: as in fa_kvcache_append.  q: packed (total_new, Hq, d) of k_new's dtype with its own
    strides, rotated at its token's position into q_out (same shape and dtype, its own strides, not overlapping q) or, with q_out=None,
    in place; q_out rows of no sequence are not written.
    Every kept byte is what fa_kvcache_append(seqlens_new=m) writes from the padded [B,Hkv,max m,d] copy of the same rows.  Nothing is
    read on the host and there is no workspace: append_varlen(seqlens_out=lens) then
    fa_forward_varlen_kvcache(q, ..., cu_seqlens_new, lens), captured once, serves every step of the same total_new.
    positions (fa_kvcache_append_varlen_ex; rotary only): None, or an int32 contiguous tensor (total_new,) on k_new's device.  Token t
    is then rotated (its K row and its q rows) at table row clamp(positions[t], 0, max_pos - 1) while it still goes to slot L_b + i:
    the drafts of a speculation tree sit in consecutive slots and share positions, their depths (tree_from_parents).  Entries of rows
    of no sequence are not read; positions[s_b + i] = L_b + i gives the bytes of the call without positions."""
    _append_varlen(k_new, v_new, k_cache, v_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, stream,
                   (q, q_out, rotary_cos, rotary_sin, rotary_interleaved), positions=positions)


def fa_kvcache_append_varlen_fp8(k_new, v_new, k_cache, v_cache, cu_seqlens_new, cache_seqlens=None, seqlens_out=None, block_table=None,
                                 k_scale=None, v_scale=None, stream=None, *, q=None, q_out=None, rotary_cos=None, rotary_sin=None,
                                 rotary_interleaved=False, positions=None) -> None:
    """fa_kvcache_append_varlen into an fp8 cache: k_cache, v_cache (or the pools) torch.float8_e4m3fn, k_scale, v_scale float32 [Hkv]
    or None (1.0); codes and scales as in fa_kvcache_append_fp8, everything else as in fa_kvcache_append_varlen, positions included."""
    _append_varlen(k_new, v_new, k_cache, v_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, stream,
                   (q, q_out, rotary_cos, rotary_sin, rotary_interleaved), scales=(k_scale, v_scale), positions=positions)


def _append_varlen(k_new, v_new, k_dst, v_dst, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, stream, rope, scales=None,
                   positions=None):
    """The two packed append front ends: scales is None (a 16-bit cache) or (k_scale, v_scale) of an fp8 one; rope is
    (q, q_out, rotary_cos, rotary_sin, rotary_interleaved); positions is None or the vector of fa_kvcache_append_varlen_ex.  Shapes
    and dtypes are judged before anything needs a device."""
    import torch
    fp8 = scales is not None
    paged = block_table is not None
    for name, t in (("k_new", k_new), ("v_new", v_new), ("k_cache", k_dst), ("v_cache", v_dst)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if fp8 and (k_dst.dtype != torch.float8_e4m3fn or v_dst.dtype != torch.float8_e4m3fn):   # judged first, as in the other front ends
        raise ValueError(f"k_cache, v_cache: {_FP8_CACHE} (got {k_dst.dtype}, {v_dst.dtype})")
    if k_new.dim() != 3 or v_new.shape != k_new.shape:
        raise ValueError("k_new, v_new must both be packed tensors (total_new, Hkv, d)")
    total, Hkv, d = k_new.shape
    dts = (torch.float16, torch.bfloat16)
    if k_new.dtype not in dts or v_new.dtype != k_new.dtype:
        raise ValueError("k_new, v_new must both be fp16 or both bf16")
    if d not in (64, 128) or total <= 0 or Hkv <= 0:
        raise ValueError("d must be 64 or 128, and k_new must not be empty")
    if k_dst.dim() != 4 or v_dst.shape != k_dst.shape or k_dst.shape[1] != Hkv or k_dst.shape[3] != d or k_dst.numel() == 0:
        raise ValueError("k_cache and v_cache must both be [B,Hkv,Ncap,d], or with block_table [num_pages,Hkv,page_size,d], with k_new's "
                         "Hkv and d")
    if not fp8 and (k_dst.dtype != k_new.dtype or v_dst.dtype != k_new.dtype):
        raise ValueError(f"k_cache, v_cache must have the dtype of k_new ({k_new.dtype}; got {k_dst.dtype}, {v_dst.dtype}); an fp8 cache "
                         "goes through fa_kvcache_append_varlen_fp8")
    if not isinstance(cu_seqlens_new, torch.Tensor) or cu_seqlens_new.dtype != torch.int32:
        raise ValueError("cu_seqlens_new must be an int32 tensor (the kernel reads 32-bit entries)")
    if cu_seqlens_new.dim() != 1 or cu_seqlens_new.numel() < 2 or not cu_seqlens_new.is_contiguous():
        raise ValueError("cu_seqlens_new must be a contiguous 1-d tensor of B+1 entries")
    B = cu_seqlens_new.numel() - 1
    if paged:
        num_pages, page_size, Ncap = k_dst.shape[0], k_dst.shape[2], 0
        if page_size < 16 or page_size & (page_size - 1):
            raise ValueError("page_size must be a power of two >= 16")
        if not isinstance(block_table, torch.Tensor) or block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] <= 0:
            raise ValueError("block_table must be an int32 device tensor of shape [B, max_pages]")
        max_pages = block_table.shape[1]
    else:
        num_pages, page_size, max_pages, Ncap = 0, 0, 0, k_dst.shape[2]
        if k_dst.shape[0] != B:
            raise ValueError(f"k_cache holds {k_dst.shape[0]} sequences, cu_seqlens_new {B}")
    for name, t in (("cache_seqlens", cache_seqlens), ("seqlens_out", seqlens_out)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.shape != (B,)):
            raise ValueError(f"{name} must be an int32 device tensor of shape [B] = [{B}]")
    (kt, kh), (vt, vh) = _packed_strides(k_new, "k_new"), _packed_strides(v_new, "v_new")
    ks_ptr, vs_ptr = _scale_ptrs(scales[0], scales[1], Hkv) if fp8 else (None, None)
    q, q_out, cos, sin, interleaved = rope
    rope_fields, rope_tensors = {}, ()
    if positions is not None:
        if cos is None:
            raise ValueError("positions are rotary positions: they need rotary_cos")
        if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32:
            raise ValueError("positions must be an int32 tensor: one rotary position per token row")
        if positions.shape != (total,) or not positions.is_contiguous():
            raise ValueError("positions must be a contiguous tensor (total_new,)")
        if positions.device != k_new.device:
            raise ValueError("positions must live on k_new's device")
    if cos is None:
        if q is not None or q_out is not None or sin is not None:
            raise ValueError("q, q_out and rotary_sin are arguments of the rotary append: they need rotary_cos")
    else:
        max_pos, rot_dim = _rope_tables(cos, sin, d)
        interleaved = 1 if interleaved else 0
        G = 1
        if q is None:
            if q_out is not None:
                raise ValueError("q_out needs q")
        else:
            if not isinstance(q, torch.Tensor) or q.dim() != 3 or q.shape[0] != total or q.shape[2] != d or q.shape[1] % Hkv != 0 \
                    or q.shape[1] == 0 or q.dtype != k_new.dtype:
                raise ValueError(f"q must be packed (total_new, Hq, d) = ({total}, Hq, {d}) with Hq a multiple of Hkv = {Hkv}, of k_new's "
                                 "dtype")
            G = q.shape[1] // Hkv
            if q_out is None:
                q_out = q   # in place
            elif not isinstance(q_out, torch.Tensor) or q_out.shape != q.shape or q_out.dtype != q.dtype:
                raise ValueError("q_out must have q's shape and dtype")
            (qt, qh), (qot, qoh) = _packed_strides(q, "q"), _packed_strides(q_out, "q_out")
            for name, t in (("q", q), ("q_out", q_out)):
                if not t.is_cuda:
                    raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
            rope_fields.update(Q=q.data_ptr(), Qout=q_out.data_ptr(), q_stride_t=qt, q_stride_h=qh, qo_stride_t=qot, qo_stride_h=qoh)
        rope_fields.update(rope_cos=_dev_ptr(cos, "rotary_cos", (torch.float32,)), rope_sin=_dev_ptr(sin, "rotary_sin", (torch.float32,)),
                           G=G, rot_dim=rot_dim, max_pos=max_pos, interleaved=interleaved)
        rope_tensors = (q, q_out, cos, sin)
    for name, t in (("k_new", k_new), ("v_new", v_new)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    cu_ptr = _dev_ptr(cu_seqlens_new, "cu_seqlens_new", (torch.int32,))
    table_ptr = _table_ptr(block_table, B) if paged else None
    cache_dts = (torch.float8_e4m3fn,) if fp8 else dts
    k_ptr, v_ptr = _dev_ptr(k_dst, "k_cache", cache_dts), _dev_ptr(v_dst, "v_cache", cache_dts)
    len_ptr = None if cache_seqlens is None else _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    out_ptr = None if seqlens_out is None else _dev_ptr(seqlens_out, "seqlens_out", (torch.int32,))
    desc = capi.new_desc(capi.KvAppendVarlenDesc)
    capi.fill(
        desc, Knew=k_new.data_ptr(), Vnew=v_new.data_ptr(), K=k_ptr, V=v_ptr, cu_seqlens_new=cu_ptr, seqlens_k=len_ptr, seqlens_out=out_ptr,
        block_table=table_ptr, k_scale=ks_ptr, v_scale=vs_ptr, kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT, B=B, Hkv=Hkv, d=d,
        total_new=total, Ncap=Ncap, num_pages=num_pages, page_size=page_size, max_pages=max_pages, dtype=_in_dt(k_new.dtype),
        k_stride_t=kt, k_stride_h=kh, v_stride_t=vt, v_stride_h=vh, stream=_stream_ptr(stream), **rope_fields)
    with torch.cuda.device(_one_device(k_new, v_new, k_dst, v_dst, cu_seqlens_new, block_table, *(scales or ()), cache_seqlens, seqlens_out,
                                       positions, *rope_tensors)):
        if positions is None:
            code = capi.lib().fa_kvcache_append_varlen(desc)
        else:
            opts = capi.new_desc(capi.KvAppendVarlenOpts)
            opts.positions = positions.data_ptr()
            code = capi.lib().fa_kvcache_append_varlen_ex(desc, opts)
    capi.check("fa_kvcache_append_varlen" if positions is None else "fa_kvcache_append_varlen_ex", code)


def tree_from_parents(parents, cu_seqlens):
    """The tree_mask words and rotary depths of a step's draft trees, from parent indices.  parents: int32 (total,), for each token the
    index WITHIN ITS SEQUENCE of its parent, -1 for a root; a parent precedes its child.  cu_seqlens: (B+1,) integer tensor; sequence b
    owns the tokens [cu[b], cu[b+1]).  -> (tree_mask int64 (total,), depth int32 (total,)): bit j of token i's word is set iff token j
    of its sequence is i itself or one of its ancestors, and depth is the number of ancestors, so that
    positions = L_before[b] + depth is the rotary position of fa_kvcache_append_varlen(positions=...).  Tokens of no sequence get 0 and 0.
    Plain torch on the inputs' device (a host-side helper, not a kernel; the bounds are read on the host).  Raises ValueError on a
    sequence of more than 64 tokens and on a parent that does not precede its child."""
    import torch
    if not isinstance(parents, torch.Tensor) or parents.dim() != 1 or parents.dtype != torch.int32:
        raise ValueError("parents must be an int32 tensor (total,)")
    if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.is_floating_point():
        raise ValueError("cu_seqlens must be an integer tensor of B+1 entries")
    total = parents.numel()
    cu = [min(max(int(c), 0), total) for c in cu_seqlens.tolist()]
    mask = torch.zeros(total, dtype=torch.int64, device=parents.device)
    depth = torch.zeros(total, dtype=torch.int32, device=parents.device)
    for b in range(len(cu) - 1):
        s, n = cu[b], max(cu[b + 1] - cu[b], 0)
        if n == 0:
            continue
        if n > 64:
            raise ValueError(f"sequence {b} has {n} tokens: a tree_mask word holds 64")
        par = parents[s:s + n].to(torch.int64)
        idx = torch.arange(n, device=parents.device)
        if bool(((par < -1) | (par >= idx)).any()):
            raise ValueError(f"sequence {b}: a parent must be -1 or precede its child")
        # bit 63 is the sign bit of the word: 1 << 63 wraps to it, which is the pattern the kernel reads
        m = torch.ones(n, dtype=torch.int64, device=parents.device) << idx
        dep = torch.zeros(n, dtype=torch.int32, device=parents.device)
        anc = par.clone()
        while bool((anc >= 0).any()):   # one level of every token's chain per pass: at most n - 1 passes
            has = anc >= 0
            at = anc.clamp(min=0)
            m = torch.where(has, m | (torch.ones_like(m) << at), m)
            dep = dep + has.to(torch.int32)
            anc = torch.where(has, par[at], anc)
        mask[s:s + n] = m
        depth[s:s + n] = dep
    return mask, depth


def tree_accept_mask(tree_mask, cu_seqlens, last):
    """The accept words of fa_kvcache_commit from a step's tree: for each sequence the tree_mask word of its last accepted token,
    tree_mask[cu_seqlens[b] + last[b]] -- that token's own bit and its ancestors', the path that is kept.  tree_mask: int64 (total,)
    as tree_from_parents returns it; cu_seqlens: integer (B+1,); last: integer (B,), the index WITHIN ITS SEQUENCE of the last
    accepted token, -1: nothing accepted (word 0).  -> int64 (B,).  Plain torch on the inputs' device with no host read (an index
    outside the tensor is clamped into it, never a fault), so it can sit inside a captured step between the tree decode and the
    commit."""
    import torch
    if not isinstance(tree_mask, torch.Tensor) or tree_mask.dim() != 1 or tree_mask.dtype != torch.int64 or tree_mask.numel() == 0:
        raise ValueError("tree_mask must be a non-empty int64 tensor (total,)")
    if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.is_floating_point():
        raise ValueError("cu_seqlens must be an integer tensor of B+1 entries")
    if not isinstance(last, torch.Tensor) or last.is_floating_point() or last.shape != (cu_seqlens.numel() - 1,):
        raise ValueError("last must be an integer tensor (B,)")
    last = last.to(torch.int64)
    at = (cu_seqlens[:-1].to(torch.int64) + last).clamp(0, tree_mask.numel() - 1)
    return torch.where(last >= 0, tree_mask[at], torch.zeros_like(last))


def fa_kvcache_commit(k_cache, v_cache, accept_mask, cache_seqlens=None, seqlens_out=None, block_table=None, max_new: int = 64,
                      stream=None) -> None:
    """The commit step of tree speculation (fa_kvcache_commit): after fa_kvcache_append_varlen(positions=...) placed a step's tokens at
    slots L_b, L_b + 1, ... in tree order and the tree decode verified them, the accepted path's K/V rows move to consecutive slots.
    k_cache, v_cache: [B,Hkv,Ncap,d] fp16, bf16 or torch.float8_e4m3fn device tensors of one dtype, d in {64,128}, or with block_table
    (int32 [B, max_pages]) the pools [num_pages,Hkv,page_size,d]; written in place.
    accept_mask: int64 contiguous device tensor (B,), one word per sequence: bit i names the step token at slot L_b + i
    (tree_accept_mask gives it from the tree_mask words).  Bits at or above max_new (1..64) and bits of tokens the append dropped at the
    capacity are ignored.
    cache_seqlens: int32 [B], the lengths BEFORE the step (what the append read), clamped to [0, capacity]; None: 0 for all.
    With i_0 < i_1 < ... the kept bits, row L_b + i_j goes to row L_b + j in every head of K and of V, every bit kept, as if all
    sources were read before any destination was written.  A word that is a low-bit prefix moves nothing and reads no table entry.
    seqlens_out: int32 [B] that receives L_b + popcount, or None; cache_seqlens itself or disjoint from it; it must not overlap
    accept_mask.  Nothing is read on the host and there is no workspace: append, tree decode, commit, captured once, serve every step."""
    import torch
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    dts = (torch.float16, torch.bfloat16, torch.float8_e4m3fn)
    if k_cache.dtype not in dts or v_cache.dtype != k_cache.dtype:
        raise ValueError(f"k_cache, v_cache must both be fp16, both bf16 or both torch.float8_e4m3fn (got {k_cache.dtype}, {v_cache.dtype})")
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape or k_cache.numel() == 0 or k_cache.shape[3] not in (64, 128):
        raise ValueError("k_cache and v_cache must both be [B,Hkv,Ncap,d], or with block_table [num_pages,Hkv,page_size,d], d 64 or 128")
    Hkv, d = k_cache.shape[1], k_cache.shape[3]
    if block_table is not None:
        if not isinstance(block_table, torch.Tensor) or block_table.dim() != 2 or block_table.shape[0] <= 0 or block_table.shape[1] <= 0:
            raise ValueError("block_table must be an int32 device tensor of shape [B, max_pages]")
        B, max_pages = block_table.shape
        num_pages, page_size, Ncap = k_cache.shape[0], k_cache.shape[2], 0
        if page_size < 16 or page_size & (page_size - 1):
            raise ValueError("page_size must be a power of two >= 16")
    else:
        B, Ncap, num_pages, page_size, max_pages = k_cache.shape[0], k_cache.shape[2], 0, 0, 0
    if not isinstance(accept_mask, torch.Tensor) or accept_mask.dtype != torch.int64:
        raise ValueError("accept_mask must be an int64 tensor: one 64-bit word per sequence")
    if accept_mask.shape != (B,) or not accept_mask.is_contiguous():
        raise ValueError(f"accept_mask must be a contiguous tensor [B] = [{B}]")
    if isinstance(max_new, bool) or not isinstance(max_new, int) or not 1 <= max_new <= 64:
        raise ValueError("max_new must be an int in 1..64: a word holds 64 tokens")
    for name, t in (("cache_seqlens", cache_seqlens), ("seqlens_out", seqlens_out)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.shape != (B,)):
            raise ValueError(f"{name} must be an int32 device tensor of shape [B] = [{B}]")
    k_ptr, v_ptr = _dev_ptr(k_cache, "k_cache", dts), _dev_ptr(v_cache, "v_cache", dts)
    word_ptr = _dev_ptr(accept_mask, "accept_mask", (torch.int64,))
    table_ptr = _table_ptr(block_table, B) if block_table is not None else None
    len_ptr = None if cache_seqlens is None else _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    out_ptr = None if seqlens_out is None else _dev_ptr(seqlens_out, "seqlens_out", (torch.int32,))
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    desc = capi.new_desc(capi.KvCommitDesc)
    capi.fill(desc, K=k_ptr, V=v_ptr, seqlens_k=len_ptr, seqlens_out=out_ptr, accept_mask=word_ptr, block_table=table_ptr,
              kv_dtype=capi.KV_FP8_E4M3 if fp8 else capi.KV_16BIT, dtype=capi.F16 if fp8 else _in_dt(k_cache.dtype), B=B, Hkv=Hkv, d=d,
              max_new=max_new, Ncap=Ncap, num_pages=num_pages, page_size=page_size, max_pages=max_pages, stream=_stream_ptr(stream))
    with torch.cuda.device(_one_device(k_cache, v_cache, accept_mask, block_table, cache_seqlens, seqlens_out)):
        code = capi.lib().fa_kvcache_commit(desc)
    capi.check("fa_kvcache_commit", code)


def _mla_cache(c_cache, block_table, B, dtype, name="c_cache"):
    """(Ncap, num_pages, page_size, max_pages, table pointer) of a latent cache [B,Ncap,576] or, with block_table, a pool
    [num_pages,page_size,576]; shapes and dtypes are judged before anything needs a device.  The _fp8 entries judge their cache's
    dtype first (_mla_fp8_cache) and pass dtype = torch.float8_e4m3fn."""
    import torch
    if not isinstance(c_cache, torch.Tensor) or c_cache.dim() != 3 or c_cache.shape[2] != capi.MLA_DQK or c_cache.numel() == 0:
        raise ValueError(f"{name} must be a latent cache [B,Ncap,{capi.MLA_DQK}] or, with block_table, a pool [num_pages,page_size,{capi.MLA_DQK}]")
    if c_cache.dtype != dtype:
        raise ValueError(f"{name} has dtype {c_cache.dtype}, expected {dtype} (an fp8 latent cache goes to fa_mla_decode_fp8 / fa_mla_append_fp8)")
    if block_table is None:
        if c_cache.shape[0] != B:
            raise ValueError(f"{name} holds {c_cache.shape[0]} sequences, the cu_seqlens vector {B}")
        return c_cache.shape[1], 0, 0, 0, None
    page_size = c_cache.shape[1]
    if page_size < 16 or page_size & (page_size - 1):
        raise ValueError("page_size must be a power of two >= 16")
    table_ptr = _table_ptr(block_table, B)
    if block_table.shape[1] <= 0:
        raise ValueError("block_table must have at least one column")
    return 0, c_cache.shape[0], page_size, block_table.shape[1], table_ptr


def _mla_fp8_cache(c_cache, name="c_cache"):
    """the first judgement of the _fp8 MLA entries: the cache's element type"""
    import torch
    if not isinstance(c_cache, torch.Tensor) or c_cache.dtype != torch.float8_e4m3fn:
        raise ValueError(f"{name}: {_FP8_CACHE} (got {getattr(c_cache, 'dtype', type(c_cache).__name__)})")


def _mla_scale_check(c_scale):
    """c_scale of an fp8 latent cache: float32 [1], or None (1.0); judged with the cache, before anything needs a device"""
    import torch
    if c_scale is not None and (not isinstance(c_scale, torch.Tensor) or c_scale.dtype != torch.float32 or tuple(c_scale.shape) != (1,)):
        raise ValueError("c_scale must be a float32 device tensor of shape [1]: the cache's one scale")


def _cu_vector(cu, name: str) -> int:
    """B of a checked cu_seqlens vector"""
    import torch
    if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32:
        raise ValueError(f"{name} must be an int32 tensor (the kernel reads 32-bit entries)")
    if cu.dim() != 1 or cu.numel() < 2 or not cu.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 1-d tensor of B+1 entries")
    return cu.numel() - 1


def mla_decode_workspace_bytes(B: int, Hq: int, max_seqlen_q: int, Ncap: int = 0, max_pages: int = 0, page_size: int = 0,
                               num_splits: int = 0) -> int:
    """Workspace of fa_mla_decode and of fa_mla_decode_fp8, which are equal (fa_mla_decode_workspace_bytes): a contiguous cache gives Ncap, a paged one max_pages and page_size;
    num_splits as in the call (0: the library's choice).  From host integers alone; 0 when one split is chosen, and 0 for a shape
    the call refuses."""
    desc = capi.new_desc(capi.MlaDecodeDesc)
    paged = bool(max_pages or page_size)
    # the pointers and strides are stand-ins that pass the checks: the size reads none of them
    capi.fill(desc, Q=16, O=16, C=16, cu_seqlens_q=16, block_table=16 if paged else None, B=B, Hq=Hq, total_q=max(B, 1) * max(max_seqlen_q, 1),
              max_q=max_seqlen_q, Ncap=0 if paged else Ncap, num_pages=1 if paged else 0, page_size=page_size, max_pages=max_pages,
              q_stride_t=capi.MLA_DQK, q_stride_h=0, o_stride_t=capi.MLA_DC, o_stride_h=0, causal=1, num_splits=num_splits,
              in_dtype=capi.F16, out_dtype=capi.OUT_F32)
    return int(capi.lib().fa_mla_decode_workspace_bytes(desc))


def fa_mla_decode(q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=None, block_table=None, scale: float | None = None,
                  causal: bool = True, num_splits: int = 0, return_lse: bool = False, out=None, workspace=None, out_dtype=None,
                  stream=None, lse=None):
    """Multi-head latent attention decode (fa_mla_decode): absorbed queries against a latent KV cache that holds ONE row of 576
    elements per token for all heads -- 512 compressed-KV elements, then 64 rotary ones.  The logits run over all 576 elements, the
    output is the softmax-weighted sum of the rows' first 512: o (total_q, Hq, 512).
    q: (total_q, Hq, 576) fp16/bf16 device tensor, the absorbed queries [q_nope . W_UK | q_rope], taken as it lies: any token and head
    strides with a contiguous last dimension (multiples of 8 elements, 16-byte aligned storage), so a slice of a fused projection
    buffer goes in without a copy.  1 <= Hq <= 128.  The absorption and the up-projection of o by W_UV stay the caller's GEMMs.
    c_cache: [B, Ncap, 576] of q's dtype, contiguous, or with block_table (int32 [B, max_pages]) a pool [num_pages, page_size, 576],
    page_size a power of two >= 16; key j of sequence b is then row j % page_size of page block_table[b, j // page_size].
    cu_seqlens_q: int32 [B+1] on the device; sequence b owns the tokens [cu[b], cu[b+1]), clamped into the tensor, and has
    n_b = min(cu[b+1] - cu[b], max_seqlen_q) rows, its first n_b tokens.  max_seqlen_q: a host int >= 1; grid, split count and workspace
    follow it, not the vector.
    cache_seqlens: int32 [B], the keys of sequence b, its new tokens INCLUDED (the lengths after fa_mla_append), or None (the capacity).
    With L_b and n_b, row i sees the keys [0, c_i): c_i = max(0, L_b - n_b + 1 + i) with causal (the default), else L_b.  A row
    without a key is O = 0, lse = -inf.  Rows at or past L_b are never used and may hold anything; table entries past the last live
    page are not read, a live entry outside the pool reads as a page of zeros.
    scale: None is 576 ** -0.5; MODELS PASS THEIR OWN -- DeepSeek's softmax scale is that of the un-absorbed head dimension
    (128 + 64) ** -0.5, times the rope-scaling factor where one applies.
    num_splits: 0 (the library chooses from the shape), or the number of key splits, 1 .. ceil(capacity / 64); 1 needs no workspace.
    -> o (total_q, Hq, 512) of out_dtype (torch.float32, the default, or q's dtype), or (o, lse) with return_lse, lse (Hq, total_q)
    float32 in natural-log units.  Tokens that are no live row of any sequence are NOT written: a fresh result holds O = 0 and
    lse = -inf there; with `out` (any token and head strides) and `lse` (contiguous; implies return_lse) they keep what they held.
    workspace: optional uint8 device tensor of at least mla_decode_workspace_bytes(...).
    Nothing is read on the host: fa_mla_append(seqlens_out=lens) then this call, captured once, serves every step of the same total_q.
    An fp8 latent cache: fa_mla_decode_fp8.  Not here: window, soft-cap, sinks, a tree mask, other latent widths."""
    return _mla_decode("fa_mla_decode", None, q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, scale, causal, num_splits,
                       return_lse, out, workspace, out_dtype, stream, lse)


def fa_mla_decode_fp8(q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=None, block_table=None, c_scale=None,
                      scale: float | None = None, causal: bool = True, num_splits: int = 0, return_lse: bool = False, out=None,
                      workspace=None, out_dtype=None, stream=None, lse=None):
    """fa_mla_decode against an fp8 latent cache (fa_mla_decode_fp8): c_cache is torch.float8_e4m3fn, [B, Ncap, 576] or with
    block_table a pool [num_pages, page_size, 576] -- one row of 576 BYTES per token, 512 compressed-KV codes then 64 rotary codes --
    and c_scale is the cache's ONE scale, float32 [1] on the device (read there: a captured call follows it), or None (1.0); an
    element is code * c_scale, c_scale finite and > 0 (quantize_mla_fp8 makes both).  q names the arithmetic's type: the codes are
    widened exactly to it on their way into LDS, and everything else -- rows, clamps, masks, splits (the same num_splits = 0 choice
    and workspace), keywords and results -- is fa_mla_decode's: s = (scale * c_scale) * q . code, o = c_scale * softmax(s) . code[:512].
    Rows at or past a sequence's length and pages no key lies in may hold NaN codes.  With c_scale None the result has the bits of
    fa_mla_decode on the widened cache.
    Not here: per-token or per-128-element scales, a 16-bit rotary tail (656-byte rows), an fp8 q, fp8 matrix instructions."""
    _mla_fp8_cache(c_cache)
    _mla_scale_check(c_scale)
    return _mla_decode("fa_mla_decode_fp8", (c_scale,), q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, scale, causal,
                       num_splits, return_lse, out, workspace, out_dtype, stream, lse)


def _mla_decode(entry, fp8, q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, scale, causal, num_splits, return_lse, out,
                workspace, out_dtype, stream, lse):
    """Both MLA decode front ends: fp8 is None (a cache of q's dtype) or (c_scale,) of a cache of e4m3fn codes."""
    import torch
    if not isinstance(q, torch.Tensor) or q.dim() != 3 or q.shape[2] != capi.MLA_DQK:
        raise ValueError(f"q must be a packed tensor (total_q, Hq, {capi.MLA_DQK}): the absorbed queries")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("q must be fp16 or bf16")
    total_q, Hq = q.shape[0], q.shape[1]
    if total_q <= 0 or not 1 <= Hq <= 128:
        raise ValueError("q must hold at least one token and 1 .. 128 heads")
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 1:
        raise ValueError("max_seqlen_q must be an int >= 1: the most rows a sequence may have")
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or num_splits < 0:
        raise ValueError("num_splits must be an int >= 0 (0: chosen by the library)")
    B = _cu_vector(cu_seqlens_q, "cu_seqlens_q")
    c_dtype = q.dtype if fp8 is None else torch.float8_e4m3fn
    Ncap, num_pages, page_size, max_pages, table_ptr = _mla_cache(c_cache, block_table, B, c_dtype)
    if cache_seqlens is not None and (not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32
                                      or cache_seqlens.shape != (B,)):
        raise ValueError("cache_seqlens must be an int32 device tensor of B entries")
    qt, qh = _packed_strides(q, "q")
    for name, t in (("q", q), ("cu_seqlens_q", cu_seqlens_q)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    c_ptr = _dev_ptr(c_cache, "c_cache", (c_dtype,))
    scale_ptr = None if fp8 is None or fp8[0] is None else _dev_ptr(fp8[0], "c_scale", (torch.float32,))
    lens_ptr = None if cache_seqlens is None else _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    out_dt = _out_dt(out_dtype, q.dtype)
    o_shape = (total_q, Hq, capi.MLA_DC)
    if out is None:   # tokens of no sequence then read as "no key"
        out = torch.zeros(o_shape, dtype=out_dtype, device=q.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or tuple(out.shape) != o_shape or out.dtype != out_dtype:
        raise ValueError(f"out must be a device tensor (total_q, Hq, {capi.MLA_DC}) of out_dtype")
    if lse is not None:
        if not isinstance(lse, torch.Tensor) or lse.shape != (Hq, total_q):
            raise ValueError("lse must be a float32 tensor (Hq, total_q)")
        _dev_ptr(lse, "lse", (torch.float32,))
        return_lse = True
    elif return_lse:
        lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    ot, oh = _packed_strides(out, "out")
    if workspace is None:
        need = mla_decode_workspace_bytes(B, Hq, max_seqlen_q, Ncap, max_pages, page_size, num_splits)
        if need:
            workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_ptr, ws_len = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    desc = capi.new_desc(capi.MlaDecodeDesc)
    capi.fill(desc, Q=q.data_ptr(), O=out.data_ptr(), lse=None if lse is None else lse.data_ptr(), C=c_ptr,
              cu_seqlens_q=cu_seqlens_q.data_ptr(), seqlens_k=lens_ptr, block_table=table_ptr, B=B, Hq=Hq, total_q=total_q,
              max_q=max_seqlen_q, Ncap=Ncap, num_pages=num_pages, page_size=page_size, max_pages=max_pages, q_stride_t=qt, q_stride_h=qh,
              o_stride_t=ot, o_stride_h=oh, scale=float(capi.MLA_DQK ** -0.5 if scale is None else scale), causal=int(bool(causal)),
              num_splits=num_splits, in_dtype=_in_dt(q.dtype), out_dtype=out_dt, workspace=ws_ptr, workspace_bytes=ws_len,
              stream=_stream_ptr(stream))
    with torch.cuda.device(_one_device(q, c_cache, out, cu_seqlens_q, cache_seqlens, block_table, lse, workspace,
                                       None if fp8 is None else fp8[0])):
        code = capi.lib().fa_mla_decode(desc) if fp8 is None else capi.lib().fa_mla_decode_fp8(desc, scale_ptr)
    capi.check(entry, code)
    return (out, lse) if return_lse else out


def fa_mla_append(c_new, c_cache, cu_seqlens_new, cache_seqlens=None, seqlens_out=None, block_table=None, stream=None) -> None:
    """The write half of fa_mla_decode (fa_mla_append): c_new (total_new, 576) fp16/bf16, the step's latent rows [compressed KV |
    rotated k_rope], taken as it lies (any token stride that is a multiple of 8 elements, contiguous rows), cut into sequences by
    cu_seqlens_new (int32 [B+1], device, clamped into the tensor).  Token i of sequence b is copied bit for bit to slot L_b + i of
    c_cache ([B,Ncap,576], or with block_table the pool [num_pages,page_size,576]), L_b = cache_seqlens[b] clamped to the capacity
    (None: 0 for all).  A token at or past the capacity is dropped; a table entry outside the pool skips the write.  No rotary here.
    seqlens_out: None, cache_seqlens itself, or a disjoint int32 [B] tensor: min(L_b + m_b, capacity), by a second kernel behind the
    copy.  Nothing is read on the host."""
    _mla_append("fa_mla_append", None, c_new, c_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, stream)


def fa_mla_append_fp8(c_new, c_cache, cu_seqlens_new, cache_seqlens=None, seqlens_out=None, block_table=None, c_scale=None,
                      stream=None) -> None:
    """fa_mla_append into an fp8 latent cache (fa_mla_append_fp8): c_cache is torch.float8_e4m3fn ([B,Ncap,576] or the pool behind
    block_table), c_scale its one scale, float32 [1] on the device, or None (1.0).  Token i of sequence b is written to slot L_b + i
    as the 576 codes of c_new / c_scale: exact widening to fp32, IEEE division, clamp to +-448, round to nearest even, NaN -> 0x7F --
    the codes quantize_mla_fp8(c_new, c_scale) gives.  Everything else is fa_mla_append's."""
    _mla_fp8_cache(c_cache)
    _mla_scale_check(c_scale)
    _mla_append("fa_mla_append_fp8", (c_scale,), c_new, c_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, stream)


def quantize_mla_fp8(c, scale=None):
    """c [..., 576] (a latent cache, a pool or a step's rows), any float type, CPU or GPU -> (c8 torch.float8_e4m3fn of c's shape,
    scale float32 [1]) with c ~= c8 * scale: the cache's ONE scale, amax / 448 (1.0 for zeros), or the given `scale` (float32 [1] on
    c's device, finite and > 0), returned as it is.  The quotient is clamped to +-448 before the conversion (torch's does not
    saturate) and a NaN becomes the code 0x7F: the codes are those fa_mla_append_fp8 writes for the same scale."""
    import torch
    if not isinstance(c, torch.Tensor) or c.dim() < 1 or c.shape[-1] != capi.MLA_DQK or not c.is_floating_point():
        raise ValueError(f"c must be a float tensor [..., {capi.MLA_DQK}]")
    cf = c.float()
    if scale is None:
        amax = cf.abs().amax().reshape(1) if cf.numel() else cf.new_zeros(1)
        scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    elif not isinstance(scale, torch.Tensor) or tuple(scale.shape) != (1,) or scale.dtype != torch.float32 or scale.device != c.device:
        raise ValueError("scale must be a float32 tensor of shape [1] on c's device")
    q = cf / scale
    nan = q != q
    codes = torch.where(nan, torch.zeros_like(q), q).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    codes = torch.where(nan, torch.full_like(codes, 0x7F), codes)
    return codes.view(torch.float8_e4m3fn), scale.contiguous()


def _mla_append(entry, fp8, c_new, c_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, stream):
    """Both MLA append front ends: fp8 is None (a cache of c_new's dtype) or (c_scale,) of a cache of e4m3fn codes."""
    import torch
    if not isinstance(c_new, torch.Tensor) or c_new.dim() != 2 or c_new.shape[1] != capi.MLA_DQK or c_new.shape[0] <= 0:
        raise ValueError(f"c_new must be a packed tensor (total_new, {capi.MLA_DQK})")
    if c_new.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("c_new must be fp16 or bf16")
    if c_new.stride(1) != 1:
        raise ValueError("c_new must be contiguous in its last dimension (any token stride is taken as it is)")
    B = _cu_vector(cu_seqlens_new, "cu_seqlens_new")
    c_dtype = c_new.dtype if fp8 is None else torch.float8_e4m3fn
    Ncap, num_pages, page_size, max_pages, table_ptr = _mla_cache(c_cache, block_table, B, c_dtype)
    for name, t in (("cache_seqlens", cache_seqlens), ("seqlens_out", seqlens_out)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.shape != (B,)):
            raise ValueError(f"{name} must be an int32 device tensor of shape [B] = [{B}]")
    for name, t in (("c_new", c_new), ("cu_seqlens_new", cu_seqlens_new)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (the HIP path has no CPU fallback)")
    c_ptr = _dev_ptr(c_cache, "c_cache", (c_dtype,))
    scale_ptr = None if fp8 is None or fp8[0] is None else _dev_ptr(fp8[0], "c_scale", (torch.float32,))
    len_ptr = None if cache_seqlens is None else _dev_ptr(cache_seqlens, "cache_seqlens", (torch.int32,))
    out_ptr = None if seqlens_out is None else _dev_ptr(seqlens_out, "seqlens_out", (torch.int32,))
    desc = capi.new_desc(capi.MlaAppendDesc)
    capi.fill(desc, Cnew=c_new.data_ptr(), C=c_ptr, cu_seqlens_new=cu_seqlens_new.data_ptr(), seqlens_k=len_ptr, seqlens_out=out_ptr,
              block_table=table_ptr, B=B, total_new=c_new.shape[0], new_stride_t=c_new.stride(0) if c_new.shape[0] > 1 else capi.MLA_DQK,
              Ncap=Ncap, num_pages=num_pages, page_size=page_size, max_pages=max_pages, dtype=_in_dt(c_new.dtype),
              stream=_stream_ptr(stream))
    with torch.cuda.device(_one_device(c_new, c_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table,
                                       None if fp8 is None else fp8[0])):
        code = capi.lib().fa_mla_append(desc) if fp8 is None else capi.lib().fa_mla_append_fp8(desc, scale_ptr)
    capi.check(entry, code)


def _streaming(fn_name: str, Q, K, V, O, num_batches: int, seq_len: int, scale: float, stream):
    import torch
    if Q.numel() != num_batches * 256 or K.numel() != num_batches * 16 * seq_len \
            or V.numel() != num_batches * 16 * seq_len or O.numel() != num_batches * 256:
        raise ValueError("tensor sizes do not match num_batches/seq_len")
    ptrs = (_dev_ptr(Q, "Q", (torch.float16,)), _dev_ptr(K, "K", (torch.float16,)),
            _dev_ptr(V, "V", (torch.float16,)), _dev_ptr(O, "O", (torch.float32,)))
    with torch.cuda.device(_one_device(Q, K, V, O)):
        code = getattr(capi.lib(), fn_name)(*ptrs, num_batches, seq_len, float(scale), _stream_ptr(stream))
    capi.check(fn_name, code)


def flashattn_streaming_16x16_mw(Q, K, V, O, num_batches: int, seq_len: int, scale: float, stream=None) -> None:
    """(Q,K,V,O,num_batches,seq_len,scale) of flashattn_streaming_16x16_kernel_mw
    (Streaming_FlashAttention_Forward_Kernel/flashattn_streaming_16x16_mw.cu:73-81).
    Q [B,16,16], K [B,16,L], V [B,L,16] fp16; O [B,16,16] fp32."""
    _streaming("flashattn_streaming_16x16_mw", Q, K, V, O, num_batches, seq_len, scale, stream)


def flashattn_streaming_16x16_mw_kt(Q, K_T, V, O, num_batches: int, seq_len: int, scale: float, stream=None) -> None:
    """v8+ ABI: K_T [B,L,16] (flashattn_warp_spc/flashattn_streaming_16x16_mw_v8.cu:103-111)."""
    _streaming("flashattn_streaming_16x16_mw_kt", Q, K_T, V, O, num_batches, seq_len, scale, stream)
