"""torch.ops.fa_mi355.forward -- the C-ABI forward as a PyTorch custom op.

Not part of the reference (it has no Python); a convenience for callers that live in PyTorch
graphs.  The op body is the same ctypes call as ops.fa_forward: HIP library or an exception, no
eager fallback.  Registered on first use:

    from flashattention_kernel_project_amd.torch_op import register
    register()
    o = torch.ops.fa_mi355.forward(q, k, v, scale, causal, out_fp32)
    o = torch.ops.fa_mi355.decode(q, k_cache, v_cache, cache_seqlens, scale, causal, out_fp32)   # ops.fa_forward_kvcache
    o = torch.ops.fa_mi355.decode_paged(q, k_pool, v_pool, block_table, cache_seqlens, scale, causal, out_fp32)   # ops.fa_forward_kvcache_paged
    o = torch.ops.fa_mi355.decode_fp8(q, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, scale, causal, out_fp32)   # ops.fa_forward_kvcache_fp8
    o = torch.ops.fa_mi355.decode_paged_fp8(q, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, scale, causal, out_fp32)
    # the same four with a sliding window: `window` (an int >= 0, 0 = none) follows `causal`, as in the C entries
    o = torch.ops.fa_mi355.decode_window(q, k_cache, v_cache, cache_seqlens, scale, causal, window, out_fp32)
    o = torch.ops.fa_mi355.decode_paged_window(q, k_pool, v_pool, block_table, cache_seqlens, scale, causal, window, out_fp32)
    o = torch.ops.fa_mi355.decode_fp8_window(q, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, scale, causal, window, out_fp32)
    o = torch.ops.fa_mi355.decode_paged_fp8_window(q, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, scale, causal,
                                                   window, out_fp32)
    # ... and with attention sinks and soft-capped logits: (window, sinks, softcap) follow `causal`; sinks is a float32 [Hq] tensor or None
    o = torch.ops.fa_mi355.decode_ex(q, k_cache, v_cache, cache_seqlens, scale, causal, window, sinks, softcap, out_fp32)
    o = torch.ops.fa_mi355.decode_paged_ex(q, k_pool, v_pool, block_table, cache_seqlens, scale, causal, window, sinks, softcap, out_fp32)
    o = torch.ops.fa_mi355.decode_fp8_ex(q, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, scale, causal, window, sinks, softcap,
                                         out_fp32)
    o = torch.ops.fa_mi355.decode_paged_fp8_ex(q, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, scale, causal, window,
                                               sinks, softcap, out_fp32)
    torch.ops.fa_mi355.append(k_new, v_new, k_cache, v_cache, cache_seqlens, seqlens_out)   # ops.fa_kvcache_append; returns nothing
    torch.ops.fa_mi355.append_paged(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out)
    torch.ops.fa_mi355.append_fp8(k_new, v_new, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, seqlens_out)
    torch.ops.fa_mi355.append_paged_fp8(k_new, v_new, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, seqlens_out)
    # the same four with rotary embedding: (q, rotary_cos, rotary_sin, interleaved) follow the base op's list; q (or None) is rotated in place
    torch.ops.fa_mi355.append_rope(k_new, v_new, k_cache, v_cache, cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin, interleaved)
    torch.ops.fa_mi355.append_paged_rope(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin,
                                         interleaved)
    torch.ops.fa_mi355.append_fp8_rope(k_new, v_new, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, seqlens_out, q, rotary_cos,
                                       rotary_sin, interleaved)
    torch.ops.fa_mi355.append_paged_fp8_rope(k_new, v_new, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, seqlens_out,
                                             q, rotary_cos, rotary_sin, interleaved)
    # a count per sequence (ops' seqlens_q / seqlens_new): the _ex schema with `Tensor? seqlens_q` after cache_seqlens, and the _rope schema
    # with q, rotary_cos, rotary_sin optional and `Tensor? seqlens_new` after seqlens_out
    o = torch.ops.fa_mi355.decode_ragged(q, k_cache, v_cache, cache_seqlens, seqlens_q, scale, causal, window, sinks, softcap, out_fp32)
    o = torch.ops.fa_mi355.decode_paged_ragged(q, k_pool, v_pool, block_table, cache_seqlens, seqlens_q, scale, causal, window, sinks,
                                               softcap, out_fp32)
    o = torch.ops.fa_mi355.decode_fp8_ragged(q, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, seqlens_q, scale, causal, window,
                                             sinks, softcap, out_fp32)
    o = torch.ops.fa_mi355.decode_paged_fp8_ragged(q, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, seqlens_q, scale,
                                                   causal, window, sinks, softcap, out_fp32)
    torch.ops.fa_mi355.append_ragged(k_new, v_new, k_cache, v_cache, cache_seqlens, seqlens_out, seqlens_new, q, rotary_cos, rotary_sin,
                                     interleaved)
    torch.ops.fa_mi355.append_paged_ragged(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out, seqlens_new, q,
                                           rotary_cos, rotary_sin, interleaved)
    torch.ops.fa_mi355.append_fp8_ragged(k_new, v_new, k_cache8, v_cache8, k_scale, v_scale, cache_seqlens, seqlens_out, seqlens_new, q,
                                         rotary_cos, rotary_sin, interleaved)
    torch.ops.fa_mi355.append_paged_fp8_ragged(k_new, v_new, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, seqlens_out,
                                               seqlens_new, q, rotary_cos, rotary_sin, interleaved)
    # the merge of R attention states, stacked [R,B,Hq,Nq,d] and [R,B,Hq,Nq] (ops.fa_merge_states), and shared-prefix decode on a
    # contiguous 16-bit suffix (ops.fa_forward_kvcache_shared_prefix)
    o, lse = torch.ops.fa_mi355.merge_states(outs, lses, out_f32)
    o = torch.ops.fa_mi355.decode_shared_prefix(q, k_prefix, v_prefix, k_cache, v_cache, prefix_len, cache_seqlens, scale, causal, sinks,
                                                softcap, out_fp32)
    # variable-length packed prefill (ops.fa_forward_varlen): q (total_q,Hq,d), k and v (total_k,Hkv,d), lse (Hq,total_q)
    o, lse = torch.ops.fa_mi355.forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, out_f32)
"""
from __future__ import annotations

import math

_registered = False


def register() -> None:
    """Define torch.ops.fa_mi355.forward, .decode, .decode_paged, .decode_fp8, .decode_paged_fp8, their four _window and four _ex forms, the
    four .append ops and their four _rope forms, the four decode and four append _ragged forms, .merge_states,
    .decode_shared_prefix and .forward_varlen (idempotent)."""
    global _registered
    if _registered:
        return
    import torch
    from . import ops

    def opt(t):
        return None if t is None else t.contiguous()

    def out_dtype(q, out_fp32):
        return torch.float32 if out_fp32 else q.dtype

    def stream(t):
        return torch.cuda.current_stream(t.device)

    def decode_fake(q, *args):   # every decode op: an output of q's shape; out_fp32 is each schema's last argument
        return q.new_empty(q.shape, dtype=out_dtype(q, args[-1]))

    @torch.library.custom_op("fa_mi355::forward", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k, Tensor v, float scale, bool causal, bool out_fp32) -> Tensor")
    def forward(q, k, v, scale, causal, out_fp32):
        return ops.fa_forward(q.contiguous(), k.contiguous(), v.contiguous(), scale=scale, out_dtype=out_dtype(q, out_fp32),
                              causal=causal, stream=stream(q))

    @forward.register_fake
    def _(q, k, v, scale, causal, out_fp32):
        return q.new_empty(q.shape, dtype=out_dtype(q, out_fp32))

    @torch.library.custom_op("fa_mi355::decode", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? cache_seqlens, float scale, bool causal, "
                                    "bool out_fp32) -> Tensor")
    def decode(q, k_cache, v_cache, cache_seqlens, scale, causal, out_fp32):
        return ops.fa_forward_kvcache(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(cache_seqlens), causal=causal,
                                      scale=scale, out_dtype=out_dtype(q, out_fp32), stream=stream(q))

    @torch.library.custom_op("fa_mi355::decode_paged", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? cache_seqlens, float scale, "
                                    "bool causal, bool out_fp32) -> Tensor")
    def decode_paged(q, k_pool, v_pool, block_table, cache_seqlens, scale, causal, out_fp32):
        return ops.fa_forward_kvcache_paged(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                            opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
                                            stream=stream(q))

    @torch.library.custom_op("fa_mi355::decode_fp8", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? k_scale, Tensor? v_scale, "
                                    "Tensor? cache_seqlens, float scale, bool causal, bool out_fp32) -> Tensor")
    def decode_fp8(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, scale, causal, out_fp32):
        return ops.fa_forward_kvcache_fp8(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(k_scale), opt(v_scale),
                                          opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
                                          stream=stream(q))

    @torch.library.custom_op("fa_mi355::decode_paged_fp8", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? k_scale, Tensor? v_scale, "
                                    "Tensor? cache_seqlens, float scale, bool causal, bool out_fp32) -> Tensor")
    def decode_paged_fp8(q, k_pool, v_pool, block_table, k_scale, v_scale, cache_seqlens, scale, causal, out_fp32):
        return ops.fa_forward_kvcache_paged_fp8(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                                opt(k_scale), opt(v_scale), opt(cache_seqlens), causal=causal, scale=scale,
                                                out_dtype=out_dtype(q, out_fp32), stream=stream(q))

    # The sliding-window forms: the schema of the op above each with `int window` after `causal`; the existing ops keep theirs.
    @torch.library.custom_op("fa_mi355::decode_window", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? cache_seqlens, float scale, bool causal, "
                                    "int window, bool out_fp32) -> Tensor")
    def decode_window(q, k_cache, v_cache, cache_seqlens, scale, causal, window, out_fp32):
        return ops.fa_forward_kvcache(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(cache_seqlens), causal=causal,
                                      scale=scale, out_dtype=out_dtype(q, out_fp32), stream=stream(q), window=window)

    @torch.library.custom_op("fa_mi355::decode_paged_window", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? cache_seqlens, float scale, "
                                    "bool causal, int window, bool out_fp32) -> Tensor")
    def decode_paged_window(q, k_pool, v_pool, block_table, cache_seqlens, scale, causal, window, out_fp32):
        return ops.fa_forward_kvcache_paged(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                            opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
                                            stream=stream(q), window=window)

    @torch.library.custom_op("fa_mi355::decode_fp8_window", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? k_scale, Tensor? v_scale, "
                                    "Tensor? cache_seqlens, float scale, bool causal, int window, bool out_fp32) -> Tensor")
    def decode_fp8_window(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, scale, causal, window, out_fp32):
        return ops.fa_forward_kvcache_fp8(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(k_scale), opt(v_scale),
                                          opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
                                          stream=stream(q), window=window)

    @torch.library.custom_op("fa_mi355::decode_paged_fp8_window", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? k_scale, Tensor? v_scale, "
                                    "Tensor? cache_seqlens, float scale, bool causal, int window, bool out_fp32) -> Tensor")
    def decode_paged_fp8_window(q, k_pool, v_pool, block_table, k_scale, v_scale, cache_seqlens, scale, causal, window, out_fp32):
        return ops.fa_forward_kvcache_paged_fp8(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                                opt(k_scale), opt(v_scale), opt(cache_seqlens), causal=causal, scale=scale,
                                                out_dtype=out_dtype(q, out_fp32), stream=stream(q), window=window)

    # The forms with attention sinks and a soft-cap: the schema of the windowed op above each with `Tensor? sinks, float softcap`
    # after `window`.
    @torch.library.custom_op("fa_mi355::decode_ex", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? cache_seqlens, float scale, bool causal, "
                                    "int window, Tensor? sinks, float softcap, bool out_fp32) -> Tensor")
    def decode_ex(q, k_cache, v_cache, cache_seqlens, scale, causal, window, sinks, softcap, out_fp32):
        return ops.fa_forward_kvcache(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(cache_seqlens), causal=causal,
                                      scale=scale, out_dtype=out_dtype(q, out_fp32), stream=stream(q), window=window,
                                      sinks=opt(sinks), softcap=softcap)

    @torch.library.custom_op("fa_mi355::decode_paged_ex", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? cache_seqlens, float scale, "
                                    "bool causal, int window, Tensor? sinks, float softcap, bool out_fp32) -> Tensor")
    def decode_paged_ex(q, k_pool, v_pool, block_table, cache_seqlens, scale, causal, window, sinks, softcap, out_fp32):
        return ops.fa_forward_kvcache_paged(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                            opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
                                            stream=stream(q), window=window, sinks=opt(sinks), softcap=softcap)

    @torch.library.custom_op("fa_mi355::decode_fp8_ex", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? k_scale, Tensor? v_scale, "
                                    "Tensor? cache_seqlens, float scale, bool causal, int window, Tensor? sinks, float softcap, "
                                    "bool out_fp32) -> Tensor")
    def decode_fp8_ex(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, scale, causal, window, sinks, softcap, out_fp32):
        return ops.fa_forward_kvcache_fp8(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(k_scale), opt(v_scale),
                                          opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
                                          stream=stream(q), window=window, sinks=opt(sinks), softcap=softcap)

    @torch.library.custom_op("fa_mi355::decode_paged_fp8_ex", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? k_scale, Tensor? v_scale, "
                                    "Tensor? cache_seqlens, float scale, bool causal, int window, Tensor? sinks, float softcap, "
                                    "bool out_fp32) -> Tensor")
    def decode_paged_fp8_ex(q, k_pool, v_pool, block_table, k_scale, v_scale, cache_seqlens, scale, causal, window, sinks, softcap,
                            out_fp32):
        return ops.fa_forward_kvcache_paged_fp8(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                                opt(k_scale), opt(v_scale), opt(cache_seqlens), causal=causal, scale=scale,
                                                out_dtype=out_dtype(q, out_fp32), stream=stream(q), window=window,
                                                sinks=opt(sinks), softcap=softcap)

    # The forms with a query count per sequence: the schema of the _ex op above each with `Tensor? seqlens_q` after `cache_seqlens`.
    RAGGED = "Tensor? cache_seqlens, Tensor? seqlens_q, float scale, bool causal, int window, Tensor? sinks, float softcap, " \
             "bool out_fp32) -> Tensor"

    def ragged_kw(q, cache_seqlens, seqlens_q, scale, causal, window, sinks, softcap, out_fp32):
        return dict(cache_seqlens=opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32), stream=stream(q),
                    window=window, sinks=opt(sinks), softcap=softcap, seqlens_q=opt(seqlens_q))

    @torch.library.custom_op("fa_mi355::decode_ragged", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, " + RAGGED)
    def decode_ragged(q, k_cache, v_cache, *rest):
        return ops.fa_forward_kvcache(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), **ragged_kw(q, *rest))

    @torch.library.custom_op("fa_mi355::decode_paged_ragged", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, " + RAGGED)
    def decode_paged_ragged(q, k_pool, v_pool, block_table, *rest):
        return ops.fa_forward_kvcache_paged(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                            **ragged_kw(q, *rest))

    @torch.library.custom_op("fa_mi355::decode_fp8_ragged", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? k_scale, Tensor? v_scale, " + RAGGED)
    def decode_fp8_ragged(q, k_cache, v_cache, k_scale, v_scale, *rest):
        return ops.fa_forward_kvcache_fp8(q.contiguous(), k_cache.contiguous(), v_cache.contiguous(), opt(k_scale), opt(v_scale),
                                          **ragged_kw(q, *rest))

    @torch.library.custom_op("fa_mi355::decode_paged_fp8_ragged", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? k_scale, Tensor? v_scale, "
                                    + RAGGED)
    def decode_paged_fp8_ragged(q, k_pool, v_pool, block_table, k_scale, v_scale, *rest):
        return ops.fa_forward_kvcache_paged_fp8(q.contiguous(), k_pool.contiguous(), v_pool.contiguous(), block_table.contiguous(),
                                                opt(k_scale), opt(v_scale), **ragged_kw(q, *rest))

    for op in (decode, decode_paged, decode_fp8, decode_paged_fp8, decode_window, decode_paged_window, decode_fp8_window,
               decode_paged_fp8_window, decode_ex, decode_paged_ex, decode_fp8_ex, decode_paged_fp8_ex, decode_ragged,
               decode_paged_ragged, decode_fp8_ragged, decode_paged_fp8_ragged):
        op.register_fake(decode_fake)

    # The appends mutate the caches (and seqlens_out) and return nothing.  The caches are passed as they are: a copy made by
    # .contiguous() would take the writes, so a cache that is not contiguous is refused by the front end.
    @torch.library.custom_op("fa_mi355::append", mutates_args=("k_cache", "v_cache", "seqlens_out"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? cache_seqlens, "
                                    "Tensor(c!)? seqlens_out) -> ()")
    def append(k_new, v_new, k_cache, v_cache, cache_seqlens, seqlens_out):
        ops.fa_kvcache_append(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache, opt(cache_seqlens), seqlens_out,
                              stream=stream(k_new))

    @append.register_fake
    def _(k_new, v_new, k_cache, v_cache, cache_seqlens, seqlens_out):
        return None

    @torch.library.custom_op("fa_mi355::append_paged", mutates_args=("k_pool", "v_pool", "seqlens_out"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                                    "Tensor? cache_seqlens, Tensor(c!)? seqlens_out) -> ()")
    def append_paged(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out):
        ops.fa_kvcache_append_paged(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                    opt(cache_seqlens), seqlens_out, stream=stream(k_new))

    @append_paged.register_fake
    def _(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out):
        return None

    @torch.library.custom_op("fa_mi355::append_fp8", mutates_args=("k_cache", "v_cache", "seqlens_out"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_scale, "
                                    "Tensor? v_scale, Tensor? cache_seqlens, Tensor(c!)? seqlens_out) -> ()")
    def append_fp8(k_new, v_new, k_cache, v_cache, k_scale, v_scale, cache_seqlens, seqlens_out):
        ops.fa_kvcache_append_fp8(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache, opt(k_scale), opt(v_scale),
                                  opt(cache_seqlens), seqlens_out, stream=stream(k_new))

    @append_fp8.register_fake
    def _(k_new, v_new, k_cache, v_cache, k_scale, v_scale, cache_seqlens, seqlens_out):
        return None

    @torch.library.custom_op("fa_mi355::append_paged_fp8", mutates_args=("k_pool", "v_pool", "seqlens_out"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                                    "Tensor? k_scale, Tensor? v_scale, Tensor? cache_seqlens, Tensor(c!)? seqlens_out) -> ()")
    def append_paged_fp8(k_new, v_new, k_pool, v_pool, block_table, k_scale, v_scale, cache_seqlens, seqlens_out):
        ops.fa_kvcache_append_paged_fp8(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                        opt(k_scale), opt(v_scale), opt(cache_seqlens), seqlens_out, stream=stream(k_new))

    @append_paged_fp8.register_fake
    def _(k_new, v_new, k_pool, v_pool, block_table, k_scale, v_scale, cache_seqlens, seqlens_out):
        return None

    # The rotary forms: the schema of the op above each plus (q, rotary_cos, rotary_sin, interleaved).  q is rotated in place, so it is
    # passed as it is, like the caches, and is among the mutated arguments.
    ROPE = "Tensor(d!)? q, Tensor rotary_cos, Tensor rotary_sin, bool interleaved) -> ()"

    def rope_kw(q, rotary_cos, rotary_sin, interleaved):
        return dict(q=q, rotary_cos=rotary_cos.contiguous(), rotary_sin=rotary_sin.contiguous(), rotary_interleaved=interleaved)

    @torch.library.custom_op("fa_mi355::append_rope", mutates_args=("k_cache", "v_cache", "seqlens_out", "q"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? cache_seqlens, "
                                    "Tensor(c!)? seqlens_out, " + ROPE)
    def append_rope(k_new, v_new, k_cache, v_cache, cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin, interleaved):
        ops.fa_kvcache_append(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache, opt(cache_seqlens), seqlens_out,
                              stream=stream(k_new), **rope_kw(q, rotary_cos, rotary_sin, interleaved))

    @torch.library.custom_op("fa_mi355::append_paged_rope", mutates_args=("k_pool", "v_pool", "seqlens_out", "q"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                                    "Tensor? cache_seqlens, Tensor(c!)? seqlens_out, " + ROPE)
    def append_paged_rope(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin,
                          interleaved):
        ops.fa_kvcache_append_paged(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                    opt(cache_seqlens), seqlens_out, stream=stream(k_new),
                                    **rope_kw(q, rotary_cos, rotary_sin, interleaved))

    @torch.library.custom_op("fa_mi355::append_fp8_rope", mutates_args=("k_cache", "v_cache", "seqlens_out", "q"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_scale, "
                                    "Tensor? v_scale, Tensor? cache_seqlens, Tensor(c!)? seqlens_out, " + ROPE)
    def append_fp8_rope(k_new, v_new, k_cache, v_cache, k_scale, v_scale, cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin,
                        interleaved):
        ops.fa_kvcache_append_fp8(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache, opt(k_scale), opt(v_scale),
                                  opt(cache_seqlens), seqlens_out, stream=stream(k_new),
                                  **rope_kw(q, rotary_cos, rotary_sin, interleaved))

    @torch.library.custom_op("fa_mi355::append_paged_fp8_rope", mutates_args=("k_pool", "v_pool", "seqlens_out", "q"),
                             device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                                    "Tensor? k_scale, Tensor? v_scale, Tensor? cache_seqlens, Tensor(c!)? seqlens_out, " + ROPE)
    def append_paged_fp8_rope(k_new, v_new, k_pool, v_pool, block_table, k_scale, v_scale, cache_seqlens, seqlens_out, q, rotary_cos,
                              rotary_sin, interleaved):
        ops.fa_kvcache_append_paged_fp8(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                        opt(k_scale), opt(v_scale), opt(cache_seqlens), seqlens_out, stream=stream(k_new),
                                        **rope_kw(q, rotary_cos, rotary_sin, interleaved))

    # The forms with a token count per sequence: the schema of the _rope op above each with `Tensor? seqlens_new` after `seqlens_out` and
    # the rotary arguments optional (all three None: no rotation).
    RAGGED_APPEND = "Tensor? cache_seqlens, Tensor(c!)? seqlens_out, Tensor? seqlens_new, Tensor(d!)? q, Tensor? rotary_cos, " \
                    "Tensor? rotary_sin, bool interleaved) -> ()"

    def ragged_append_kw(k_new, cache_seqlens, seqlens_out, seqlens_new, q, rotary_cos, rotary_sin, interleaved):
        return dict(cache_seqlens=opt(cache_seqlens), seqlens_out=seqlens_out, stream=stream(k_new), q=q, rotary_cos=opt(rotary_cos),
                    rotary_sin=opt(rotary_sin), rotary_interleaved=interleaved, seqlens_new=opt(seqlens_new))

    @torch.library.custom_op("fa_mi355::append_ragged", mutates_args=("k_cache", "v_cache", "seqlens_out", "q"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, " + RAGGED_APPEND)
    def append_ragged(k_new, v_new, k_cache, v_cache, *rest):
        ops.fa_kvcache_append(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache, **ragged_append_kw(k_new, *rest))

    @torch.library.custom_op("fa_mi355::append_paged_ragged", mutates_args=("k_pool", "v_pool", "seqlens_out", "q"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                                    + RAGGED_APPEND)
    def append_paged_ragged(k_new, v_new, k_pool, v_pool, block_table, *rest):
        ops.fa_kvcache_append_paged(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                    **ragged_append_kw(k_new, *rest))

    @torch.library.custom_op("fa_mi355::append_fp8_ragged", mutates_args=("k_cache", "v_cache", "seqlens_out", "q"), device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_scale, "
                                    "Tensor? v_scale, " + RAGGED_APPEND)
    def append_fp8_ragged(k_new, v_new, k_cache, v_cache, k_scale, v_scale, *rest):
        ops.fa_kvcache_append_fp8(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache, opt(k_scale), opt(v_scale),
                                  **ragged_append_kw(k_new, *rest))

    @torch.library.custom_op("fa_mi355::append_paged_fp8_ragged", mutates_args=("k_pool", "v_pool", "seqlens_out", "q"),
                             device_types="cuda",
                             schema="(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                                    "Tensor? k_scale, Tensor? v_scale, " + RAGGED_APPEND)
    def append_paged_fp8_ragged(k_new, v_new, k_pool, v_pool, block_table, k_scale, v_scale, *rest):
        ops.fa_kvcache_append_paged_fp8(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                        opt(k_scale), opt(v_scale), **ragged_append_kw(k_new, *rest))

    for op in (append_rope, append_paged_rope, append_fp8_rope, append_paged_fp8_rope, append_ragged, append_paged_ragged,
               append_fp8_ragged, append_paged_fp8_ragged):
        op.register_fake(lambda *args: None)

    # The merge of attention states over key ranges (ops.fa_merge_states) on stacked parts, and shared-prefix decode on a contiguous
    # 16-bit suffix (ops.fa_forward_kvcache_shared_prefix; the paged and fp8 forms are the front end's).
    @torch.library.custom_op("fa_mi355::merge_states", mutates_args=(), device_types="cuda",
                             schema="(Tensor outs, Tensor lses, bool out_f32) -> (Tensor, Tensor)")
    def merge_states(outs, lses, out_f32):
        outs, lses = outs.contiguous(), lses.contiguous()
        return ops.fa_merge_states(list(outs.unbind(0)), list(lses.unbind(0)), out_dtype=out_dtype(outs, out_f32), stream=stream(outs))

    @merge_states.register_fake
    def _(outs, lses, out_f32):
        return outs.new_empty(outs.shape[1:], dtype=out_dtype(outs, out_f32)), lses.new_empty(lses.shape[1:], dtype=torch.float32)

    @torch.library.custom_op("fa_mi355::decode_shared_prefix", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k_prefix, Tensor v_prefix, Tensor k_cache, Tensor v_cache, Tensor? prefix_len, "
                                    "Tensor? cache_seqlens, float scale, bool causal, Tensor? sinks, float softcap, bool out_fp32) "
                                    "-> Tensor")
    def decode_shared_prefix(q, k_prefix, v_prefix, k_cache, v_cache, prefix_len, cache_seqlens, scale, causal, sinks, softcap,
                             out_fp32):
        return ops.fa_forward_kvcache_shared_prefix(
            q.contiguous(), k_prefix.contiguous(), v_prefix.contiguous(), k_cache.contiguous(), v_cache.contiguous(),
            prefix_len=opt(prefix_len), cache_seqlens=opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32),
            sinks=opt(sinks), softcap=softcap, stream=stream(q))

    decode_shared_prefix.register_fake(decode_fake)

    # Variable-length packed prefill (ops.fa_forward_varlen): q (total_q,Hq,d), k and v (total_k,Hkv,d) as they lie (any token and head
    # strides), cu_seqlens_k None = cu_seqlens_q; lse (Hq,total_q) is always returned.
    @torch.library.custom_op("fa_mi355::forward_varlen", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k, float scale, bool causal, "
                                    "bool out_f32) -> (Tensor, Tensor)")
    def forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, out_f32):
        return ops.fa_forward_varlen(q, k, v, cu_seqlens_q.contiguous(), opt(cu_seqlens_k), causal=causal, scale=scale,
                                     out_dtype=out_dtype(q, out_f32), return_lse=True, stream=stream(q))

    @forward_varlen.register_fake
    def _(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, out_f32):
        return (q.new_empty(q.shape, dtype=out_dtype(q, out_f32)),
                q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32))

    _registered = True


def sdpa_like(q, k, v, is_causal: bool = False, scale: float | None = None):
    """Same call shape as torch.nn.functional.scaled_dot_product_attention for [B,H,N,d] fp16/bf16
    self-attention without dropout or an explicit mask; output in the input dtype."""
    import torch
    register()
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return torch.ops.fa_mi355.forward(q, k, v, float(scale), bool(is_causal), False)
