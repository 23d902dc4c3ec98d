"""torch.ops.fa_mi355.forward -- the C-ABI forward as a PyTorch custom op.

Not part of the reference (it has no Python); a convenience for callers that live in PyTorch
graphs.  The op body is the same ctypes call as ops.fa_forward: HIP library or an exception, no
eager fallback.  Registered on first use:

    from flashattention_kernel_project_amd.torch_op import register
    register()
    o = torch.ops.fa_mi355.forward(q, k, v, scale, causal, out_fp32)
    # KV-cache decode: torch.ops.fa_mi355.decode + layout + form, 16 ops.  The layout names the ops function and the leading arguments:
    #   ""           (q, k_cache, v_cache, ...                                   ops.fa_forward_kvcache
    #   "_paged"     (q, k_pool, v_pool, block_table, ...                        ops.fa_forward_kvcache_paged
    #   "_fp8"       (q, k_cache8, v_cache8, k_scale, v_scale, ...               ops.fa_forward_kvcache_fp8
    #   "_paged_fp8" (q, k_pool8, v_pool8, block_table, k_scale, v_scale, ...    ops.fa_forward_kvcache_paged_fp8
    # and the form the rest (window: an int >= 0, 0 = none; sinks: a float32 [Hq] tensor or None; seqlens_q: ops' keyword):
    #   ""        ... cache_seqlens, scale, causal, out_fp32)
    #   "_window" ... cache_seqlens, scale, causal, window, out_fp32)
    #   "_ex"     ... cache_seqlens, scale, causal, window, sinks, softcap, out_fp32)
    #   "_ragged" ... cache_seqlens, seqlens_q, scale, causal, window, sinks, softcap, out_fp32)
    o = torch.ops.fa_mi355.decode_paged_fp8_ex(q, k_pool8, v_pool8, block_table, k_scale, v_scale, cache_seqlens, scale, causal, window,
                                               sinks, softcap, out_fp32)
    # KV-cache append: torch.ops.fa_mi355.append + layout + form, 12 ops that return nothing.  The layouts are the decode ops' with
    # (k_new, v_new, cache or pool, ... in the place of (q, cache or pool, ... (ops.fa_kvcache_append and its _paged, _fp8, _paged_fp8
    # forms); q (or None) is rotated in place; in "_ragged" the three rotary arguments may be None:
    #   ""        ... cache_seqlens, seqlens_out)
    #   "_rope"   ... cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin, interleaved)
    #   "_ragged" ... cache_seqlens, seqlens_out, seqlens_new, q, rotary_cos, rotary_sin, interleaved)
    torch.ops.fa_mi355.append_paged_rope(k_new, v_new, k_pool, v_pool, block_table, cache_seqlens, seqlens_out, q, rotary_cos, rotary_sin,
                                         interleaved)
    # the append of a token-packed batch (ops.fa_kvcache_append_varlen, _fp8): packed sources taken as they lie, q_out None = in place
    torch.ops.fa_mi355.append_varlen(k_new, v_new, k_cache, v_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, q, q_out,
                                     rotary_cos, rotary_sin, interleaved)
    torch.ops.fa_mi355.append_varlen_fp8(k_new, v_new, k_cache8, v_cache8, cu_seqlens_new, cache_seqlens, seqlens_out, block_table,
                                         k_scale, v_scale, q, q_out, rotary_cos, rotary_sin, interleaved)
    # the merge of R attention states, stacked [R,B,Hq,Nq,d] and [R,B,Hq,Nq] (ops.fa_merge_states), and shared-prefix decode on a
    # contiguous 16-bit suffix (ops.fa_forward_kvcache_shared_prefix)
    o, lse = torch.ops.fa_mi355.merge_states(outs, lses, out_f32)
    o = torch.ops.fa_mi355.decode_shared_prefix(q, k_prefix, v_prefix, k_cache, v_cache, prefix_len, cache_seqlens, scale, causal, sinks,
                                                softcap, out_fp32)
    # variable-length packed prefill (ops.fa_forward_varlen): q (total_q,Hq,d), k and v (total_k,Hkv,d), lse (Hq,total_q)
    o, lse = torch.ops.fa_mi355.forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, out_f32)
    # the same with a sliding window, sinks and a soft-cap (the decode _ex form's three arguments, in its order)
    o, lse = torch.ops.fa_mi355.forward_varlen_ex(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, window, sinks, softcap, out_f32)
    # the same against the KV cache, contiguous or (with a block table) paged (ops.fa_forward_varlen_kvcache)
    o, lse = torch.ops.fa_mi355.forward_varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, scale, causal, window,
                                                       sinks, softcap, out_f32)
    # ... and against an fp8 (e4m3fn) cache with per-head scales (ops.fa_forward_varlen_kvcache_fp8)
    o, lse = torch.ops.fa_mi355.forward_varlen_kvcache_fp8(q, k_cache8, v_cache8, cu_seqlens_q, cache_seqlens, block_table, k_scale,
                                                           v_scale, scale, causal, window, sinks, softcap, out_f32)
    # the tree step (speculative decoding): the packed append with explicit rotary positions (int32, total_new) in front of q, and the
    # packed split-KV decode with one int64 ancestor word per token row behind block_table; _fp8 forms take k_scale, v_scale as above
    torch.ops.fa_mi355.append_varlen_pos(k_new, v_new, k_cache, v_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table,
                                         positions, q, q_out, rotary_cos, rotary_sin, interleaved)
    o, lse = torch.ops.fa_mi355.decode_varlen_tree(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, tree_mask,
                                                   scale, causal, window, sinks, softcap, out_f32)
    # ... and its commit (ops.fa_kvcache_commit): the accepted path's K/V rows to consecutive slots, one int64 word per sequence;
    # any cache dtype, block_table None = contiguous
    torch.ops.fa_mi355.commit(k_cache, v_cache, accept_mask, cache_seqlens, seqlens_out, block_table, max_new)
    # the mixed prefill + decode step (ops.fa_kvcache_attend_varlen): sequences of up to split_rows rows on the split-KV stream, longer
    # ones on the tiled kernel, routed on the device; always causal; parts 3 = both halves; _fp8 takes k_scale, v_scale behind block_table
    o, lse = torch.ops.fa_mi355.attend_varlen(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, split_rows, scale, window,
                                              sinks, softcap, parts, out_f32)
    # multi-head latent attention (ops.fa_mla_decode, ops.fa_mla_append): absorbed q (total_q,Hq,576) against a latent cache
    # [B,Ncap,576] or, with a block table, a pool [num_pages,page_size,576]; o is (total_q,Hq,512); num_splits 0 = the library's choice
    o, lse = torch.ops.fa_mi355.mla_decode(q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, scale, causal, num_splits,
                                           out_f32)
    torch.ops.fa_mi355.mla_append(c_new, c_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table)
    # the same against a latent cache of e4m3fn codes (ops.fa_mla_decode_fp8, ops.fa_mla_append_fp8): c_scale, float32 [1] or None,
    # follows block_table
    o, lse = torch.ops.fa_mi355.mla_decode_fp8(q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, c_scale, scale, causal,
                                               num_splits, out_f32)
    torch.ops.fa_mi355.mla_append_fp8(c_new, c_cache, cu_seqlens_new, cache_seqlens, seqlens_out, block_table, c_scale)
"""
from __future__ import annotations

import math

_registered = False


def register() -> None:
    """Define torch.ops.fa_mi355.forward, the 16 .decode and 12 .append ops (layout x form, as the module's docstring lists them),
    .merge_states, .decode_shared_prefix, .forward_varlen, .forward_varlen_ex and .forward_varlen_kvcache (idempotent), and
    .forward_varlen_kvcache_fp8, .append_varlen and .append_varlen_fp8, .decode_varlen and .decode_varlen_fp8, and the tree step's
    .append_varlen_pos, .append_varlen_pos_fp8, .decode_varlen_tree, .decode_varlen_tree_fp8 and .commit, and the mixed step's
    .attend_varlen and .attend_varlen_fp8, and .mla_decode, .mla_append, .mla_decode_fp8 and .mla_append_fp8."""
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

    # The 16 decode and 12 append ops are made from two tables each: the layout gives the leading part of the schema, the ops function
    # and how each leading argument is passed on; the form gives the schema's tail and the keywords made of the arguments behind the
    # leading ones.  The op is <family> + layout + form.
    PASS = {"c": lambda t: t.contiguous(), "o": opt, "-": lambda t: t}

    def define(name, schema, mutates, fn, how, kw, fake):
        def body(*args):   # kw gets the first argument (q, k_new) for the stream and the output type
            return fn(*(PASS[h](t) for h, t in zip(how, args)), **kw(args[0], *args[len(how):]))
        torch.library.custom_op("fa_mi355::" + name, mutates_args=mutates, device_types="cuda", schema=schema)(body).register_fake(fake)

    # `int window` follows `causal`, `Tensor? sinks, float softcap` follow it, `Tensor? seqlens_q` follows `cache_seqlens`
    def ragged_kw(q, cache_seqlens, seqlens_q, scale, causal, window, sinks, softcap, out_fp32):
        return dict(cache_seqlens=opt(cache_seqlens), causal=causal, scale=scale, out_dtype=out_dtype(q, out_fp32), stream=stream(q),
                    window=window, sinks=opt(sinks), softcap=softcap, seqlens_q=opt(seqlens_q))

    DECODE_LAYOUTS = (
        ("", "(Tensor q, Tensor k_cache, Tensor v_cache, ", ops.fa_forward_kvcache, "ccc"),
        ("_paged", "(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, ", ops.fa_forward_kvcache_paged, "cccc"),
        ("_fp8", "(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? k_scale, Tensor? v_scale, ", ops.fa_forward_kvcache_fp8, "cccoo"),
        ("_paged_fp8", "(Tensor q, Tensor k_pool, Tensor v_pool, Tensor block_table, Tensor? k_scale, Tensor? v_scale, ",
         ops.fa_forward_kvcache_paged_fp8, "ccccoo"))
    DECODE_FORMS = (
        ("", "Tensor? cache_seqlens, float scale, bool causal, bool out_fp32) -> Tensor",
         lambda q, lens, scale, causal, out_fp32: ragged_kw(q, lens, None, scale, causal, 0, None, 0.0, out_fp32)),
        ("_window", "Tensor? cache_seqlens, float scale, bool causal, int window, bool out_fp32) -> Tensor",
         lambda q, lens, scale, causal, window, out_fp32: ragged_kw(q, lens, None, scale, causal, window, None, 0.0, out_fp32)),
        ("_ex", "Tensor? cache_seqlens, float scale, bool causal, int window, Tensor? sinks, float softcap, bool out_fp32) -> Tensor",
         lambda q, lens, *rest: ragged_kw(q, lens, None, *rest)),
        ("_ragged", "Tensor? cache_seqlens, Tensor? seqlens_q, float scale, bool causal, int window, Tensor? sinks, float softcap, "
                    "bool out_fp32) -> Tensor", ragged_kw))
    for layout, lead, fn, how in DECODE_LAYOUTS:
        for form, tail, kw in DECODE_FORMS:
            define("decode" + layout + form, lead + tail, (), fn, how, kw, decode_fake)

    # The appends mutate the caches (and seqlens_out) and return nothing.  The caches are passed as they are: a copy made by
    # .contiguous() would take the writes, so a cache that is not contiguous is refused by the front end.  So is q, which the rotary
    # forms rotate in place: it is among their mutated arguments.  In the _ragged form the rotary arguments are optional (all three
    # None: no rotation).
    def ragged_append_kw(k_new, cache_seqlens, seqlens_out, seqlens_new, q, rotary_cos, rotary_sin, interleaved):
        return dict(cache_seqlens=opt(cache_seqlens), seqlens_out=seqlens_out, stream=stream(k_new), q=q, rotary_cos=opt(rotary_cos),
                    rotary_sin=opt(rotary_sin), rotary_interleaved=interleaved, seqlens_new=opt(seqlens_new))

    APPEND_LAYOUTS = (
        ("", "(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, ", ("k_cache", "v_cache"), ops.fa_kvcache_append, "cc--"),
        ("_paged", "(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, ", ("k_pool", "v_pool"),
         ops.fa_kvcache_append_paged, "cc--c"),
        ("_fp8", "(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_scale, Tensor? v_scale, ",
         ("k_cache", "v_cache"), ops.fa_kvcache_append_fp8, "cc--oo"),
        ("_paged_fp8", "(Tensor k_new, Tensor v_new, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, Tensor? k_scale, "
                       "Tensor? v_scale, ", ("k_pool", "v_pool"), ops.fa_kvcache_append_paged_fp8, "cc--coo"))
    APPEND_FORMS = (
        ("", "Tensor? cache_seqlens, Tensor(c!)? seqlens_out) -> ()", ("seqlens_out",),
         lambda k_new, lens, out: dict(cache_seqlens=opt(lens), seqlens_out=out, stream=stream(k_new))),
        ("_rope", "Tensor? cache_seqlens, Tensor(c!)? seqlens_out, Tensor(d!)? q, Tensor rotary_cos, Tensor rotary_sin, "
                  "bool interleaved) -> ()", ("seqlens_out", "q"),
         lambda k_new, lens, out, q, rotary_cos, rotary_sin, interleaved: dict(
             cache_seqlens=opt(lens), seqlens_out=out, stream=stream(k_new), q=q, rotary_cos=rotary_cos.contiguous(),
             rotary_sin=rotary_sin.contiguous(), rotary_interleaved=interleaved)),
        ("_ragged", "Tensor? cache_seqlens, Tensor(c!)? seqlens_out, Tensor? seqlens_new, Tensor(d!)? q, Tensor? rotary_cos, "
                    "Tensor? rotary_sin, bool interleaved) -> ()", ("seqlens_out", "q"), ragged_append_kw))
    for layout, lead, caches, fn, how in APPEND_LAYOUTS:
        for form, tail, more, kw in APPEND_FORMS:
            define("append" + layout + form, lead + tail, caches + more, fn, how, kw, lambda *args: None)

    # The append of a token-packed batch (ops.fa_kvcache_append_varlen, _fp8): k_new, v_new (total_new,Hkv,d) and q, q_out
    # (total_new,Hq,d) go in as they lie -- views of a fused projection buffer are the point -- and the caches are [B,Hkv,Ncap,d] or,
    # with a block table, pools.  q_out None rotates q in place; all of q, q_out and the tables None: no rotation.
    def varlen_append_kw(k_new, cache_seqlens, seqlens_out, block_table, *rest):
        *scales, q, q_out, rotary_cos, rotary_sin, interleaved = rest
        kw = dict(cache_seqlens=opt(cache_seqlens), seqlens_out=seqlens_out, block_table=opt(block_table), stream=stream(k_new), q=q,
                  q_out=q_out, rotary_cos=opt(rotary_cos), rotary_sin=opt(rotary_sin), rotary_interleaved=interleaved)
        if scales:
            kw.update(k_scale=opt(scales[0]), v_scale=opt(scales[1]))
        return kw

    VARLEN_APPEND = "(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_new, Tensor? cache_seqlens, " \
                    "Tensor(c!)? seqlens_out, Tensor? block_table, "
    VARLEN_APPEND_TAIL = "Tensor(d!)? q, Tensor(e!)? q_out, Tensor? rotary_cos, Tensor? rotary_sin, bool interleaved) -> ()"
    for name, mid, fn in (("append_varlen", "", ops.fa_kvcache_append_varlen),
                          ("append_varlen_fp8", "Tensor? k_scale, Tensor? v_scale, ", ops.fa_kvcache_append_varlen_fp8)):
        define(name, VARLEN_APPEND + mid + VARLEN_APPEND_TAIL, ("k_cache", "v_cache", "seqlens_out", "q", "q_out"), fn, "----c",
               varlen_append_kw, lambda *args: None)

    # the same with explicit rotary positions (fa_kvcache_append_varlen_ex): `Tensor positions` (int32, total_new) stands in front of q
    def varlen_append_pos_kw(k_new, cache_seqlens, seqlens_out, block_table, *rest):
        *scales, positions, q, q_out, rotary_cos, rotary_sin, interleaved = rest
        kw = varlen_append_kw(k_new, cache_seqlens, seqlens_out, block_table, *scales, q, q_out, rotary_cos, rotary_sin, interleaved)
        kw.update(positions=positions.contiguous())
        return kw

    for name, mid, fn in (("append_varlen_pos", "", ops.fa_kvcache_append_varlen),
                          ("append_varlen_pos_fp8", "Tensor? k_scale, Tensor? v_scale, ", ops.fa_kvcache_append_varlen_fp8)):
        define(name, VARLEN_APPEND + mid + "Tensor positions, " + VARLEN_APPEND_TAIL, ("k_cache", "v_cache", "seqlens_out", "q", "q_out"),
               fn, "----c", varlen_append_pos_kw, lambda *args: None)

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

    # forward_varlen with `int window, Tensor? sinks, float softcap` behind `causal`, as in the decode _ex form
    @torch.library.custom_op("fa_mi355::forward_varlen_ex", mutates_args=(), device_types="cuda",
                             schema="(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k, float scale, bool causal, "
                                    "int window, Tensor? sinks, float softcap, bool out_f32) -> (Tensor, Tensor)")
    def forward_varlen_ex(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, window, sinks, softcap, out_f32):
        return ops.fa_forward_varlen(q, k, v, cu_seqlens_q.contiguous(), opt(cu_seqlens_k), causal=causal, scale=scale,
                                     out_dtype=out_dtype(q, out_f32), return_lse=True, stream=stream(q), window=window,
                                     softcap=softcap, sinks=opt(sinks))

    @forward_varlen_ex.register_fake
    def _(q, k, v, cu_seqlens_q, cu_seqlens_k, scale, causal, window, sinks, softcap, out_f32):
        return (q.new_empty(q.shape, dtype=out_dtype(q, out_f32)),
                q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32))

    def varlen_fake(q, *args):   # out_f32 is the schema's last argument
        return (q.new_empty(q.shape, dtype=out_dtype(q, args[-1])), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32))

    # forward_varlen_ex against the KV cache (ops.fa_forward_varlen_kvcache): `cache_seqlens` and `Tensor? block_table` take the place
    # of cu_seqlens_k; the caches are [B,Hkv,Ncap,d], or with a block table the pools [num_pages,Hkv,page_size,d]
    define("forward_varlen_kvcache",
           "(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, Tensor cache_seqlens, Tensor? block_table, float scale, "
           "bool causal, int window, Tensor? sinks, float softcap, bool out_f32) -> (Tensor, Tensor)", (),
           ops.fa_forward_varlen_kvcache, "-cccco",
           lambda q, scale, causal, window, sinks, softcap, out_f32: dict(
               causal=causal, scale=scale, out_dtype=out_dtype(q, out_f32), return_lse=True, stream=stream(q), window=window,
               softcap=softcap, sinks=opt(sinks)), varlen_fake)

    # the same on an fp8 cache (ops.fa_forward_varlen_kvcache_fp8): `Tensor? k_scale, Tensor? v_scale` follow `block_table`
    define("forward_varlen_kvcache_fp8",
           "(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, Tensor cache_seqlens, Tensor? block_table, Tensor? k_scale, "
           "Tensor? v_scale, float scale, bool causal, int window, Tensor? sinks, float softcap, bool out_f32) -> (Tensor, Tensor)", (),
           ops.fa_forward_varlen_kvcache_fp8, "-ccccooo",
           lambda q, scale, causal, window, sinks, softcap, out_f32: dict(
               causal=causal, scale=scale, out_dtype=out_dtype(q, out_f32), return_lse=True, stream=stream(q), window=window,
               softcap=softcap, sinks=opt(sinks)), varlen_fake)

    # split-KV decode on a token-packed batch (ops.fa_kvcache_decode_varlen, _fp8): q (total_q,Hq,d) as it lies, `int max_seqlen_q`
    # behind cu_seqlens_q, `Tensor? cache_seqlens`; o and lse come back as from forward_varlen_kvcache, fresh results zero / -inf
    # where no sequence has a live row
    def decode_varlen_kw(q, *rest):
        *scales, scale, causal, window, sinks, softcap, out_f32 = rest
        kw = dict(causal=causal, scale=scale, out_dtype=out_dtype(q, out_f32), return_lse=True, stream=stream(q), window=window,
                  softcap=softcap, sinks=opt(sinks))
        if scales:
            kw.update(k_scale=opt(scales[0]), v_scale=opt(scales[1]))
        return kw

    def decode_varlen(fn):   # max_seqlen_q is positional in ops, behind cu_seqlens_q; the tensors behind it go by keyword
        def call(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, **kw):
            return fn(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=cache_seqlens, block_table=block_table, **kw)
        return call

    DECODE_VARLEN = "(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, int max_seqlen_q, Tensor? cache_seqlens, " \
                    "Tensor? block_table, "
    DECODE_VARLEN_TAIL = "float scale, bool causal, int window, Tensor? sinks, float softcap, bool out_f32) -> (Tensor, Tensor)"
    for name, mid, fn in (("decode_varlen", "", ops.fa_kvcache_decode_varlen),
                          ("decode_varlen_fp8", "Tensor? k_scale, Tensor? v_scale, ", ops.fa_kvcache_decode_varlen_fp8)):
        define(name, DECODE_VARLEN + mid + DECODE_VARLEN_TAIL, (), decode_varlen(fn), "-ccc-oo",
               decode_varlen_kw, varlen_fake)

    # the same with a tree mask (fa_kvcache_decode_varlen_ex): `Tensor tree_mask` (int64, total_q) follows block_table; causal must be True
    def decode_varlen_tree(fn):
        def call(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, tree_mask, **kw):
            return fn(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=cache_seqlens, block_table=block_table,
                      tree_mask=tree_mask, **kw)
        return call

    for name, mid, fn in (("decode_varlen_tree", "", ops.fa_kvcache_decode_varlen),
                          ("decode_varlen_tree_fp8", "Tensor? k_scale, Tensor? v_scale, ", ops.fa_kvcache_decode_varlen_fp8)):
        define(name, DECODE_VARLEN + "Tensor tree_mask, " + mid + DECODE_VARLEN_TAIL, (), decode_varlen_tree(fn), "-ccc-ooc",
               decode_varlen_kw, varlen_fake)

    # the mixed prefill + decode step (ops.fa_kvcache_attend_varlen, _fp8): forward_varlen_kvcache's leading arguments, then
    # `int split_rows` (the routing threshold) and, before out_f32, `int parts` (3: both halves); always causal
    def attend_varlen_kw(q, split_rows, scale, window, sinks, softcap, parts, out_f32):
        return dict(split_rows=split_rows, scale=scale, out_dtype=out_dtype(q, out_f32), return_lse=True, stream=stream(q), window=window,
                    softcap=softcap, sinks=opt(sinks), parts=parts)

    ATTEND_VARLEN_TAIL = "int split_rows, float scale, int window, Tensor? sinks, float softcap, int parts, bool out_f32) -> (Tensor, Tensor)"
    for name, mid, fn, how in (("attend_varlen", "", ops.fa_kvcache_attend_varlen, "-cccco"),
                               ("attend_varlen_fp8", "Tensor? k_scale, Tensor? v_scale, ", ops.fa_kvcache_attend_varlen_fp8, "-ccccooo")):
        define(name, "(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, Tensor cache_seqlens, Tensor? block_table, " + mid +
               ATTEND_VARLEN_TAIL, (), fn, how, attend_varlen_kw, varlen_fake)

    # the commit behind the tree decode (ops.fa_kvcache_commit): the caches go in as they are and are written in place, like the appends'
    define("commit",
           "(Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor accept_mask, Tensor? cache_seqlens, Tensor(c!)? seqlens_out, "
           "Tensor? block_table, int max_new) -> ()", ("k_cache", "v_cache", "seqlens_out"), ops.fa_kvcache_commit, "--c",
           lambda k_cache, cache_seqlens, seqlens_out, block_table, max_new: dict(
               cache_seqlens=opt(cache_seqlens), seqlens_out=seqlens_out, block_table=opt(block_table), max_new=max_new,
               stream=stream(k_cache)), lambda *args: None)

    # MLA (ops.fa_mla_decode, ops.fa_mla_append and their _fp8 forms): q (total_q,Hq,576) as it lies, the latent cache [B,Ncap,576] or
    # with a block table the pool [num_pages,page_size,576]; o (total_q,Hq,512) and lse (Hq,total_q) come back as from decode_varlen.
    # One table: (suffix, what follows block_table in the schema, the front ends, the keywords made of it)
    MLA = (("", "", ops.fa_mla_decode, ops.fa_mla_append, lambda: {}),
           ("_fp8", "Tensor? c_scale, ", ops.fa_mla_decode_fp8, ops.fa_mla_append_fp8, lambda c_scale: dict(c_scale=opt(c_scale))))
    for suffix, mid, decode_fn, append_fn, scale_kw in MLA:
        def mla_decode(q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, decode_fn=decode_fn, **kw):
            return decode_fn(q, c_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens=cache_seqlens, block_table=block_table, **kw)

        def mla_decode_kw(q, *rest, scale_kw=scale_kw):
            *scales, scale, causal, num_splits, out_f32 = rest
            return dict(scale=scale, causal=causal, num_splits=num_splits, out_dtype=out_dtype(q, out_f32), return_lse=True,
                        stream=stream(q), **scale_kw(*scales))

        define("mla_decode" + suffix,
               "(Tensor q, Tensor c_cache, Tensor cu_seqlens_q, int max_seqlen_q, Tensor? cache_seqlens, Tensor? block_table, " + mid +
               "float scale, bool causal, int num_splits, bool out_f32) -> (Tensor, Tensor)", (), mla_decode, "-cc-oo", mla_decode_kw,
               lambda q, *args: (q.new_empty((q.shape[0], q.shape[1], 512), dtype=out_dtype(q, args[-1])),
                                 q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)))

        def mla_append_kw(c_new, cache_seqlens, seqlens_out, block_table, *scales, scale_kw=scale_kw):
            return dict(cache_seqlens=opt(cache_seqlens), seqlens_out=seqlens_out, block_table=opt(block_table), stream=stream(c_new),
                        **scale_kw(*scales))

        # the cache goes in as it is and is written in place, like the other appends'
        define("mla_append" + suffix,
               "(Tensor c_new, Tensor(a!) c_cache, Tensor cu_seqlens_new, Tensor? cache_seqlens, Tensor(b!)? seqlens_out, "
               "Tensor? block_table" + (", " + mid[:-2] if mid else "") + ") -> ()", ("c_cache", "seqlens_out"), append_fn, "--c",
               mla_append_kw, lambda *args: None)

    _registered = True


def sdpa_like(q, k, v, is_causal: bool = False, scale: float | None = None):
    """Same call shape as torch.nn.functional.scaled_dot_product_attention for [B,H,N,d] fp16/bf16
    self-attention without dropout or an explicit mask; output in the input dtype."""
    import torch
    register()
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return torch.ops.fa_mi355.forward(q, k, v, float(scale), bool(is_causal), False)
