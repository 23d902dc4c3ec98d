"""flashattention_kernel_project_amd -- MI355X-native FlashAttention forward behind the
launch signatures of jeehun98/FlashAttention_Kernel_Project.

The product is `libfa_mi355.so` (hand-written HIP for gfx950, C ABI in include/fa_mi355.h).
This package is the Python host side: a ctypes binding of that ABI (`capi`), a torch-tensor
front end with the reference's argument lists (`ops`), and the B x H sharding helper used for
multi-GPU runs (`shard`).  There is no CPU or PyTorch fallback: if the HIP library is missing
or fails to load, every op raises.
"""
from .capi import build, lib, version, FaError  # noqa: F401
from .ops import (  # noqa: F401
    fa_forward,
    fa_forward_splitkv,
    splitkv_workspace_bytes,
    fa_forward_kvcache,
    kvcache_workspace_bytes,
    fa_forward_kvcache_paged,
    kvcache_paged_workspace_bytes,
    kvcache_window_workspace_bytes,
    kvcache_paged_window_workspace_bytes,
    fa_forward_kvcache_fp8,
    fa_forward_kvcache_paged_fp8,
    quantize_kv_fp8,
    fa_kvcache_append,
    fa_kvcache_append_paged,
    fa_kvcache_append_fp8,
    fa_kvcache_append_paged_fp8,
    fa_kvcache_append_varlen,
    fa_kvcache_append_varlen_fp8,
    fa_merge_states,
    fa_forward_kvcache_shared_prefix,
    fa_forward_varlen,
    fa_forward_varlen_kvcache,
    fa_forward_varlen_kvcache_fp8,
    fa_kvcache_decode_varlen,
    fa_kvcache_decode_varlen_fp8,
    kvcache_decode_varlen_workspace_bytes,
    fa_kvcache_attend_varlen,
    fa_kvcache_attend_varlen_fp8,
    tree_from_parents,
    tree_accept_mask,
    fa_kvcache_commit,
    fa_mla_decode,
    mla_decode_workspace_bytes,
    fa_mla_append,
    fa_mla_decode_fp8,
    fa_mla_append_fp8,
    quantize_mla_fp8,
    flashattn_forward_wmma,
    flashattn_streaming_16x16_mw,
    flashattn_streaming_16x16_mw_kt,
    attention_flops,
    attention_min_bytes,
)
from .shard import shard_range  # noqa: F401

__all__ = [
    "build", "lib", "version", "FaError",
    "fa_forward", "fa_forward_splitkv", "splitkv_workspace_bytes", "fa_forward_kvcache",
    "kvcache_workspace_bytes", "fa_forward_kvcache_paged", "kvcache_paged_workspace_bytes", "flashattn_forward_wmma",
    "kvcache_window_workspace_bytes", "kvcache_paged_window_workspace_bytes",
    "fa_forward_kvcache_fp8", "fa_forward_kvcache_paged_fp8", "quantize_kv_fp8",
    "fa_kvcache_append", "fa_kvcache_append_paged", "fa_kvcache_append_fp8", "fa_kvcache_append_paged_fp8",
    "fa_kvcache_append_varlen", "fa_kvcache_append_varlen_fp8",
    "fa_merge_states", "fa_forward_kvcache_shared_prefix", "fa_forward_varlen", "fa_forward_varlen_kvcache",
    "fa_forward_varlen_kvcache_fp8",
    "fa_kvcache_decode_varlen", "fa_kvcache_decode_varlen_fp8", "kvcache_decode_varlen_workspace_bytes", "tree_from_parents",
    "tree_accept_mask", "fa_kvcache_commit", "fa_kvcache_attend_varlen", "fa_kvcache_attend_varlen_fp8",
    "fa_mla_decode", "mla_decode_workspace_bytes", "fa_mla_append", "fa_mla_decode_fp8", "fa_mla_append_fp8", "quantize_mla_fp8",
    "flashattn_streaming_16x16_mw", "flashattn_streaming_16x16_mw_kt",
    "attention_flops", "attention_min_bytes", "shard_range",
]
