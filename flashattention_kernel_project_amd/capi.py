"""ctypes binding of include/fa_mi355.h (libfa_mi355.so, built in-tree by csrc/Makefile)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FA_MI355_LIB") or os.path.join(_HERE, "libfa_mi355.so")   # override: A/B of experimental builds
CSRC = os.path.join(_HERE, "csrc")

F16, BF16 = 0, 1
OUT_F32, OUT_SAME = 0, 1
ALGO_AUTO, ALGO_GENERIC, ALGO_TILED, ALGO_INTERLEAVED, ALGO_INTERLEAVED_2WG = 0, 1, 2, 5, 6
ALGO_RP, ALGO_RP_FOLD, ALGO_RP16, ALGO_RP16_FOLD = 21, 22, 23, 24
ALGO_RP16_DMA = 25
ALGO_RP16_FOLD_HALF, ALGO_RP16_FOLD_QUARTER, ALGO_RP16_FOLD_1W, ALGO_RP16_FOLD_KS2 = 26, 27, 28, 29

KV_16BIT, KV_FP8_E4M3 = 0, 1
MLA_DC, MLA_DR, MLA_DQK = 512, 64, 576   # FA_MLA_*: a latent row's compressed and rotary parts, and its width
ATTEND_SHORT, ATTEND_LONG = 1, 2   # the parts of fa_kvcache_attend_varlen_part


class KvDecodeDesc(C.Structure):
    """fa_kvdecode_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p), ("lse", C.c_void_p),
                ("seqlens_k", C.c_void_p), ("block_table", C.c_void_p), ("k_scale", C.c_void_p), ("v_scale", C.c_void_p),
                ("sinks", C.c_void_p), ("kv_dtype", C.c_int), ("B", C.c_int), ("Hkv", C.c_int), ("G", C.c_int), ("Nq", C.c_int),
                ("d", C.c_int), ("Ncap", C.c_int), ("num_pages", C.c_int), ("page_size", C.c_int), ("max_pages", C.c_int),
                ("scale", C.c_float), ("causal", C.c_int), ("window", C.c_int), ("softcap", C.c_float), ("in_dtype", C.c_int),
                ("out_dtype", C.c_int), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
                ("seqlens_q", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvDecodeDesc)


class KvAppendDesc(C.Structure):
    """fa_kvappend_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Knew", C.c_void_p), ("Vnew", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p),
                ("seqlens_k", C.c_void_p), ("seqlens_out", C.c_void_p), ("seqlens_new", C.c_void_p), ("block_table", C.c_void_p),
                ("k_scale", C.c_void_p), ("v_scale", C.c_void_p), ("Q", C.c_void_p), ("Qout", C.c_void_p), ("rope_cos", C.c_void_p),
                ("rope_sin", C.c_void_p), ("kv_dtype", C.c_int), ("B", C.c_int), ("Hkv", C.c_int), ("Nnew", C.c_int), ("d", C.c_int),
                ("Ncap", C.c_int), ("num_pages", C.c_int), ("page_size", C.c_int), ("max_pages", C.c_int), ("G", C.c_int),
                ("rot_dim", C.c_int), ("max_pos", C.c_int), ("interleaved", C.c_int), ("dtype", C.c_int), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvAppendDesc)


class KvAppendVarlenDesc(C.Structure):
    """fa_kvappend_varlen_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Knew", C.c_void_p), ("Vnew", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p),
                ("cu_seqlens_new", C.c_void_p), ("seqlens_k", C.c_void_p), ("seqlens_out", C.c_void_p), ("block_table", C.c_void_p),
                ("k_scale", C.c_void_p), ("v_scale", C.c_void_p), ("Q", C.c_void_p), ("Qout", C.c_void_p), ("rope_cos", C.c_void_p),
                ("rope_sin", C.c_void_p), ("kv_dtype", C.c_int), ("B", C.c_int), ("Hkv", C.c_int), ("d", C.c_int), ("total_new", C.c_int),
                ("Ncap", C.c_int), ("num_pages", C.c_int), ("page_size", C.c_int), ("max_pages", C.c_int), ("G", C.c_int),
                ("rot_dim", C.c_int), ("max_pos", C.c_int), ("interleaved", C.c_int), ("dtype", C.c_int),
                ("k_stride_t", C.c_longlong), ("k_stride_h", C.c_longlong), ("v_stride_t", C.c_longlong), ("v_stride_h", C.c_longlong),
                ("q_stride_t", C.c_longlong), ("q_stride_h", C.c_longlong), ("qo_stride_t", C.c_longlong), ("qo_stride_h", C.c_longlong),
                ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvAppendVarlenDesc)


def new_desc(cls):
    """A zeroed descriptor with its `size` set, to be filled by fill(desc, field=value, ...).  The pair is the per-call path of
    ops._decode and ops._append: Structure's own keyword initialiser costs half of what cls(**fields) costs through the Python-level
    __init__ above, and that difference is what a decode or append call may cost over the flat entries' positional call
    (profiles/frontend_refactor.txt)."""
    desc = cls.__new__(cls)
    desc.size = C.sizeof(cls)
    return desc


fill = C.Structure.__init__


MERGE_MAX_PARTS = 16
STATE_F16, STATE_BF16, STATE_F32 = 0, 1, 2


class StatePart(C.Structure):
    """fa_state_part of include/fa_mi355.h: one (O, lse) pair and its two row strides."""
    _fields_ = [("O", C.c_void_p), ("lse", C.c_void_p), ("stride_b", C.c_longlong), ("stride_h", C.c_longlong)]


class MergeDesc(C.Structure):
    """fa_merge_desc of include/fa_mi355.h, field for field; `size` is filled in.  `parts` takes a sequence of up to MERGE_MAX_PARTS
    StatePart (or (O, lse, stride_b, stride_h) tuples); the rest stay zero."""
    _fields_ = [("size", C.c_size_t), ("parts", StatePart * MERGE_MAX_PARTS), ("R", C.c_int), ("B", C.c_int), ("H", C.c_int),
                ("rows", C.c_int), ("d", C.c_int), ("part_dtype", C.c_int), ("O", C.c_void_p), ("lse", C.c_void_p),
                ("out_dtype", C.c_int), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        parts = fields.pop("parts", ())
        super().__init__(**fields)
        for i, p in enumerate(parts):
            self.parts[i] = p if isinstance(p, StatePart) else StatePart(*p)
        if "size" not in fields:
            self.size = C.sizeof(MergeDesc)


class VarlenDesc(C.Structure):
    """fa_varlen_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p), ("lse", C.c_void_p),
                ("cu_seqlens_q", C.c_void_p), ("cu_seqlens_k", C.c_void_p), ("B", C.c_int), ("Hkv", C.c_int), ("G", C.c_int),
                ("d", C.c_int), ("total_q", C.c_int), ("total_k", C.c_int), ("q_stride_t", C.c_longlong), ("q_stride_h", C.c_longlong),
                ("k_stride_t", C.c_longlong), ("k_stride_h", C.c_longlong), ("v_stride_t", C.c_longlong), ("v_stride_h", C.c_longlong),
                ("o_stride_t", C.c_longlong), ("o_stride_h", C.c_longlong), ("scale", C.c_float), ("causal", C.c_int),
                ("in_dtype", C.c_int), ("out_dtype", C.c_int), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(VarlenDesc)


class VarlenOpts(C.Structure):
    """fa_varlen_opts of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("sinks", C.c_void_p), ("window", C.c_int), ("softcap", C.c_float)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(VarlenOpts)


class VarlenKvcacheDesc(C.Structure):
    """fa_varlen_kvcache_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Q", C.c_void_p), ("O", C.c_void_p), ("lse", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p),
                ("cu_seqlens_q", C.c_void_p), ("seqlens_k", C.c_void_p), ("block_table", C.c_void_p), ("B", C.c_int), ("Hkv", C.c_int),
                ("G", C.c_int), ("d", C.c_int), ("total_q", C.c_int), ("Ncap", C.c_int), ("num_pages", C.c_int),
                ("page_size", C.c_int), ("max_pages", C.c_int), ("q_stride_t", C.c_longlong), ("q_stride_h", C.c_longlong),
                ("o_stride_t", C.c_longlong), ("o_stride_h", C.c_longlong), ("scale", C.c_float), ("causal", C.c_int),
                ("in_dtype", C.c_int), ("out_dtype", C.c_int), ("sinks", C.c_void_p), ("window", C.c_int), ("softcap", C.c_float),
                ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(VarlenKvcacheDesc)


class KvDecodeVarlenDesc(C.Structure):
    """fa_kvdecode_varlen_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Q", C.c_void_p), ("O", C.c_void_p), ("lse", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p),
                ("cu_seqlens_q", C.c_void_p), ("seqlens_k", C.c_void_p), ("block_table", C.c_void_p), ("k_scale", C.c_void_p),
                ("v_scale", C.c_void_p), ("sinks", C.c_void_p), ("kv_dtype", C.c_int), ("B", C.c_int), ("Hkv", C.c_int), ("G", C.c_int),
                ("d", C.c_int), ("total_q", C.c_int), ("max_q", C.c_int), ("Ncap", C.c_int), ("num_pages", C.c_int),
                ("page_size", C.c_int), ("max_pages", C.c_int), ("q_stride_t", C.c_longlong), ("q_stride_h", C.c_longlong),
                ("o_stride_t", C.c_longlong), ("o_stride_h", C.c_longlong), ("scale", C.c_float), ("causal", C.c_int),
                ("window", C.c_int), ("softcap", C.c_float), ("in_dtype", C.c_int), ("out_dtype", C.c_int), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvDecodeVarlenDesc)


class KvDecodeTreeOpts(C.Structure):
    """fa_kvdecode_tree_opts of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("tree_mask", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvDecodeTreeOpts)


class KvAppendVarlenOpts(C.Structure):
    """fa_kvappend_varlen_opts of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("positions", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvAppendVarlenOpts)


class KvCommitDesc(C.Structure):
    """fa_kvcommit_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("K", C.c_void_p), ("V", C.c_void_p), ("seqlens_k", C.c_void_p), ("seqlens_out", C.c_void_p),
                ("accept_mask", C.c_void_p), ("block_table", C.c_void_p), ("kv_dtype", C.c_int), ("dtype", C.c_int), ("B", C.c_int),
                ("Hkv", C.c_int), ("d", C.c_int), ("max_new", C.c_int), ("Ncap", C.c_int), ("num_pages", C.c_int),
                ("page_size", C.c_int), ("max_pages", C.c_int), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(KvCommitDesc)


class MlaDecodeDesc(C.Structure):
    """fa_mla_decode_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Q", C.c_void_p), ("O", C.c_void_p), ("lse", C.c_void_p), ("C", C.c_void_p),
                ("cu_seqlens_q", C.c_void_p), ("seqlens_k", C.c_void_p), ("block_table", C.c_void_p), ("B", C.c_int), ("Hq", C.c_int),
                ("total_q", C.c_int), ("max_q", C.c_int), ("Ncap", C.c_int), ("num_pages", C.c_int), ("page_size", C.c_int),
                ("max_pages", C.c_int), ("q_stride_t", C.c_longlong), ("q_stride_h", C.c_longlong), ("o_stride_t", C.c_longlong),
                ("o_stride_h", C.c_longlong), ("scale", C.c_float), ("causal", C.c_int), ("num_splits", C.c_int), ("in_dtype", C.c_int),
                ("out_dtype", C.c_int), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(MlaDecodeDesc)


class MlaAppendDesc(C.Structure):
    """fa_mla_append_desc of include/fa_mi355.h, field for field; `size` is filled in."""
    _fields_ = [("size", C.c_size_t), ("Cnew", C.c_void_p), ("C", C.c_void_p), ("cu_seqlens_new", C.c_void_p), ("seqlens_k", C.c_void_p),
                ("seqlens_out", C.c_void_p), ("block_table", C.c_void_p), ("B", C.c_int), ("total_new", C.c_int),
                ("new_stride_t", C.c_longlong), ("Ncap", C.c_int), ("num_pages", C.c_int), ("page_size", C.c_int), ("max_pages", C.c_int),
                ("dtype", C.c_int), ("stream", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(**fields)
        if "size" not in fields:
            self.size = C.sizeof(MlaAppendDesc)


def _signatures() -> dict:
    """{symbol: (restype, argtypes)} of every function include/fa_mi355.h declares."""
    vp, i, f, sz, s = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_char_p
    sig = {
        "flashattn_forward_wmma": (i, [vp, vp, vp, vp, i, i, i, f, vp]),
        "fa_forward": (i, [vp, vp, vp, vp, i, i, i, i, f, i, i, vp]),
        "fa_forward_ex": (i, [vp, vp, vp, vp, i, i, i, i, f, i, i, i, vp]),
        "fa_forward_causal": (i, [vp, vp, vp, vp, i, i, i, i, f, i, i, i, vp]),
        "fa_forward_splitkv_workspace_bytes": (sz, [i, i, i, i, i]),
        "fa_forward_splitkv": (i, [vp, vp, vp, vp, i, i, i, i, i, f, i, i, vp, sz, vp]),
        "fa_debug_stage": (i, [i, vp, vp, vp, i, i, i, f, i, vp]),
        "flashattn_streaming_16x16_mw": (i, [vp, vp, vp, vp, i, i, f, vp]),
        "flashattn_streaming_16x16_mw_kt": (i, [vp, vp, vp, vp, i, i, f, vp]),
        "fa_mi355_version": (s, []),
        "fa_mi355_has_experiments": (i, []),
        "fa_selected_algo": (i, [i, i, i, i, i]),
        "fa_selected_kernel": (s, [i, i, i, i, i, i]),
        "fa_forward_kvcache_workspace_bytes": (sz, [i, i, i, i, i, i]),
        "fa_forward_kvcache_paged_workspace_bytes": (sz, [i, i, i, i, i, i, i]),
        # the windowed sizing functions: the base one's list with `int window` at the end
        "fa_forward_kvcache_window_workspace_bytes": (sz, [i, i, i, i, i, i, i]),
        "fa_forward_kvcache_paged_window_workspace_bytes": (sz, [i, i, i, i, i, i, i, i]),
        # the descriptor form of the eight decode entries, with sinks, softcap and seqlens_q
        "fa_kvcache_decode_workspace_bytes": (sz, [C.POINTER(KvDecodeDesc)]),
        "fa_kvcache_decode": (i, [C.POINTER(KvDecodeDesc)]),
        # the descriptor form of the eight append entries, with seqlens_new
        "fa_kvcache_append_ex": (i, [C.POINTER(KvAppendDesc)]),
        # the same eight forms on token-packed (cu_seqlens) sources read through their strides
        "fa_kvcache_append_varlen": (i, [C.POINTER(KvAppendVarlenDesc)]),
        "fa_merge_states": (i, [C.POINTER(MergeDesc)]),
        "fa_forward_varlen": (i, [C.POINTER(VarlenDesc)]),
        # the same with a window, a soft-cap and sinks; a null opts is fa_forward_varlen
        "fa_forward_varlen_ex": (i, [C.POINTER(VarlenDesc), C.POINTER(VarlenOpts)]),
        # the same with K/V in the KV cache, contiguous or paged
        "fa_forward_varlen_kvcache": (i, [C.POINTER(VarlenKvcacheDesc)]),
        # the same on an e4m3fn cache: the descriptor as it is, then k_scale, v_scale
        "fa_forward_varlen_kvcache_fp8": (i, [C.POINTER(VarlenKvcacheDesc), vp, vp]),
        # split-KV decode on token-packed (cu_seqlens) Q, O and lse: the read half of fa_kvcache_append_varlen
        "fa_kvcache_decode_varlen_workspace_bytes": (sz, [C.POINTER(KvDecodeVarlenDesc)]),
        "fa_kvcache_decode_varlen": (i, [C.POINTER(KvDecodeVarlenDesc)]),
        # the same with one 64-bit ancestor word per token row (tree speculation); a null opts is fa_kvcache_decode_varlen
        "fa_kvcache_decode_varlen_ex": (i, [C.POINTER(KvDecodeVarlenDesc), C.POINTER(KvDecodeTreeOpts)]),
        # the mixed prefill + decode step on the same descriptor: max_q is the routing threshold; parts: ATTEND_SHORT | ATTEND_LONG
        "fa_kvcache_attend_varlen": (i, [C.POINTER(KvDecodeVarlenDesc)]),
        "fa_kvcache_attend_varlen_part": (i, [C.POINTER(KvDecodeVarlenDesc), i]),
        # the packed append with explicit rotary positions; a null opts is fa_kvcache_append_varlen
        "fa_kvcache_append_varlen_ex": (i, [C.POINTER(KvAppendVarlenDesc), C.POINTER(KvAppendVarlenOpts)]),
        # the commit of a tree step: the accepted path's K/V rows to consecutive slots, one 64-bit word per sequence
        "fa_kvcache_commit": (i, [C.POINTER(KvCommitDesc)]),
        # MLA: absorbed-query decode over a latent cache [.., 576] (O from its first 512 elements) and the copy that fills the cache
        "fa_mla_decode_workspace_bytes": (sz, [C.POINTER(MlaDecodeDesc)]),
        "fa_mla_decode": (i, [C.POINTER(MlaDecodeDesc)]),
        "fa_mla_append": (i, [C.POINTER(MlaAppendDesc)]),
        # the same on a latent cache of e4m3fn codes [.., 576 bytes]: the descriptor as it is, then c_scale (one float on the device)
        "fa_mla_decode_fp8_workspace_bytes": (sz, [C.POINTER(MlaDecodeDesc)]),
        "fa_mla_decode_fp8": (i, [C.POINTER(MlaDecodeDesc), vp]),
        "fa_mla_append_fp8": (i, [C.POINTER(MlaAppendDesc), vp]),
    }
    for paged in (False, True):
        for fp8 in (False, True):
            layout = "_paged" * paged + "_fp8" * fp8
            geometry = [i] * (3 if paged else 1)   # Ncap, or of a pool: num_pages, page_size, max_pages
            # the eight decode entries, from one rule: Q, K, V, O, lse, seqlens [, table] [, k_scale, v_scale], B, Hkv, G, Nq, geometry,
            # d, scale, causal [, window], in_dtype, out_dtype, workspace, workspace_bytes, stream
            for window in (False, True):
                sig["fa_forward_kvcache" + layout + "_window" * window] = (
                    i, [vp] * (6 + paged + 2 * fp8) + [i] * 4 + geometry + [i, f, i] + [i] * window + [i, i, vp, sz, vp])
            # the eight append entries, from one rule: Knew, Vnew, K, V, seqlens_k, seqlens_out [, table] [, k_scale, v_scale]
            # [, Q, Qout, rope_cos, rope_sin], B, Hkv, Nnew, geometry, d [, G, rot_dim, max_pos, interleaved], dtype, stream
            for rope in (False, True):
                sig["fa_kvcache_append" + layout + "_rope" * rope] = (
                    i, [vp] * (6 + paged + 2 * fp8 + 4 * rope) + [i] * 3 + geometry + [i] + [i] * (4 * rope) + [i, vp])
    for name in ("fa_forward_kvcache_paged_workspace_bytes", "fa_forward_kvcache_paged"):
        sig[name] = sig.pop(name)   # SYMBOLS ends with this pair, as it always has (tests/test_kvcache_paged_host.py)
    return sig


SIGNATURES = _signatures()
SYMBOLS = tuple(SIGNATURES)   # every symbol include/fa_mi355.h declares


class FaError(RuntimeError):
    """A launcher returned a non-zero hipError_t."""

    def __init__(self, fn: str, code: int):
        super().__init__(f"{fn} failed with hipError_t {code}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile libfa_mi355.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def _share_torch_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64 (soname libamdhip64.so.7).  Device
    pointers and stream handles are only meaningful inside ONE HIP runtime, so that copy must be
    in the process before libfa_mi355.so is loaded: its DT_NEEDED libamdhip64.so.7 then binds to
    it by soname instead of pulling /opt/rocm's copy in as a second runtime (which sees no device:
    hipErrorNoDevice).  A pure C/C++ host (bench/fa_bench) links /opt/rocm's runtime directly."""
    try:
        import torch
    except ImportError:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib() -> C.CDLL:
    """Load the HIP library.  No fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C flashattention_kernel_project_amd/csrc`")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def version() -> str:
    return lib().fa_mi355_version().decode()


def check(fn: str, code: int) -> None:
    if code != 0:
        raise FaError(fn, code)
