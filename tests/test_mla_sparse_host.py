"""CPU tier of fa_mla_decode_sparse through the C ABI: the symbols are exported and bound, the refusals the header lists hold before
the device is touched, and the sizing function follows (B, Hq, max_q, topk, num_splits).  Only calls that must be rejected are issued;
the descriptor is tests/test_mla_host.py's, which passes every check of fa_mla_decode but the workspace's."""
import ctypes

import pytest

import test_mla_host as dense

INVALID = 1  # hipErrorInvalidValue
TOPK = 200   # ceil(200 / 64) = 4 tiles


def _call(fa, indices=4096, topk=TOPK, stride=None, **kw):
    kw.setdefault("num_splits", 1)
    return fa.lib().fa_mla_decode_sparse(ctypes.byref(dense._desc(fa, **kw)), indices, topk, topk if stride is None else stride)


def _bytes(fa, topk=TOPK, paged=False, **kw):
    return fa.lib().fa_mla_decode_sparse_workspace_bytes(ctypes.byref(dense._desc(fa, paged, **kw)), topk)


def test_symbols_and_front_ends(fa):
    raw, L, D = ctypes.CDLL(fa.capi.LIB_PATH), fa.lib(), ctypes.POINTER(fa.capi.MlaDecodeDesc)
    for n in ("fa_mla_decode_sparse_workspace_bytes", "fa_mla_decode_sparse"):
        assert n in fa.capi.SYMBOLS and hasattr(raw, n), n
    assert L.fa_mla_decode_sparse.argtypes == [D, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong]
    assert L.fa_mla_decode_sparse_workspace_bytes.argtypes == [D, ctypes.c_int]
    assert L.fa_mla_decode_sparse_workspace_bytes.restype is ctypes.c_size_t
    for name in ("fa_mla_decode_sparse", "mla_decode_sparse_workspace_bytes"):
        assert callable(getattr(fa, name)) and name in fa.__all__


REFUSED = [
    dict(indices=None), dict(indices=4098),          # NULL, not 4-byte aligned
    dict(topk=0), dict(topk=(1 << 20) + 1),
    dict(stride=TOPK - 1),
    dict(num_splits=5),                              # ceil(200 / 64) + 1
    dict(Hq=129),                                    # one of fa_mla_decode's: the shared checks run
]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_rejected_before_the_device(fa, bad):
    assert _call(fa, **bad) == INVALID
    assert _call(fa, workspace=4096, workspace_bytes=1 << 40, **bad) == INVALID   # not for want of a workspace


def test_workspace(fa):
    assert _bytes(fa, num_splits=1) == 0
    need = _bytes(fa, num_splits=3)
    assert need > 0 and _bytes(fa, paged=True, num_splits=3) == need == _bytes(fa, num_splits=3, Ncap=1 << 20)   # not the capacity's
    assert 3 * _bytes(fa, num_splits=2) == 2 * need
    assert _bytes(fa, num_splits=3, Hq=129) == 0 and _bytes(fa, num_splits=5) == 0 and _bytes(fa, topk=0, num_splits=1) == 0
    assert fa.mla_decode_sparse_workspace_bytes(2, 16, 2, TOPK, Ncap=256, num_splits=3) == need
    # the call stops at a missing, short or misaligned workspace, and only there
    assert _call(fa, num_splits=3) == INVALID
    assert _call(fa, num_splits=3, workspace=4096, workspace_bytes=need - 1) == INVALID
    assert _call(fa, num_splits=3, workspace=4100, workspace_bytes=need) == INVALID
    # the automatic choice: one pass for a short list on many workgroups, splits for a long list on few
    assert _bytes(fa, num_splits=0, B=64) == 0 and _bytes(fa, topk=2048, num_splits=0, B=1, max_q=1, total_q=1) > 0


def test_front_end_refuses_cpu_tensors_and_wrong_indices(fa):
    import torch
    q, c = torch.zeros(2, 4, 576, dtype=torch.float16), torch.zeros(2, 64, 576, dtype=torch.float16)
    cu, idx = torch.tensor([0, 1, 2], dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        fa.fa_mla_decode_sparse(q, c, idx, cu, 1)
    for bad in (idx.long(), idx[:1], idx.t().contiguous().t(), None):
        with pytest.raises(ValueError, match="indices"):
            fa.fa_mla_decode_sparse(q, c, bad, cu, 1)
