"""Attention of a decode step over a KV cache, over the C ABI of the tenth library (include/nnop_hip_decode_attn.h; no counterpart in the
reference): QL new tokens per sequence (1; 2 ... for speculative decoding) against that sequence's cache, forward only.

    o = decode_attention(q, k_cache, v_cache, seqlens, *, window_left=None, sinks=None, num_splits=None, return_lse=False,
                         workspace=None)                                        # o, or (o, lse)
    decode_attention_into(o, lse, q, k_cache, v_cache, seqlens, ...)            # caller-owned buffers: the form for captured graphs
    splits, workspace_bytes = decode_attention_plan(q, k_cache, v_cache, window_left=None, num_splits=None)

q [B, QH, QL, E] contiguous; k_cache, v_cache [B, KH, cap, E] with any strides whose last is 1 -- a [B, cap, KH, E] cache is passed as
`cache.transpose(1, 2)`, never copied; seqlens [B] int32 on the device: the valid keys of each sequence INCLUDING the QL new ones (the
caller has written them into the cache); sinks [QH] float32, one more softmax column per query head without a value vector; o like q, lse
[B, QH, QL] float32.  float16 or bfloat16, E 64 or 128, (QH / KH) QL <= 16.

Alignment is bottom-right: query i of sequence b stands at p = seqlens[b] - QL + i and sees key j iff 0 <= j <= p and (window_left is
None or j >= p - window_left).  Scale 1 / sqrt(E).  A row that sees no key gives o = 0 and lse = its sink (-inf without one), not the NaN
of flash_attention's dead rows: padded sequences of length 0 are routine in a captured decode batch.

Contracts (the header states them in full): seqlens is read on the device and the grid depends on host values alone, so a captured
call can be replayed after seqlens and the cache have changed; no sync, no allocation inside the call, no atomics, two runs bitwise
equal; masking by selection -- nothing of a cache row that no query of its sequence sees enters a result, NaN or inf included; the bits
of a sequence's rows do not depend on the batch around it; fp32 scores, softmax and accumulation, one rounding of o.

There is no autograd: a tensor that requires a gradient raises -- use flash_attention for training.  GPU-only: no CPU or PyTorch
fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_decode_attn
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_decode_attn import EMBS, MAX_ROWS, MAX_SPLITS, DecodeAttnDesc

__all__ = ["decode_attention", "decode_attention_into", "decode_attention_plan"]

FN = "decode_attention"


def _tensor(name, t, dims):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{FN}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise NNopError(f"{FN} is GPU-only: {name} is on {t.device}")
    if t.dim() != dims:
        raise NNopError(f"{FN}: {name} must have {dims} dimensions, got {t.dim()}", _lib.NNOP_ERR_SHAPE)


def _int(name, x, lo):
    if isinstance(x, bool) or not isinstance(x, int):
        raise TypeError(f"{FN}: {name} must be None or an int, got {x!r}")
    if x < lo:
        raise ValueError(f"{FN}: {name} must be >= {lo}, got {x}")
    return x


def _cache_strides(name, t, E):
    """element strides (b, kvh, j) of a cache; a dimension of one row has no stride of its own"""
    if t.stride(3) != 1:
        raise NNopError(f"{FN}: {name} must be contiguous in its last dimension", _lib.NNOP_ERR_SHAPE)
    strides = tuple(t.stride(i) if t.size(i) > 1 else E for i in range(3))
    if any(s < E or s % 8 for s in strides):
        raise NNopError(f"{FN}: the strides of {name} must be multiples of 8 elements and at least a row, got {t.stride()}",
                        _lib.NNOP_ERR_SHAPE)
    return strides


def _desc(q, k_cache, v_cache, window_left, num_splits):
    """every host check of q and the caches -> the descriptor"""
    _tensor("q", q, 4), _tensor("k_cache", k_cache, 4), _tensor("v_cache", v_cache, 4)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: q must be float16 or bfloat16, got {_dtype_name(q.dtype)}", _lib.NNOP_ERR_DTYPE)
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype != q.dtype or t.device != q.device:
            raise NNopError(f"{FN}: {name} must have q's dtype and device", _lib.NNOP_ERR_DTYPE)
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in (q, k_cache, v_cache)) and torch.is_grad_enabled():
        raise NNopError(f"{FN} has no backward: use flash_attention for a tensor that requires a gradient")
    B, QH, QL, E = q.shape
    if not q.is_contiguous():
        raise NNopError(f"{FN}: q must be contiguous", _lib.NNOP_ERR_SHAPE)
    if E not in EMBS:
        raise NNopError(f"{FN}: the head dimension must be 64 or 128, got {E}", _lib.NNOP_ERR_SHAPE)
    if k_cache.shape != v_cache.shape or k_cache.size(0) != B or k_cache.size(3) != E:
        raise NNopError(f"{FN}: k_cache and v_cache must both be [B, KH, cap, E] = [{B}, KH, cap, {E}], got {tuple(k_cache.shape)} and "
                        f"{tuple(v_cache.shape)}", _lib.NNOP_ERR_SHAPE)
    KH, cap = k_cache.size(1), k_cache.size(2)
    if B < 1 or KH < 1 or QH % KH or QL < 1 or (QH // KH) * QL > MAX_ROWS or cap < QL:
        raise NNopError(f"{FN}: QH must be a multiple of KH, (QH / KH) QL must be at most {MAX_ROWS} and the cache must hold the QL new "
                        f"tokens; got QH {QH}, KH {KH}, QL {QL}, cap {cap}", _lib.NNOP_ERR_SHAPE)
    w = -1 if window_left is None else min(_int("window_left", window_left, 0), cap)       # a window beyond the cache removes no key
    s = 0 if num_splits is None else _int("num_splits", num_splits, 1)
    if s > MAX_SPLITS:
        raise ValueError(f"{FN}: num_splits must be at most {MAX_SPLITS}, got {s}")
    ks, vs = _cache_strides("k_cache", k_cache, E), _cache_strides("v_cache", v_cache, E)
    return DecodeAttnDesc(dtype=_DTYPES[q.dtype], emb=E, ql=QL, qh=QH, kh=KH, batch=B, capacity=cap, window_left=w, splits=s, flags=0,
                          k_stride_b=ks[0], k_stride_h=ks[1], k_stride_l=ks[2], v_stride_b=vs[0], v_stride_h=vs[1], v_stride_l=vs[2])


def _plan(d):
    splits, nbytes = C.c_int32(0), C.c_size_t(0)
    _raise(_lib_decode_attn.load().nnop_decode_attn_plan(C.byref(d), C.byref(splits), C.byref(nbytes)))
    return splits.value, nbytes.value


def _side(name, t, shape, dtype, like):
    _tensor(name, t, len(shape))
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise NNopError(f"{FN}: {name} must be a contiguous {_dtype_name(dtype)} tensor of shape {tuple(shape)} on q's device, got "
                        f"{_dtype_name(t.dtype)} {tuple(t.shape)}", _lib.NNOP_ERR_SHAPE)


def decode_attention_plan(q, k_cache, v_cache, *, window_left=None, num_splits=None):
    """(splits, workspace_bytes) the call will use for these tensors: host-only, from shapes alone."""
    return _plan(_desc(q, k_cache, v_cache, window_left, num_splits))


def _run(d, o, lse, q, k_cache, v_cache, seqlens, sinks, workspace):
    """the checks of everything but q and the caches (those made `d`), the workspace, the call"""
    B, QH, QL, E = q.shape
    _side("o", o, q.shape, q.dtype, q)
    if lse is not None:
        _side("lse", lse, (B, QH, QL), torch.float32, q)
    _side("seqlens", seqlens, (B,), torch.int32, q)
    if sinks is not None:
        _side("sinks", sinks, (QH,), torch.float32, q)
    splits, need = _plan(d)
    with _on_device(q):
        if workspace is None and need:
            workspace = torch.empty(need // 4, dtype=torch.float32, device=q.device)
        have = 0
        if workspace is not None:
            if not isinstance(workspace, torch.Tensor) or workspace.device != q.device or not workspace.is_contiguous():
                raise NNopError(f"{FN}: workspace must be a contiguous tensor on q's device", _lib.NNOP_ERR_WORKSPACE)
            have = workspace.numel() * workspace.element_size()
        _raise(_lib_decode_attn.load().nnop_decode_attn(C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(seqlens),
                                                        _ptr(sinks), _ptr(workspace), have, _stream(q)))
    return o if lse is None else (o, lse)


def decode_attention_into(o, lse, q, k_cache, v_cache, seqlens, *, window_left=None, sinks=None, num_splits=None, workspace=None):
    """Writes o (like q) and, unless it is None, lse [B, QH, QL] float32.  With a `workspace` of decode_attention_plan's size nothing is
    allocated: the form for captured graphs."""
    return _run(_desc(q, k_cache, v_cache, window_left, num_splits), o, lse, q, k_cache, v_cache, seqlens, sinks, workspace)


def decode_attention(q, k_cache, v_cache, seqlens, *, window_left=None, sinks=None, num_splits=None, return_lse=False, workspace=None):
    """o [B, QH, QL, E], or (o, lse [B, QH, QL] float32): the QL new tokens of every sequence against its cache, bottom-right aligned."""
    d = _desc(q, k_cache, v_cache, window_left, num_splits)
    with _on_device(q):
        o = torch.empty_like(q)
        lse = torch.empty(q.shape[:3], dtype=torch.float32, device=q.device) if return_lse else None
    return _run(d, o, lse, q, k_cache, v_cache, seqlens, sinks, workspace)
