"""Attention of a decode step over a KV cache kept in 8-bit floating point, over the C ABI of the eleventh library
(include/nnop_hip_decode_attn_fp8.h; no counterpart in the reference): decode_attention with K and V as one-byte OCP E4M3 codes and one
float32 scale per KV head each.  The codes are read where they lie and expanded in registers, exactly; q, o and the arithmetic are
decode_attention's.

    o = decode_attention_fp8(q, k_cache, v_cache, seqlens, *, k_scale=None, v_scale=None, window_left=None, sinks=None, num_splits=None,
                             return_lse=False, workspace=None)                  # o, or (o, lse)
    decode_attention_fp8_into(o, lse, q, k_cache, v_cache, seqlens, ...)        # caller-owned buffers: the form for captured graphs
    splits, workspace_bytes = decode_attention_fp8_plan(q, k_cache, v_cache, window_left=None, num_splits=None)

q [B, QH, QL, E] float16 or bfloat16, contiguous; k_cache, v_cache [B, KH, cap, E] of torch.float8_e4m3fn, or of uint8 taken as the same
codes, with any strides whose last is 1 and whose others are multiples of 16 -- a [B, cap, KH, E] cache is passed as
`cache.transpose(1, 2)`, never copied; k_scale, v_scale [KH] float32 on the device or None (= 1): the value of a cache element is its
code's value times the scale of its KV head; seqlens, sinks, o, lse, the alignment, the window and the dead rows as in decode_attention.

x = (q . code(k)) (k_scale / sqrt(E)), one factor applied to the float32 scores, so sinks and lse are in the domain of the scaled
scores; o = v_scale sum softmax(x) code(v), scaled in float32 in front of its one rounding.  A NaN code in a row a query sees gives NaN.
The contracts are decode_attention's (the header states them in full), the scales included in what a replayed graph may change.

Writing the new rows into the cache is the caller's: `(x / scale).to(torch.float8_e4m3fn)`.  No autograd, GPU-only, no fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_decode_attn_fp8
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_decode_attn_fp8 import EMBS, KV_E4M3, MAX_ROWS, MAX_SPLITS, DecodeAttnFp8Desc

__all__ = ["decode_attention_fp8", "decode_attention_fp8_into", "decode_attention_fp8_plan"]

FN = "decode_attention_fp8"
CACHE_DTYPES = (torch.float8_e4m3fn, torch.uint8)


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
    """byte strides (b, kvh, j) of a cache of one-byte elements; a dimension of one row has no stride of its own"""
    if t.stride(3) != 1:
        raise NNopError(f"{FN}: {name} must be contiguous in its last dimension", _lib.NNOP_ERR_SHAPE)
    strides = tuple(t.stride(i) if t.size(i) > 1 else E for i in range(3))
    if any(s < E or s % 16 for s in strides):
        raise NNopError(f"{FN}: the strides of {name} must be multiples of 16 and at least a row, got {t.stride()}", _lib.NNOP_ERR_SHAPE)
    return strides


def _desc(q, k_cache, v_cache, window_left, num_splits):
    """every host check of q and the caches -> the descriptor"""
    _tensor("q", q, 4), _tensor("k_cache", k_cache, 4), _tensor("v_cache", v_cache, 4)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: q must be float16 or bfloat16, got {_dtype_name(q.dtype)}", _lib.NNOP_ERR_DTYPE)
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype not in CACHE_DTYPES or t.device != q.device:
            raise NNopError(f"{FN}: {name} must be float8_e4m3fn (or uint8 holding those codes) on q's device, got "
                            f"{_dtype_name(t.dtype)}; decode_attention takes a 16-bit cache", _lib.NNOP_ERR_DTYPE)
    if any(t.requires_grad for t in (q, k_cache, v_cache)) and torch.is_grad_enabled():
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
    return DecodeAttnFp8Desc(dtype=_DTYPES[q.dtype], emb=E, ql=QL, qh=QH, kh=KH, batch=B, capacity=cap, window_left=w, splits=s, flags=0,
                             kv_format=KV_E4M3, reserved=0,
                             k_stride_b=ks[0], k_stride_h=ks[1], k_stride_l=ks[2], v_stride_b=vs[0], v_stride_h=vs[1], v_stride_l=vs[2])


def _plan(d):
    splits, nbytes = C.c_int32(0), C.c_size_t(0)
    _raise(_lib_decode_attn_fp8.load().nnop_decode_attn_fp8_plan(C.byref(d), C.byref(splits), C.byref(nbytes)))
    return splits.value, nbytes.value


def _side(name, t, shape, dtype, like):
    _tensor(name, t, len(shape))
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise NNopError(f"{FN}: {name} must be a contiguous {_dtype_name(dtype)} tensor of shape {tuple(shape)} on q's device, got "
                        f"{_dtype_name(t.dtype)} {tuple(t.shape)}", _lib.NNOP_ERR_SHAPE)


def decode_attention_fp8_plan(q, k_cache, v_cache, *, window_left=None, num_splits=None):
    """(splits, workspace_bytes) the call will use for these tensors: host-only, from shapes alone; decode_attention_plan's figures."""
    return _plan(_desc(q, k_cache, v_cache, window_left, num_splits))


def _run(d, o, lse, q, k_cache, v_cache, k_scale, v_scale, seqlens, sinks, workspace):
    """the checks of everything but q and the caches (those made `d`), the workspace, the call"""
    B, QH, QL, E = q.shape
    _side("o", o, q.shape, q.dtype, q)
    if lse is not None:
        _side("lse", lse, (B, QH, QL), torch.float32, q)
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is not None:
            _side(name, t, (d.kh,), torch.float32, q)
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
        _raise(_lib_decode_attn_fp8.load().nnop_decode_attn_fp8(C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(k_cache), _ptr(v_cache),
                                                                _ptr(k_scale), _ptr(v_scale), _ptr(seqlens), _ptr(sinks), _ptr(workspace),
                                                                have, _stream(q)))
    return o if lse is None else (o, lse)


def decode_attention_fp8_into(o, lse, q, k_cache, v_cache, seqlens, *, k_scale=None, v_scale=None, window_left=None, sinks=None,
                              num_splits=None, workspace=None):
    """Writes o (like q) and, unless it is None, lse [B, QH, QL] float32.  With a `workspace` of decode_attention_fp8_plan's size nothing
    is allocated: the form for captured graphs."""
    return _run(_desc(q, k_cache, v_cache, window_left, num_splits), o, lse, q, k_cache, v_cache, k_scale, v_scale, seqlens, sinks, workspace)


def decode_attention_fp8(q, k_cache, v_cache, seqlens, *, k_scale=None, v_scale=None, window_left=None, sinks=None, num_splits=None,
                         return_lse=False, workspace=None):
    """o [B, QH, QL, E], or (o, lse [B, QH, QL] float32): the QL new tokens of every sequence against its 8-bit cache."""
    d = _desc(q, k_cache, v_cache, window_left, num_splits)
    with _on_device(q):
        o = torch.empty_like(q)
        lse = torch.empty(q.shape[:3], dtype=torch.float32, device=q.device) if return_lse else None
    return _run(d, o, lse, q, k_cache, v_cache, k_scale, v_scale, seqlens, sinks, workspace)
