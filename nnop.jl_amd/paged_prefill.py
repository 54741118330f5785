"""Attention of a PREFILL step over a paged KV cache, over the C ABI of the thirteenth library (include/nnop_hip_paged_prefill.h; no
counterpart in the reference): a prompt behind a cached prefix, a chunk of a chunked prefill, speculative verification of more than 16
rows.  Every sequence brings its own number of new tokens; their queries are packed token-major and the keys and values -- the new
tokens' included, which the caller has written already -- are read from paged_decode_attention's pools where they lie.

    o = paged_prefill_attention(q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, window_left=None, sinks=None,
                                return_lse=False, workspace=None)                                   # o, or (o, lse)
    paged_prefill_attention_into(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, ...)   # caller-owned buffers: for captured graphs
    workspace_bytes = paged_prefill_attention_plan(q, k_pages, v_pages, block_table)                # 0: see below

q, o [T, QH, E], float16 or bfloat16, E 64 or 128, QH / KH <= 16, last stride 1, token and head strides multiples of 8 elements (a slice
of a fused QKV projection is not copied); lse [T, QH] float32.  k_pages, v_pages, block_table: paged_decode_attention's.  cu_seqlens_q
[B + 1] int32 on the device, non-decreasing from 0: sequence b owns tokens cu[b] ... cu[b + 1] - 1, n_b of them; entries are clamped into
[0, T] on the device.  seqlens [B] int32 on the device: the valid keys of each sequence INCLUDING its n_b new ones, clamped into
[0, max_pages page_size].  Query i of sequence b stands at p = seqlens[b] - n_b + i and sees keys max(0, p - window_left) ... p; the
scale is 1 / sqrt(E); a sink is one more column of the softmax; a row that sees no key (p < 0 included) has o = 0 and lse = its sink, or
-inf.  Never NaN.

Contracts (the header states them in full): paged_decode_attention's.  The grid comes from T, B, QH, KH, E alone and every length is read
on the device -- no sync, no allocation, no atomics, and a captured graph follows cu_seqlens_q, seqlens, the table and the pages at fixed
T and B.  Two runs are bitwise equal.  Masking is by selection: a pool row no query of its sequence sees may hold NaN.  Only table
entries of pages with a visible key are read, and every id is clamped into [0, P - 1] before it forms an address.  A sequence's bits do
not depend on P, on where its pages lie, on page_size or on the other sequences of the call.  A workgroup finds its block of tokens by a
search over cu_seqlens_q, so the workspace is 0 bytes; `workspace` is accepted for the shape of the decode calls and not used.

No autograd, GPU-only, no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_paged_prefill
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_paged_prefill import EMBS, MAX_GROUP, MIN_PAGE_SIZE, PagedPrefillDesc

__all__ = ["paged_prefill_attention", "paged_prefill_attention_into", "paged_prefill_attention_plan"]

FN = "paged_prefill_attention"


def _tensor(name, t, dims):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{FN}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise NNopError(f"{FN} is GPU-only: {name} is on {t.device}")
    if t.dim() != dims:
        raise NNopError(f"{FN}: {name} must have {dims} dimensions, got {t.dim()}", _lib.NNOP_ERR_SHAPE)


def _strides(name, t, floors):
    """element strides of every dimension but the last; a dimension of one row has none of its own and gets its floor"""
    if t.stride(-1) != 1:
        raise NNopError(f"{FN}: {name} must be contiguous in its last dimension", _lib.NNOP_ERR_SHAPE)
    strides = tuple(t.stride(i) if t.size(i) > 1 else f for i, f in enumerate(floors))
    if any(s < f or s % 8 for s, f in zip(strides, floors)):
        raise NNopError(f"{FN}: the strides of {name} must be multiples of 8 elements and at least {floors}, got {t.stride()}",
                        _lib.NNOP_ERR_SHAPE)
    return strides


def _desc(q, k_pages, v_pages, block_table, window_left, o=None):
    """every host check of q, o, the pools and the table -> the descriptor"""
    _tensor("q", q, 3), _tensor("k_pages", k_pages, 4), _tensor("v_pages", v_pages, 4), _tensor("block_table", block_table, 2)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: q must be float16 or bfloat16, got {_dtype_name(q.dtype)}", _lib.NNOP_ERR_DTYPE)
    for name, t in (("k_pages", k_pages), ("v_pages", v_pages)):
        if t.dtype != q.dtype or t.device != q.device:
            raise NNopError(f"{FN}: {name} must have q's dtype and device", _lib.NNOP_ERR_DTYPE)
    if block_table.dtype != torch.int32 or block_table.device != q.device:
        raise NNopError(f"{FN}: block_table must be int32 on q's device, got {_dtype_name(block_table.dtype)}", _lib.NNOP_ERR_DTYPE)
    if any(t.requires_grad for t in (q, k_pages, v_pages)) and torch.is_grad_enabled():
        raise NNopError(f"{FN} has no backward: use flash_attention for a tensor that requires a gradient")
    T, QH, E = q.shape
    if E not in EMBS:
        raise NNopError(f"{FN}: the head dimension must be 64 or 128, got {E}", _lib.NNOP_ERR_SHAPE)
    if k_pages.shape != v_pages.shape or k_pages.size(3) != E or k_pages.size(0) < 1:
        raise NNopError(f"{FN}: k_pages and v_pages must both be [P, KH, page_size, E] = [P, KH, page_size, {E}], got "
                        f"{tuple(k_pages.shape)} and {tuple(v_pages.shape)}", _lib.NNOP_ERR_SHAPE)
    P, KH, page = k_pages.shape[:3]
    if page < MIN_PAGE_SIZE or page & (page - 1):
        raise NNopError(f"{FN}: page_size must be a power of two, {MIN_PAGE_SIZE} or more, got {page}", _lib.NNOP_ERR_SHAPE)
    B, max_pages = block_table.shape
    if B < 1 or max_pages < 1 or max_pages * page > 2 ** 31 - 1:
        raise NNopError(f"{FN}: block_table must be [B, max_pages] with B, max_pages >= 1 and max_pages page_size < 2^31, got "
                        f"{tuple(block_table.shape)}", _lib.NNOP_ERR_SHAPE)
    ts = block_table.stride(0) if B > 1 else max_pages
    if (max_pages > 1 and block_table.stride(1) != 1) or ts < max_pages:
        raise NNopError(f"{FN}: block_table must have a last stride of 1 and a row stride of at least max_pages, got "
                        f"{block_table.stride()}", _lib.NNOP_ERR_SHAPE)
    if KH < 1 or QH < 1 or QH % KH or QH // KH > MAX_GROUP:
        raise NNopError(f"{FN}: QH must be a multiple of KH and QH / KH at most {MAX_GROUP}; got QH {QH}, KH {KH}", _lib.NNOP_ERR_SHAPE)
    if isinstance(window_left, bool) or not isinstance(window_left, (int, type(None))):
        raise TypeError(f"{FN}: window_left must be None or an int, got {window_left!r}")
    if window_left is not None and window_left < 0:
        raise ValueError(f"{FN}: window_left must be >= 0, got {window_left}")
    w = -1 if window_left is None else min(window_left, max_pages * page)       # a window beyond the table removes no key
    ks, vs = _strides("k_pages", k_pages, (E, E, E)), _strides("v_pages", v_pages, (E, E, E))
    qs = _strides("q", q, (QH * E, E))
    if o is not None:
        _tensor("o", o, 3)
        if o.dtype != q.dtype or o.shape != q.shape or o.device != q.device:
            raise NNopError(f"{FN}: o must have q's dtype, shape and device, got {_dtype_name(o.dtype)} {tuple(o.shape)}", _lib.NNOP_ERR_SHAPE)
    os_ = qs if o is None else _strides("o", o, (QH * E, E))
    return PagedPrefillDesc(dtype=_DTYPES[q.dtype], emb=E, tokens=T, qh=QH, kh=KH, batch=B, max_pages=max_pages, window_left=w, reserved=0,
                            flags=0, page_size=page, num_pages=P, k_stride_p=ks[0], k_stride_h=ks[1], k_stride_l=ks[2],
                            v_stride_p=vs[0], v_stride_h=vs[1], v_stride_l=vs[2], table_stride=ts,
                            q_stride_t=qs[0], q_stride_h=qs[1], o_stride_t=os_[0], o_stride_h=os_[1])


def _side(name, t, shape, dtype, like):
    _tensor(name, t, len(shape))
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise NNopError(f"{FN}: {name} must be a contiguous {_dtype_name(dtype)} tensor of shape {tuple(shape)} on q's device, got "
                        f"{_dtype_name(t.dtype)} {tuple(t.shape)}", _lib.NNOP_ERR_SHAPE)


def paged_prefill_attention_plan(q, k_pages, v_pages, block_table, *, window_left=None):
    """workspace bytes the call needs for these tensors: host-only, from shapes alone.  0 -- a workgroup finds its block by a search over
    cu_seqlens_q and keeps no list -- after every check of the call itself."""
    d = _desc(q, k_pages, v_pages, block_table, window_left)
    if d.tokens == 0:                                                           # nothing to launch: the library is not asked
        return 0
    nbytes = C.c_size_t(1)
    _raise(_lib_paged_prefill.load().nnop_paged_prefill_plan(C.byref(d), C.byref(nbytes)))
    return nbytes.value


def _run(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, window_left, sinks, workspace, want_lse=False):
    """every check, then o and lse where the caller brought none (o is None), then the call; with no token at all (every sequence at
    n_b = 0) nothing is launched"""
    d = _desc(q, k_pages, v_pages, block_table, window_left, o)
    (T, QH, E), B = q.shape, block_table.size(0)
    if lse is not None:
        _side("lse", lse, (T, QH), torch.float32, q)
    _side("cu_seqlens_q", cu_seqlens_q, (B + 1,), torch.int32, q)
    _side("seqlens", seqlens, (B,), torch.int32, q)
    if sinks is not None:
        _side("sinks", sinks, (QH,), torch.float32, q)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.device != q.device or not workspace.is_contiguous()):
        raise NNopError(f"{FN}: workspace must be a contiguous tensor on q's device", _lib.NNOP_ERR_WORKSPACE)
    have = 0 if workspace is None else workspace.numel() * workspace.element_size()
    with _on_device(q):
        if o is None:
            o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
            lse = torch.empty((T, QH), dtype=torch.float32, device=q.device) if want_lse else None
        if T:
            _raise(_lib_paged_prefill.load().nnop_paged_prefill(C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(k_pages), _ptr(v_pages),
                                                               _ptr(block_table), _ptr(cu_seqlens_q), _ptr(seqlens), _ptr(sinks),
                                                               _ptr(workspace) if have else None, have, _stream(q)))
    return o if lse is None else (o, lse)


def paged_prefill_attention_into(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, window_left=None, sinks=None,
                                 workspace=None):
    """Writes o (q's shape and dtype, strides of its own) and, unless it is None, lse [T, QH] float32.  Nothing is allocated: the form
    for captured graphs."""
    _tensor("o", o, 3)
    return _run(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, window_left, sinks, workspace)


def paged_prefill_attention(q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, window_left=None, sinks=None, return_lse=False,
                            workspace=None):
    """o [T, QH, E], or (o, lse [T, QH] float32): every sequence's new tokens against its pages, aligned to the sequence's end."""
    return _run(None, None, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, window_left, sinks, workspace, want_lse=return_lse)
