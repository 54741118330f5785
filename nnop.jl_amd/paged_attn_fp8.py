"""Attention of a decode step over a PAGED KV cache kept in 8-bit floating point, over the C ABI of the fourteenth library
(include/nnop_hip_paged_attn_fp8.h; no counterpart in the reference): decode_attention_fp8 with the cache kept as serving engines keep
it -- a pool of pages of page_size keys and an int32 block table per sequence -- or, read the other way, paged_decode_attention on
pages of one-byte OCP E4M3 codes with one float32 scale per KV head.  The pages are read where they lie and the codes are expanded in
registers: no dense copy of a sequence's keys is gathered and no 16-bit copy of the pool is kept.

    o = paged_decode_attention_fp8(q, k_pages, v_pages, block_table, seqlens, *, k_scale=None, v_scale=None, window_left=None,
                                   sinks=None, num_splits=None, return_lse=False, workspace=None)      # o, or (o, lse)
    paged_decode_attention_fp8_into(o, lse, q, k_pages, v_pages, block_table, seqlens, ...)   # caller-owned buffers: for captured graphs
    splits, workspace_bytes = paged_decode_attention_fp8_plan(q, k_pages, v_pages, block_table, window_left=None, num_splits=None)

q [B, QH, QL, E] contiguous, float16 or bfloat16, E 64 or 128, (QH / KH) QL <= 16; k_pages, v_pages [P, KH, page_size, E] of
torch.float8_e4m3fn, or of uint8 taken as the same codes, with any strides whose last is 1 and whose others are multiples of 16 bytes
and at least a row -- a [P, page_size, KH, E] pool (the vLLM layout) is passed as `pool.transpose(1, 2)`, never copied; K and V may
differ in their strides.  page_size is a power of two, 16 or more.  block_table [B, max_pages] int32 on the device, last stride 1, row
stride >= max_pages: entry (b, n) is the page that holds keys n page_size ... of sequence b, for K and for V.  seqlens [B] int32 on the
device, INCLUDING the QL new tokens, clamped into [0, max_pages page_size].  k_scale, v_scale [KH] float32 on the device or None (= 1).

The semantics are decode_attention_fp8's: x = (q . code(k)) (k_scale / sqrt(E)), one factor applied to the float32 scores, so sinks and
lse are in that domain; o = v_scale sum softmax(x) code(v), scaled in float32 after the division and in front of its one rounding;
sinks, lse, the bottom-right alignment, window_left and the dead rows (o = 0, lse = the sink or -inf) as in that call.

Contracts (the header states them in full): decode_attention_fp8's, and four more.
1. At the same resolved split count o and lse equal, bit for bit, decode_attention_fp8 on the same codes gathered into a dense cache.
2. Only table entries of pages that hold a visible key are read, so the others may hold anything; every id read is clamped into
   [0, P - 1] before it forms an address: a wrong table gives wrong numbers, never an access outside the pool.
3. A sequence's bits do not depend on P, on where its pages lie, or on the other sequences.
4. A captured call follows seqlens, the table, the pages and the scales.

Writing the new rows into the pages is the caller's: `(x / scale).to(torch.float8_e4m3fn)` and an index write.  No autograd, GPU-only,
no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_paged_attn_fp8
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_paged_attn_fp8 import EMBS, KV_E4M3, MAX_ROWS, MAX_SPLITS, MIN_PAGE_SIZE, PagedAttnFp8Desc

__all__ = ["paged_decode_attention_fp8", "paged_decode_attention_fp8_into", "paged_decode_attention_fp8_plan"]

FN = "paged_decode_attention_fp8"
PAGE_DTYPES = (torch.float8_e4m3fn, torch.uint8)


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


def _pool_strides(name, t, E):
    """byte strides (page, kvh, row) of a pool of one-byte elements; a dimension of one row has no stride of its own"""
    if t.stride(3) != 1:
        raise NNopError(f"{FN}: {name} must be contiguous in its last dimension", _lib.NNOP_ERR_SHAPE)
    strides = tuple(t.stride(i) if t.size(i) > 1 else E for i in range(3))
    if any(s < E or s % 16 for s in strides) or (t.size(2) - 1) * strides[2] + E > 2 ** 32 - 1:
        raise NNopError(f"{FN}: the strides of {name} must be multiples of 16 bytes and at least a row, and the rows of a page must lie "
                        f"within 2^32 bytes, got {t.stride()}", _lib.NNOP_ERR_SHAPE)
    return strides


def _desc(q, k_pages, v_pages, block_table, window_left, num_splits):
    """every host check of q, the pools and the table -> the descriptor"""
    _tensor("q", q, 4), _tensor("k_pages", k_pages, 4), _tensor("v_pages", v_pages, 4), _tensor("block_table", block_table, 2)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: q must be float16 or bfloat16, got {_dtype_name(q.dtype)}", _lib.NNOP_ERR_DTYPE)
    for name, t in (("k_pages", k_pages), ("v_pages", v_pages)):
        if t.dtype not in PAGE_DTYPES or t.device != q.device:
            raise NNopError(f"{FN}: {name} must be float8_e4m3fn (or uint8 holding those codes) on q's device, got "
                            f"{_dtype_name(t.dtype)}; paged_decode_attention takes 16-bit pages", _lib.NNOP_ERR_DTYPE)
    if block_table.dtype != torch.int32 or block_table.device != q.device:
        raise NNopError(f"{FN}: block_table must be int32 on q's device, got {_dtype_name(block_table.dtype)}", _lib.NNOP_ERR_DTYPE)
    if any(t.requires_grad for t in (q, k_pages, v_pages)) and torch.is_grad_enabled():
        raise NNopError(f"{FN} has no backward: use flash_attention for a tensor that requires a gradient")
    B, QH, QL, E = q.shape
    if not q.is_contiguous():
        raise NNopError(f"{FN}: q must be contiguous", _lib.NNOP_ERR_SHAPE)
    if E not in EMBS:
        raise NNopError(f"{FN}: the head dimension must be 64 or 128, got {E}", _lib.NNOP_ERR_SHAPE)
    if k_pages.shape != v_pages.shape or k_pages.size(3) != E or k_pages.size(0) < 1:
        raise NNopError(f"{FN}: k_pages and v_pages must both be [P, KH, page_size, E] = [P, KH, page_size, {E}], got "
                        f"{tuple(k_pages.shape)} and {tuple(v_pages.shape)}", _lib.NNOP_ERR_SHAPE)
    P, KH, page = k_pages.shape[:3]
    if page < MIN_PAGE_SIZE or page & (page - 1):
        raise NNopError(f"{FN}: page_size must be a power of two, {MIN_PAGE_SIZE} or more, got {page}", _lib.NNOP_ERR_SHAPE)
    max_pages = block_table.size(1)
    if block_table.size(0) != B or max_pages < 1 or max_pages * page > 2 ** 31 - 1:
        raise NNopError(f"{FN}: block_table must be [B, max_pages] = [{B}, max_pages] with max_pages page_size < 2^31, got "
                        f"{tuple(block_table.shape)}", _lib.NNOP_ERR_SHAPE)
    ts = block_table.stride(0) if B > 1 else max_pages
    if (max_pages > 1 and block_table.stride(1) != 1) or ts < max_pages:
        raise NNopError(f"{FN}: block_table must have a last stride of 1 and a row stride of at least max_pages, got "
                        f"{block_table.stride()}", _lib.NNOP_ERR_SHAPE)
    cap = max_pages * page
    if B < 1 or KH < 1 or QH % KH or QL < 1 or (QH // KH) * QL > MAX_ROWS or cap < QL:
        raise NNopError(f"{FN}: QH must be a multiple of KH, (QH / KH) QL must be at most {MAX_ROWS} and the table must hold the QL new "
                        f"tokens; got QH {QH}, KH {KH}, QL {QL}, max_pages page_size {cap}", _lib.NNOP_ERR_SHAPE)
    w = -1 if window_left is None else min(_int("window_left", window_left, 0), cap)       # a window beyond the table removes no key
    s = 0 if num_splits is None else _int("num_splits", num_splits, 1)
    if s > MAX_SPLITS:
        raise ValueError(f"{FN}: num_splits must be at most {MAX_SPLITS}, got {s}")
    ks, vs = _pool_strides("k_pages", k_pages, E), _pool_strides("v_pages", v_pages, E)
    return PagedAttnFp8Desc(dtype=_DTYPES[q.dtype], emb=E, ql=QL, qh=QH, kh=KH, batch=B, max_pages=max_pages, window_left=w, splits=s,
                            flags=0, page_size=page, num_pages=P, kv_format=KV_E4M3, reserved=0,
                            k_stride_p=ks[0], k_stride_h=ks[1], k_stride_l=ks[2],
                            v_stride_p=vs[0], v_stride_h=vs[1], v_stride_l=vs[2], table_stride=ts)


def _plan(d):
    splits, nbytes = C.c_int32(0), C.c_size_t(0)
    _raise(_lib_paged_attn_fp8.load().nnop_paged_attn_fp8_plan(C.byref(d), C.byref(splits), C.byref(nbytes)))
    return splits.value, nbytes.value


def _side(name, t, shape, dtype, like):
    _tensor(name, t, len(shape))
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise NNopError(f"{FN}: {name} must be a contiguous {_dtype_name(dtype)} tensor of shape {tuple(shape)} on q's device, got "
                        f"{_dtype_name(t.dtype)} {tuple(t.shape)}", _lib.NNOP_ERR_SHAPE)


def paged_decode_attention_fp8_plan(q, k_pages, v_pages, block_table, *, window_left=None, num_splits=None):
    """(splits, workspace_bytes) the call will use for these tensors: host-only, from shapes alone; decode_attention_fp8_plan's figures
    at a capacity of max_pages page_size."""
    return _plan(_desc(q, k_pages, v_pages, block_table, window_left, num_splits))


def _run(d, o, lse, q, k_pages, v_pages, k_scale, v_scale, block_table, seqlens, sinks, workspace):
    """the checks of everything but q, the pools and the table (those made `d`), the workspace, the call"""
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
        _raise(_lib_paged_attn_fp8.load().nnop_paged_attn_fp8(C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(k_pages), _ptr(v_pages),
                                                              _ptr(k_scale), _ptr(v_scale), _ptr(block_table), _ptr(seqlens), _ptr(sinks),
                                                              _ptr(workspace), have, _stream(q)))
    return o if lse is None else (o, lse)


def paged_decode_attention_fp8_into(o, lse, q, k_pages, v_pages, block_table, seqlens, *, k_scale=None, v_scale=None, window_left=None,
                                    sinks=None, num_splits=None, workspace=None):
    """Writes o (like q) and, unless it is None, lse [B, QH, QL] float32.  With a `workspace` of paged_decode_attention_fp8_plan's size
    nothing is allocated: the form for captured graphs."""
    return _run(_desc(q, k_pages, v_pages, block_table, window_left, num_splits), o, lse, q, k_pages, v_pages, k_scale, v_scale,
                block_table, seqlens, sinks, workspace)


def paged_decode_attention_fp8(q, k_pages, v_pages, block_table, seqlens, *, k_scale=None, v_scale=None, window_left=None, sinks=None,
                               num_splits=None, return_lse=False, workspace=None):
    """o [B, QH, QL, E], or (o, lse [B, QH, QL] float32): the QL new tokens of every sequence against its pages of E4M3 codes."""
    d = _desc(q, k_pages, v_pages, block_table, window_left, num_splits)
    with _on_device(q):
        o = torch.empty_like(q)
        lse = torch.empty(q.shape[:3], dtype=torch.float32, device=q.device) if return_lse else None
    return _run(d, o, lse, q, k_pages, v_pages, k_scale, v_scale, block_table, seqlens, sinks, workspace)
