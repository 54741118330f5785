"""Attention of a PREFILL step over a paged KV cache kept in 8-bit floating point, over the C ABI of the fifteenth library
(include/nnop_hip_paged_prefill_fp8.h; no counterpart in the reference): paged_prefill_attention on paged_decode_attention_fp8's pools --
pages of one-byte OCP E4M3 codes with one float32 scale per KV head.  A caller who keeps the cache as E4M3 pages runs its prefill steps
here and its decode steps through paged_decode_attention_fp8 over the same pages; nothing is gathered, and no 16-bit copy of the pool is
kept.  The codes are expanded to q's type in the registers that stage a tile for LDS; everything behind that is
paged_prefill_attention's kernel.

    o = paged_prefill_attention_fp8(q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, k_scale=None, v_scale=None,
                                    window_left=None, sinks=None, return_lse=False, workspace=None)          # o, or (o, lse)
    paged_prefill_attention_fp8_into(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, ...)   # caller-owned buffers: for captured graphs
    workspace_bytes = paged_prefill_attention_fp8_plan(q, k_pages, v_pages, block_table)                     # 0

q, o, lse, cu_seqlens_q, seqlens, block_table, window_left and sinks are paged_prefill_attention's: q, o [T, QH, E] float16 or bfloat16, E
64 or 128, QH / KH <= 16, last stride 1, token and head strides multiples of 8 elements; query i of sequence b stands at
p = seqlens[b] - n_b + i and sees keys max(0, p - window_left) ... p; a row that sees no key has o = 0 and lse = its sink, or -inf.
k_pages, v_pages, k_scale and v_scale are paged_decode_attention_fp8's: [P, KH, page_size, E] of torch.float8_e4m3fn, or of uint8 taken
as the same codes, with any strides whose last is 1 and whose others are multiples of 16 bytes and at least a row -- a
[P, page_size, KH, E] pool is passed as `pool.transpose(1, 2)`, never copied; page_size a power of two, 16 or more; the scales [KH]
float32 on the device or None (= 1), read when the kernel runs.

x = (q . code(k)) (k_scale / sqrt(E)), one factor applied to the float32 scores, so sinks and lse are in that domain;
o = v_scale sum softmax(x) code(v), scaled in float32 after the division and in front of its one rounding.  A NaN code in a row some
query of the sequence sees gives NaN; in a row none sees it changes nothing.

Contracts (the header states them in full): paged_prefill_attention's -- a grid from host values alone, no sync, no allocation, no
atomics, two runs bitwise equal, only live table entries read, every id clamped into [0, P - 1] before it forms an address, rows outside
a sequence's visible range never loaded, a sequence's bits independent of P, of where its pages lie, of page_size and of the other
sequences -- and a captured graph follows cu_seqlens_q, seqlens, the table, the pages and the scales.  The conversion of a code is exact,
so without scales o and lse equal, bit for bit, paged_prefill_attention on a pool that holds the same values in q's type.

Writing the new rows into the pages is the caller's: `(x / scale).to(torch.float8_e4m3fn)` and an index write.  No autograd, GPU-only,
no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_paged_prefill_fp8
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_paged_prefill_fp8 import EMBS, KV_E4M3, MAX_GROUP, MIN_PAGE_SIZE, PagedPrefillFp8Desc

__all__ = ["paged_prefill_attention_fp8", "paged_prefill_attention_fp8_into", "paged_prefill_attention_fp8_plan"]

FN = "paged_prefill_attention_fp8"
PAGE_DTYPES = (torch.float8_e4m3fn, torch.uint8)


def _tensor(name, t, dims):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{FN}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise NNopError(f"{FN} is GPU-only: {name} is on {t.device}")
    if t.dim() != dims:
        raise NNopError(f"{FN}: {name} must have {dims} dimensions, got {t.dim()}", _lib.NNOP_ERR_SHAPE)


def _strides(name, t, floors, unit, what):
    """strides of every dimension but the last, multiples of `unit`; a dimension of one row has none of its own and gets its floor"""
    if t.stride(-1) != 1:
        raise NNopError(f"{FN}: {name} must be contiguous in its last dimension", _lib.NNOP_ERR_SHAPE)
    strides = tuple(t.stride(i) if t.size(i) > 1 else f for i, f in enumerate(floors))
    if any(s < f or s % unit for s, f in zip(strides, floors)):
        raise NNopError(f"{FN}: the strides of {name} must be multiples of {unit} {what} and at least {floors}, got {t.stride()}",
                        _lib.NNOP_ERR_SHAPE)
    return strides


def _desc(q, k_pages, v_pages, block_table, window_left, o=None):
    """every host check of q, o, the pools and the table -> the descriptor"""
    _tensor("q", q, 3), _tensor("k_pages", k_pages, 4), _tensor("v_pages", v_pages, 4), _tensor("block_table", block_table, 2)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: q must be float16 or bfloat16, got {_dtype_name(q.dtype)}", _lib.NNOP_ERR_DTYPE)
    for name, t in (("k_pages", k_pages), ("v_pages", v_pages)):
        if t.dtype not in PAGE_DTYPES or t.device != q.device:
            raise NNopError(f"{FN}: {name} must be float8_e4m3fn (or uint8 holding those codes) on q's device, got "
                            f"{_dtype_name(t.dtype)}; paged_prefill_attention takes 16-bit pages", _lib.NNOP_ERR_DTYPE)
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
    ks, vs = (_strides(name, t, (E, E, E), 16, "bytes") for name, t in (("k_pages", k_pages), ("v_pages", v_pages)))
    qs = _strides("q", q, (QH * E, E), 8, "elements")
    if o is not None:
        _tensor("o", o, 3)
        if o.dtype != q.dtype or o.shape != q.shape or o.device != q.device:
            raise NNopError(f"{FN}: o must have q's dtype, shape and device, got {_dtype_name(o.dtype)} {tuple(o.shape)}", _lib.NNOP_ERR_SHAPE)
    os_ = qs if o is None else _strides("o", o, (QH * E, E), 8, "elements")
    return PagedPrefillFp8Desc(dtype=_DTYPES[q.dtype], emb=E, tokens=T, qh=QH, kh=KH, batch=B, max_pages=max_pages, window_left=w,
                               reserved=0, flags=0, page_size=page, num_pages=P, kv_format=KV_E4M3, reserved2=0,
                               k_stride_p=ks[0], k_stride_h=ks[1], k_stride_l=ks[2], v_stride_p=vs[0], v_stride_h=vs[1], v_stride_l=vs[2],
                               table_stride=ts, q_stride_t=qs[0], q_stride_h=qs[1], o_stride_t=os_[0], o_stride_h=os_[1])


def _side(name, t, shape, dtype, like):
    _tensor(name, t, len(shape))
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise NNopError(f"{FN}: {name} must be a contiguous {_dtype_name(dtype)} tensor of shape {tuple(shape)} on q's device, got "
                        f"{_dtype_name(t.dtype)} {tuple(t.shape)}", _lib.NNOP_ERR_SHAPE)


def paged_prefill_attention_fp8_plan(q, k_pages, v_pages, block_table, *, window_left=None):
    """workspace bytes the call needs for these tensors: host-only, from shapes alone.  0, as for paged_prefill_attention, after every
    check of the call itself."""
    d = _desc(q, k_pages, v_pages, block_table, window_left)
    if d.tokens == 0:                                                           # nothing to launch: the library is not asked
        return 0
    nbytes = C.c_size_t(1)
    _raise(_lib_paged_prefill_fp8.load().nnop_paged_prefill_fp8_plan(C.byref(d), C.byref(nbytes)))
    return nbytes.value


def _run(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, k_scale, v_scale, window_left, sinks, workspace, want_lse=False):
    """every check, then o and lse where the caller brought none (o is None), then the call; with no token at all (every sequence at
    n_b = 0) nothing is launched"""
    d = _desc(q, k_pages, v_pages, block_table, window_left, o)
    (T, QH, E), B = q.shape, block_table.size(0)
    if lse is not None:
        _side("lse", lse, (T, QH), torch.float32, q)
    _side("cu_seqlens_q", cu_seqlens_q, (B + 1,), torch.int32, q)
    _side("seqlens", seqlens, (B,), torch.int32, q)
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is not None:
            _side(name, t, (d.kh,), torch.float32, q)
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
            _raise(_lib_paged_prefill_fp8.load().nnop_paged_prefill_fp8(
                C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(k_pages), _ptr(v_pages), _ptr(k_scale), _ptr(v_scale), _ptr(block_table),
                _ptr(cu_seqlens_q), _ptr(seqlens), _ptr(sinks), _ptr(workspace) if have else None, have, _stream(q)))
    return o if lse is None else (o, lse)


def paged_prefill_attention_fp8_into(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, k_scale=None, v_scale=None,
                                     window_left=None, sinks=None, workspace=None):
    """Writes o (q's shape and dtype, strides of its own) and, unless it is None, lse [T, QH] float32.  Nothing is allocated: the form
    for captured graphs."""
    _tensor("o", o, 3)
    return _run(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, k_scale, v_scale, window_left, sinks, workspace)


def paged_prefill_attention_fp8(q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, k_scale=None, v_scale=None, window_left=None,
                                sinks=None, return_lse=False, workspace=None):
    """o [T, QH, E], or (o, lse [T, QH] float32): every sequence's new tokens against its pages of E4M3 codes, aligned to the sequence's
    end."""
    return _run(None, None, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, k_scale, v_scale, window_left, sinks, workspace,
                want_lse=return_lse)
