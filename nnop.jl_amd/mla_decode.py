"""The decode step of multi-head latent attention (MLA: DeepSeek-V2 / V3 / R1, Kimi-K2) in its weight-absorbed form over a paged latent
cache, over the C ABI of the eighteenth library (include/nnop_hip_mla_decode.h; no counterpart in the reference).  There is one "KV
head": a 576-wide row per key -- 512 compressed latent values, then 64 rotary values -- that is the key (all 576 columns) and the value
(the first 512) of every query head.  The pages are read where they lie; nothing is gathered or expanded per step.

    o = mla_decode_attention(q, kv_pages, block_table, seqlens, *, softmax_scale=None, num_splits=None, return_lse=False,
                             workspace=None)                                               # o, or (o, lse)
    mla_decode_attention_into(o, lse, q, kv_pages, block_table, seqlens, ...)              # caller-owned buffers: for captured graphs
    splits, workspace_bytes = mla_decode_attention_plan(q, kv_pages, block_table, num_splits=None)

q [B, QH, QL, 576], float16 or bfloat16: a head's absorbed query (q_nope W_UK, 512 wide) followed by its rotary part (64 wide); last
stride 1, the B, QH and QL strides free as multiples of 8 elements, so a [B, QL, QH, 576] projection is passed as `.transpose(1, 2)` and
never copied.  QH a multiple of 16 in 16 ... 128; QL 1 ... 8.  kv_pages [P, page_size, 576] of q's dtype, the layout FlashMLA and vLLM
keep ([P, page_size, 1, 576] is taken as a view); page and row strides multiples of 8 elements, at least a row; page_size a power of
two, 16 or more.  block_table [B, max_pages] int32 and seqlens [B] int32 on the device, INCLUDING the QL new tokens, exactly as in
paged_decode_attention.  Row (b, h, i) stands at p = seqlens[b] - QL + i and sees keys 0 ... p; the score is softmax_scale <q, c_j> in
fp32 and o [B, QH, QL, 512] = sum_j softmax_j c_j[:512], rounded once; lse [B, QH, QL] float32; a row without a key has o = 0 and
lse = -inf.  softmax_scale is a finite positive host float; None means 192 ** -0.5 -- DeepSeek's 128 + 64 wide heads, not 1 / sqrt(576);
callers with YaRN pass their own.  No window, no sinks.

Contracts (the header states them in full): paged_decode_attention's.  The grid comes from host values alone -- no sync, no allocation,
no atomics, and a captured graph follows seqlens, the table and the pages.  Two runs are bitwise equal.  Masking is by selection: a
pool row no query of its sequence sees may hold NaN.  Only table entries of pages with a visible key are read, and every id is clamped
into [0, P - 1] before it forms an address.  At a fixed split count a sequence's bits depend neither on the batch, nor on P, nor on
where its pages lie.  The workspace may hold anything.

No autograd, GPU-only, no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib, _lib_mla_decode
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_mla_decode import LATENT, MAX_HEADS, MAX_QL, MAX_SPLITS, MIN_PAGE_SIZE, WIDTH, MlaDecodeDesc
from .paged_prefill import _side, _strides, _tensor

__all__ = ["mla_decode_attention", "mla_decode_attention_into", "mla_decode_attention_plan"]

FN = "mla_decode_attention"
DEFAULT_SCALE = 192 ** -0.5


def _desc(q, kv_pages, block_table, softmax_scale, num_splits):
    """every host check of q, the pool, the table and the options -> the descriptor"""
    _tensor("q", q, 4), _tensor("block_table", block_table, 2)
    if isinstance(kv_pages, torch.Tensor) and kv_pages.dim() == 4 and kv_pages.size(2) == 1:
        kv_pages = kv_pages[:, :, 0]                                              # [P, page_size, 1, 576]: a view
    _tensor("kv_pages", kv_pages, 3)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: q must be float16 or bfloat16, got {_dtype_name(q.dtype)}", _lib.NNOP_ERR_DTYPE)
    if kv_pages.dtype != q.dtype or kv_pages.device != q.device:
        raise NNopError(f"{FN}: kv_pages must have q's dtype and device", _lib.NNOP_ERR_DTYPE)
    if block_table.dtype != torch.int32 or block_table.device != q.device:
        raise NNopError(f"{FN}: block_table must be int32 on q's device, got {_dtype_name(block_table.dtype)}", _lib.NNOP_ERR_DTYPE)
    if any(t.requires_grad for t in (q, kv_pages)) and torch.is_grad_enabled():
        raise NNopError(f"{FN} has no backward")
    scale = DEFAULT_SCALE if softmax_scale is None else softmax_scale
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"{FN}: softmax_scale must be None or a float, got {softmax_scale!r}")
    if not (math.isfinite(scale) and 0 < scale <= 3.4e38):
        raise NNopError(f"{FN}: softmax_scale must be finite and positive, got {scale}", _lib.NNOP_ERR_OPTS)
    if isinstance(num_splits, bool) or not isinstance(num_splits, (int, type(None))):
        raise TypeError(f"{FN}: num_splits must be None or an int, got {num_splits!r}")
    if num_splits is not None and not 1 <= num_splits <= MAX_SPLITS:
        raise ValueError(f"{FN}: num_splits must be 1 ... {MAX_SPLITS}, got {num_splits}")
    B, QH, QL, W = q.shape
    if W != WIDTH or kv_pages.size(2) != WIDTH or kv_pages.size(0) < 1:
        raise NNopError(f"{FN}: the last dimension of q and kv_pages must be {WIDTH} (512 latent + 64 rotary values), got {tuple(q.shape)} "
                        f"and {tuple(kv_pages.shape)}", _lib.NNOP_ERR_SHAPE)
    if B < 1 or QH < 16 or QH > MAX_HEADS or QH % 16 or not 1 <= QL <= MAX_QL:
        raise NNopError(f"{FN}: QH must be a multiple of 16 in 16 ... {MAX_HEADS} and QL 1 ... {MAX_QL}; got B {B}, QH {QH}, QL {QL}",
                        _lib.NNOP_ERR_SHAPE)
    P, page = kv_pages.shape[:2]
    if page < MIN_PAGE_SIZE or page & (page - 1):
        raise NNopError(f"{FN}: page_size must be a power of two, {MIN_PAGE_SIZE} or more, got {page}", _lib.NNOP_ERR_SHAPE)
    max_pages = block_table.size(1)
    if block_table.size(0) != B or max_pages < 1 or max_pages * page > 2 ** 31 - 1 or max_pages * page < QL:
        raise NNopError(f"{FN}: block_table must be [B, max_pages] = [{B}, max_pages] with QL <= max_pages page_size < 2^31, got "
                        f"{tuple(block_table.shape)}", _lib.NNOP_ERR_SHAPE)
    ts = block_table.stride(0) if B > 1 else max_pages
    if (max_pages > 1 and block_table.stride(1) != 1) or ts < max_pages:
        raise NNopError(f"{FN}: block_table must have a last stride of 1 and a row stride of at least max_pages, got "
                        f"{block_table.stride()}", _lib.NNOP_ERR_SHAPE)
    qs, cs = _strides("q", q, (WIDTH,) * 3), _strides("kv_pages", kv_pages, (WIDTH,) * 2)
    return kv_pages, MlaDecodeDesc(dtype=_DTYPES[q.dtype], ql=QL, qh=QH, batch=B, max_pages=max_pages, page_size=page, num_pages=P,
                                   splits=num_splits or 0, flags=0, reserved0=0, reserved1=0, softmax_scale=scale,
                                   q_stride_b=qs[0], q_stride_h=qs[1], q_stride_l=qs[2], kv_stride_p=cs[0], kv_stride_l=cs[1],
                                   table_stride=ts)


def _plan(d):
    splits, nbytes = C.c_int32(0), C.c_size_t(0)
    _raise(_lib_mla_decode.load().nnop_mla_decode_plan(C.byref(d), C.byref(splits), C.byref(nbytes)))
    return splits.value, nbytes.value


def mla_decode_attention_plan(q, kv_pages, block_table, *, softmax_scale=None, num_splits=None):
    """(splits, workspace_bytes) the call will use for these tensors: host-only, from shapes alone.  The automatic count is
    min(max(min(ceil(512 / (B QL ceil(QH / 64))), ceil(max_pages page_size / 32) / 4), 1), 64); the workspace is 0 bytes at one split,
    else 4 B QH QL splits (512 + 2)."""
    return _plan(_desc(q, kv_pages, block_table, softmax_scale, num_splits)[1])


def _run(checked, o, lse, q, block_table, seqlens, workspace):
    """the checks of everything but q, the pool and the table (those made `checked`), the workspace where the caller brought none, the call"""
    kv_pages, d = checked
    B, QH, QL, _ = q.shape
    _side("o", o, (B, QH, QL, LATENT), q.dtype, q)
    if lse is not None:
        _side("lse", lse, (B, QH, QL), torch.float32, q)
    _side("seqlens", seqlens, (B,), torch.int32, q)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.device != q.device or not workspace.is_contiguous()):
        raise NNopError(f"{FN}: workspace must be a contiguous tensor on q's device", _lib.NNOP_ERR_WORKSPACE)
    need = _plan(d)[1]
    with _on_device(q):
        if workspace is None and need:
            workspace = torch.empty(need // 4, dtype=torch.float32, device=q.device)
        have = 0 if workspace is None else workspace.numel() * workspace.element_size()
        _raise(_lib_mla_decode.load().nnop_mla_decode(C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(kv_pages), _ptr(block_table),
                                                      _ptr(seqlens), _ptr(workspace) if have else None, have, _stream(q)))
    return o if lse is None else (o, lse)


def mla_decode_attention_into(o, lse, q, kv_pages, block_table, seqlens, *, softmax_scale=None, num_splits=None, workspace=None):
    """Writes o [B, QH, QL, 512] of q's dtype and, unless it is None, lse [B, QH, QL] float32.  With a `workspace` of
    mla_decode_attention_plan's size nothing is allocated: the form for captured graphs."""
    return _run(_desc(q, kv_pages, block_table, softmax_scale, num_splits), o, lse, q, block_table, seqlens, workspace)


def mla_decode_attention(q, kv_pages, block_table, seqlens, *, softmax_scale=None, num_splits=None, return_lse=False, workspace=None):
    """o [B, QH, QL, 512], or (o, lse [B, QH, QL] float32): the QL new tokens of every sequence against its latent pages."""
    checked = _desc(q, kv_pages, block_table, softmax_scale, num_splits)          # in front of any allocation
    with _on_device(q):
        o = q.new_empty((*q.shape[:3], LATENT))
        lse = q.new_empty(q.shape[:3], dtype=torch.float32) if return_lse else None
    return _run(checked, o, lse, q, block_table, seqlens, workspace)
