"""The WRITE side of the paged KV cache, over the C ABI of the seventeenth library (include/nnop_hip_paged_kv_write.h; no counterpart in the
reference): the K and V rows of a step's new tokens go into the pages that paged_decode_attention, paged_prefill_attention and their
_fp8 and _split forms read, K and V in one launch.

    paged_kv_cache_write(k, v, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, k_scale=None, v_scale=None)   # in place, None

k, v [T, KH, E], float16 or bfloat16, E 64 or 128: the new tokens of all sequences packed token-major, exactly as paged_prefill_attention
takes q; last stride 1, token and head strides multiples of 8 elements, each tensor with its own -- the K and V slices of a fused QKV
projection are read where they lie.  k_pages, v_pages: the pools of the reading calls, [P, KH, page_size, E] with any strides they accept
(a [P, page_size, KH, E] pool is passed as `pool.transpose(1, 2)`), page_size a power of two, 16 or more.  A pool of k's dtype gets the
rows bit for bit; a pool of torch.float8_e4m3fn (or uint8) gets their E4M3 codes.  Both pools have the same format.  block_table
[B, max_pages], cu_seqlens_q [B + 1] and seqlens [B] are paged_prefill_attention's, int32 on the device and read there: seqlens[b] counts
the keys of sequence b INCLUDING its n_b = cu[b + 1] - cu[b] new ones.  k_scale, v_scale: [KH] float32 on the device or None (= 1), for
E4M3 pools only.

Token i of sequence b stands at p = seqlens[b] - n_b + i, where paged_prefill_attention places its query, and its rows go to row
p mod page_size of page block_table[b][p // page_size].  A token with p < 0, or whose table entry lies outside [0, P) (-1: a page of
another rank), writes nothing: an id is never clamped here, a clamped write would destroy another sequence's page.  Nothing else in the
pools is touched.

The quantisation rule, the one the project has:  code = RNE_to_E4M3(clamp(fp32(x) / scale[h], -448, +448)), which is
`(x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn)` bit for bit -- a correctly rounded division, ties to the even code, +-inf and
everything beyond +-448 to +-448, NaN to a NaN code.

Contracts (the header states them in full): the grid comes from T alone and everything else is read on the device -- no sync, no
allocation, no workspace, no atomics, so the call is itself the form for captured graphs, and a captured graph follows cu_seqlens_q,
seqlens, the table, the source rows and the scales at fixed T and B.  Two runs are bitwise equal; what a sequence's tokens write depends
neither on P, nor on where its pages lie, nor on the other sequences.  With T == 0 nothing is launched.

No autograd, GPU-only, no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_paged_kv_write
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_paged_kv_write import EMBS, KV_16BIT, KV_E4M3, MIN_PAGE_SIZE, PagedKvWriteDesc
from .paged_prefill import _side, _tensor

__all__ = ["paged_kv_cache_write"]

FN = "paged_kv_cache_write"
CODE_DTYPES = (torch.float8_e4m3fn, torch.uint8)


def _strides(name, t, floors, unit):
    """strides of every dimension but the last, multiples of `unit` elements; a dimension of one row has none of its own and gets its
    floor"""
    if t.stride(-1) != 1:
        raise NNopError(f"{FN}: {name} must be contiguous in its last dimension", _lib.NNOP_ERR_SHAPE)
    strides = tuple(t.stride(i) if t.size(i) > 1 else f for i, f in enumerate(floors))
    if any(s < f or s % unit for s, f in zip(strides, floors)):
        raise NNopError(f"{FN}: the strides of {name} must be multiples of {unit} elements and at least {floors}, got {t.stride()}",
                        _lib.NNOP_ERR_SHAPE)
    return strides


def _desc(k, v, k_pages, v_pages, block_table, scales=False):
    """every host check of the sources, the pools and the table -> the descriptor"""
    _tensor("k", k, 3), _tensor("v", v, 3), _tensor("k_pages", k_pages, 4), _tensor("v_pages", v_pages, 4), _tensor("block_table", block_table, 2)
    if k.dtype not in (torch.float16, torch.bfloat16):
        raise NNopError(f"{FN}: k must be float16 or bfloat16, got {_dtype_name(k.dtype)}", _lib.NNOP_ERR_DTYPE)
    if v.dtype != k.dtype or v.device != k.device:
        raise NNopError(f"{FN}: v must have k's dtype and device, got {_dtype_name(v.dtype)}", _lib.NNOP_ERR_DTYPE)
    fmt = KV_E4M3 if k_pages.dtype in CODE_DTYPES else KV_16BIT
    for name, t in (("k_pages", k_pages), ("v_pages", v_pages)):
        if (t.dtype not in CODE_DTYPES if fmt == KV_E4M3 else t.dtype != k.dtype) or t.device != k.device:
            raise NNopError(f"{FN}: k_pages and v_pages must both have k's dtype, or both be float8_e4m3fn (or uint8 holding those codes), "
                            f"on k's device; {name} is {_dtype_name(t.dtype)}", _lib.NNOP_ERR_DTYPE)
    if block_table.dtype != torch.int32 or block_table.device != k.device:
        raise NNopError(f"{FN}: block_table must be int32 on k's device, got {_dtype_name(block_table.dtype)}", _lib.NNOP_ERR_DTYPE)
    if scales and fmt == KV_16BIT:
        raise NNopError(f"{FN}: k_scale and v_scale are for E4M3 pools; a 16-bit pool gets the rows as they are", _lib.NNOP_ERR_OPTS)
    T, KH, E = k.shape
    if E not in EMBS or KH < 1 or v.shape != k.shape:
        raise NNopError(f"{FN}: k and v must both be [T, KH, E] with E 64 or 128, got {tuple(k.shape)} and {tuple(v.shape)}", _lib.NNOP_ERR_SHAPE)
    if k_pages.shape != v_pages.shape or k_pages.size(0) < 1 or tuple(k_pages.shape[1::2]) != (KH, E):
        raise NNopError(f"{FN}: k_pages and v_pages must both be [P, KH, page_size, E] = [P, {KH}, page_size, {E}], got "
                        f"{tuple(k_pages.shape)} and {tuple(v_pages.shape)}", _lib.NNOP_ERR_SHAPE)
    P, page = k_pages.size(0), k_pages.size(2)
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
    unit = 16 if fmt == KV_E4M3 else 8                                          # 16 bytes of the pool
    kps, vps = (_strides(name, t, (E, E, E), unit) for name, t in (("k_pages", k_pages), ("v_pages", v_pages)))
    ks, vs = (_strides(name, t, (KH * E, E), 8) for name, t in (("k", k), ("v", v)))
    return PagedKvWriteDesc(dtype=_DTYPES[k.dtype], emb=E, tokens=T, kh=KH, batch=B, max_pages=max_pages, page_size=page, num_pages=P,
                            kv_format=fmt, reserved=0, flags=0, reserved2=0, kp_stride_p=kps[0], kp_stride_h=kps[1], kp_stride_l=kps[2],
                            vp_stride_p=vps[0], vp_stride_h=vps[1], vp_stride_l=vps[2], table_stride=ts,
                            k_stride_t=ks[0], k_stride_h=ks[1], v_stride_t=vs[0], v_stride_h=vs[1])


def paged_kv_cache_write(k, v, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, k_scale=None, v_scale=None):
    """Writes the K and V rows of every sequence's new tokens into its pages, in place; returns None.  Nothing is allocated: the form
    for captured graphs.  With no token at all nothing is launched."""
    d = _desc(k, v, k_pages, v_pages, block_table, scales=k_scale is not None or v_scale is not None)
    _side("cu_seqlens_q", cu_seqlens_q, (d.batch + 1,), torch.int32, k)
    _side("seqlens", seqlens, (d.batch,), torch.int32, k)
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is not None:
            _side(name, t, (d.kh,), torch.float32, k)
    if d.tokens:
        with _on_device(k):
            _raise(_lib_paged_kv_write.load().nnop_paged_kv_write(
                C.byref(d), _ptr(k_pages), _ptr(v_pages), _ptr(k), _ptr(v), _ptr(k_scale), _ptr(v_scale), _ptr(block_table),
                _ptr(cu_seqlens_q), _ptr(seqlens), _stream(k)))
