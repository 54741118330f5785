"""Split-KV attention of a PREFILL step over a paged KV cache, over the C ABI of the sixteenth library
(include/nnop_hip_paged_prefill_split.h; no counterpart in the reference): paged_prefill_attention for FEW new tokens behind a LONG
context -- a chunk of a chunked prefill behind 32K-128K keys, a short follow-up turn behind a long cached prefix, speculative verification
of more than 16 rows per sequence at a moderate batch -- where that call's KH (T / TB + B) workgroups, each walking a whole key range
alone, do not fill the chip.  Every row block's key tiles are cut into `splits` chunks, a workgroup each; a merge kernel joins them.

    o = paged_prefill_attention_split(q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, window_left=None, sinks=None,
                                      num_splits=None, return_lse=False, workspace=None)          # o, or (o, lse)
    paged_prefill_attention_split_into(o, lse, q, ..., num_splits=None, workspace=None)           # nothing allocated: captured graphs
    splits, workspace_bytes = paged_prefill_attention_split_plan(q, k_pages, v_pages, block_table, *, window_left=None, num_splits=None)

Arguments, shapes, strides, dtypes, semantics and host checks are paged_prefill_attention's (its module states them, and its checks run
here under its name); 16-bit pages only.  num_splits: None for the automatic count -- ceil(512 / (KH (T / TB + B))), at most a chunk of
8 key tiles of 32 out of ceil(max_pages page_size / 32) or, with a window, of (TB + window_left) / 32 + 2, within 1 ... 64: host values
alone, and 1 wherever the unsplit call already fills the chip -- or 1 ... 64 to force it.  workspace: float32 or bytes, the plan's size
(4 T QH splits (E + 2), 0 at one split), allocated here when the caller brings none -- except by the _into form, which allocates nothing;
it may hold anything on entry, NaN included.  At a resolved count of 1 no merge runs and o and lse are paged_prefill_attention's bit for
bit.

Contracts (the header states them in full): paged_prefill_attention's with the resolved split count added to what the bits depend on.
No sync, no allocation in the library, no atomics, a fixed merge order; two runs are bitwise equal; a captured graph follows
cu_seqlens_q, seqlens, the table and the pages at fixed T, B and split count.  Masking is by selection.  At a FIXED count a sequence's
bits do not depend on P, on where its pages lie, on page_size or on the other sequences of the call; the automatic count depends on T
and B.

No autograd, GPU-only, no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_paged_prefill_split
from ._common import NNopError, _on_device, _ptr, _raise, _stream
from ._lib_paged_prefill_split import MAX_SPLITS
from .paged_prefill import _desc as _prefill_desc, _side, _tensor

__all__ = ["paged_prefill_attention_split", "paged_prefill_attention_split_into", "paged_prefill_attention_split_plan"]

FN = "paged_prefill_attention_split"


def _desc(q, k_pages, v_pages, block_table, window_left, num_splits, o=None):
    """paged_prefill_attention's host checks and descriptor, with the split count where that call keeps 0"""
    d = _prefill_desc(q, k_pages, v_pages, block_table, window_left, o)
    if num_splits is not None:
        if isinstance(num_splits, bool) or not isinstance(num_splits, int):
            raise TypeError(f"{FN}: num_splits must be None or an int, got {num_splits!r}")
        if not 1 <= num_splits <= MAX_SPLITS:
            raise ValueError(f"{FN}: num_splits must be 1 ... {MAX_SPLITS}, got {num_splits}")
        d.reserved = num_splits
    return d


def _plan(d):
    if d.tokens == 0:                                                           # nothing to launch: the library is not asked
        return 1, 0
    splits, nbytes = C.c_int32(0), C.c_size_t(0)
    _raise(_lib_paged_prefill_split.load().nnop_paged_prefill_split_plan(C.byref(d), C.byref(splits), C.byref(nbytes)))
    return splits.value, nbytes.value


def paged_prefill_attention_split_plan(q, k_pages, v_pages, block_table, *, window_left=None, num_splits=None):
    """(splits, workspace_bytes) the call will use for these tensors: host-only, from shapes alone, after every check of the call."""
    return _plan(_desc(q, k_pages, v_pages, block_table, window_left, num_splits))


def _run(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, window_left, sinks, num_splits, workspace, want_lse=False):
    """every check, then o, lse and the workspace where the caller brought none (o is None), then the call; with no token at all
    nothing is launched"""
    d = _desc(q, k_pages, v_pages, block_table, window_left, num_splits, o)
    (T, QH, E), B = q.shape, block_table.size(0)
    if lse is not None:
        _side("lse", lse, (T, QH), torch.float32, q)
    _side("cu_seqlens_q", cu_seqlens_q, (B + 1,), torch.int32, q)
    _side("seqlens", seqlens, (B,), torch.int32, q)
    if sinks is not None:
        _side("sinks", sinks, (QH,), torch.float32, q)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.device != q.device or not workspace.is_contiguous()):
        raise NNopError(f"{FN}: workspace must be a contiguous tensor on q's device", _lib.NNOP_ERR_WORKSPACE)
    need = _plan(d)[1]
    with _on_device(q):
        if o is None:
            o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
            lse = torch.empty((T, QH), dtype=torch.float32, device=q.device) if want_lse else None
            if workspace is None and need:
                workspace = torch.empty(need // 4, dtype=torch.float32, device=q.device)
        have = 0 if workspace is None else workspace.numel() * workspace.element_size()
        if T:
            _raise(_lib_paged_prefill_split.load().nnop_paged_prefill_split(
                C.byref(d), _ptr(o), _ptr(lse), _ptr(q), _ptr(k_pages), _ptr(v_pages), _ptr(block_table), _ptr(cu_seqlens_q),
                _ptr(seqlens), _ptr(sinks), _ptr(workspace) if have else None, have, _stream(q)))
    return o if lse is None else (o, lse)


def paged_prefill_attention_split_into(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, window_left=None, sinks=None,
                                       num_splits=None, workspace=None):
    """Writes o (q's shape and dtype, strides of its own) and, unless it is None, lse [T, QH] float32.  Nothing is allocated -- the form
    for captured graphs -- so beyond one split the caller brings a `workspace` of paged_prefill_attention_split_plan's size."""
    _tensor("o", o, 3)
    return _run(o, lse, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, window_left, sinks, num_splits, workspace)


def paged_prefill_attention_split(q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, *, window_left=None, sinks=None,
                                  num_splits=None, return_lse=False, workspace=None):
    """o [T, QH, E], or (o, lse [T, QH] float32): every sequence's new tokens against its pages, aligned to the sequence's end."""
    return _run(None, None, q, k_pages, v_pages, block_table, cu_seqlens_q, seqlens, window_left, sinks, num_splits, workspace,
                want_lse=return_lse)
