"""Mixture-of-experts routing over the C ABI of the third library (include/nnop_hip_moe.h; no counterpart in the reference).

The gate -- top-k over the expert logits, the routing weights, the row's log-sum-exp -- as one kernel each way, and the expert
dispatch plan (a stable counting sort of the assignments by expert) as a fixed four-kernel sequence:

    w, idx = moe_router(logits, k, norm="topk")                   # differentiable in logits; leading dims are flattened to T
    w, idx, lse = moe_router(logits, k, norm="all", return_lse=True)      # lse differentiable too (router z-loss)
    w, idx, lse = _moe_router(logits, k, norm=...)
    dlogits = grad_moe_router(dw, w, idx, lse, logits, norm=..., dlse=None, out=None)
    counts, offsets, perm, slot = moe_dispatch_plan(idx, num_experts)
    moe_router_into(w, idx, lse, logits, k, norm=...)             # caller-owned buffers
    grad_moe_router_into(dlogits, dw, w, idx, lse, logits, norm=..., dlse=None)
    moe_dispatch_plan_into(counts, offsets, perm, slot, idx, num_experts, workspace=None)

It replaces softmax / topk / gather / renormalise and argsort / bincount / cumsum with their autograd.  logits [..., E] in float32,
float16 or bfloat16 (a 2-D logits may have a row stride above E: the padding columns are neither read nor written); w, lse float32,
idx int32.  norm="topk": softmax over the k selected logits (gpt-oss, Mixtral, Qwen3 with norm_topk_prob); norm="all": the full
softmax, gathered and not renormalised (Qwen-MoE, OLMoE).  Ties go to the lower expert index; NaN ranks above +inf.
`perm // k` is the token of each expert-sorted slot, `offsets` delimits the experts' row ranges, `slot` brings the rows back:
INTEGRATION.md shows the composition.  GPU-only: no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import numbers

import torch

from . import _lib, _lib_moe
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_moe import MoePlanDesc, MoeRouterDesc, NORMS, MAX_EXPERTS, MAX_TOPK

__all__ = ["moe_router", "_moe_router", "grad_moe_router", "moe_router_into", "grad_moe_router_into", "moe_dispatch_plan",
           "moe_dispatch_plan_into"]


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError(f"`{name}` must be an integer, got {v!r}")
    return int(v)


def _check(logits, k, norm):
    """-> (T, E, k): raises before any device work"""
    if not isinstance(logits, torch.Tensor) or logits.dim() < 1:
        raise TypeError("`logits` must be a tensor [..., E]")
    if not logits.is_cuda:
        raise NNopError("NNop moe_router is GPU-only: tensors must live on a HIP device "
                        "(there is no CPU or PyTorch fallback).")
    if logits.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {logits.dtype}; expected float32, float16 or bfloat16")
    k = _int("k", k)
    if norm not in NORMS:
        raise NNopError(f"norm must be one of {sorted(NORMS)}, got {norm!r}", _lib.NNOP_ERR_OPTS)
    E = logits.shape[-1]
    T = logits.numel() // E if E else 0
    if not 1 <= E <= MAX_EXPERTS:
        raise NNopError(f"the number of experts must be in 1 ... {MAX_EXPERTS}, got {E}", _lib.NNOP_ERR_SHAPE)
    if not 1 <= k <= min(E, MAX_TOPK):
        raise NNopError(f"k must be in 1 ... min(E, {MAX_TOPK}) = {min(E, MAX_TOPK)}, got {k}", _lib.NNOP_ERR_SHAPE)
    if T < 1:
        raise NNopError("moe_router needs non-empty logits", _lib.NNOP_ERR_SHAPE)
    if T * k > 2 ** 31 - 1:
        raise NNopError("T * k must be below 2^31", _lib.NNOP_ERR_SHAPE)
    return T, E, k


def _rows(logits, E):
    """logits as the library reads it: (tensor, ld).  A 2-D tensor with unit column stride is taken as it is, row stride and all."""
    if logits.dim() == 2 and (E == 1 or logits.stride(1) == 1) and (logits.shape[0] == 1 or E <= logits.stride(0) < 2 ** 31):
        return logits, (E if logits.shape[0] == 1 else logits.stride(0))
    return logits.contiguous(), E


def _check_buf(name, t, shape, dtype, like):
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != like.device
            or not t.is_contiguous()):
        raise NNopError(f"`{name}` must be a dense {_dtype_name(dtype)} tensor of shape {tuple(shape)} on the device of logits")


def _desc(logits, T, E, k, ld, norm):
    return MoeRouterDesc(dtype=_DTYPES[logits.dtype], tokens=T, experts=E, topk=k, ld=ld, norm=NORMS[norm])


def moe_router_into(w, idx, lse, logits, k, *, norm: str = "topk"):
    """Lowest-level forward: writes w [..., k] float32, idx [..., k] int32 and lse [...] float32, caller-owned and dense."""
    T, E, k = _check(logits, k, norm)
    lead = tuple(logits.shape[:-1])
    _check_buf("w", w, lead + (k,), torch.float32, logits)
    _check_buf("idx", idx, lead + (k,), torch.int32, logits)
    _check_buf("lse", lse, lead, torch.float32, logits)
    x, ld = _rows(logits, E)
    d = _desc(logits, T, E, k, ld, norm)
    with _on_device(logits):
        _raise(_lib_moe.load().nnop_moe_router(C.byref(d), _ptr(idx), _ptr(w), _ptr(lse), _ptr(x), _stream(logits)))
    return w, idx, lse


def _moe_router(logits, k, *, norm: str = "topk"):
    """(w, idx, lse) as new tensors."""
    T, E, k = _check(logits, k, norm)
    lead = tuple(logits.shape[:-1])
    with _on_device(logits):
        w = torch.empty(lead + (k,), dtype=torch.float32, device=logits.device)
        idx = torch.empty(lead + (k,), dtype=torch.int32, device=logits.device)
        lse = torch.empty(lead, dtype=torch.float32, device=logits.device)
    return moe_router_into(w, idx, lse, logits, k, norm=norm)


def grad_moe_router_into(dlogits, dw, w, idx, lse, logits, *, norm: str = "topk", dlse=None):
    """Lowest-level pullback: writes dlogits, which has the shape, dtype and strides of logits; its padding columns stay as they are."""
    k = w.shape[-1] if isinstance(w, torch.Tensor) and w.dim() >= 1 else 0
    T, E, k = _check(logits, k, norm)
    lead = tuple(logits.shape[:-1])
    _check_buf("dw", dw, lead + (k,), torch.float32, logits)
    _check_buf("w", w, lead + (k,), torch.float32, logits)
    _check_buf("idx", idx, lead + (k,), torch.int32, logits)
    _check_buf("lse", lse, lead, torch.float32, logits)
    if dlse is not None:
        _check_buf("dlse", dlse, lead, torch.float32, logits)
    x, ld = _rows(logits, E)
    if (not isinstance(dlogits, torch.Tensor) or dlogits.shape != logits.shape or dlogits.dtype != logits.dtype
            or dlogits.device != logits.device):
        raise NNopError("`dlogits` must match logits in shape, dtype and device")
    y, ld_y = _rows(dlogits, E)
    if y is not dlogits or (T > 1 and ld_y != ld):                # (_rows would have copied it, or the strides differ)
        raise NNopError("`dlogits` must be dense like logits, or 2-D with the row stride of logits")
    d = _desc(logits, T, E, k, ld, norm)
    with _on_device(logits):
        _raise(_lib_moe.load().nnop_moe_router_bwd(C.byref(d), _ptr(dlogits), _ptr(dw), _ptr(dlse), _ptr(w), _ptr(idx), _ptr(lse),
                                                   _ptr(x), _stream(logits)))
    return dlogits


def grad_moe_router(dw, w, idx, lse, logits, *, norm: str = "topk", dlse=None, out=None):
    """Pullback of `_moe_router`: (dw, dlse) -> dlogits in the dtype of logits.  `out`: see grad_moe_router_into."""
    if out is None:
        k = w.shape[-1] if isinstance(w, torch.Tensor) and w.dim() >= 1 else 0
        _check(logits, k, norm)
        logits = logits.contiguous()
        with _on_device(logits):
            out = torch.empty_like(logits)
    return grad_moe_router_into(out, dw, w, idx, lse, logits, norm=norm, dlse=dlse)


class _MoeRouter(torch.autograd.Function):
    """logits gets the pullback's gradient from the cotangents of w and lse; idx carries none."""

    @staticmethod
    def forward(ctx, logits, k, norm):
        w, idx, lse = _moe_router(logits, k, norm=norm)
        ctx.save_for_backward(logits, w, idx, lse)
        ctx.norm = norm
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return w, idx, lse

    @staticmethod
    def backward(ctx, dw, _didx, dlse):
        logits, w, idx, lse = ctx.saved_tensors
        dw = torch.zeros_like(w) if dw is None else dw.to(torch.float32).contiguous()
        if dlse is not None:
            dlse = dlse.to(torch.float32).contiguous()
        return grad_moe_router(dw, w, idx, lse, logits, norm=ctx.norm, dlse=dlse), None, None


def moe_router(logits, k, norm: str = "topk", return_lse: bool = False):
    """(w, idx) -- or (w, idx, lse) -- of the top-k gate over logits [..., E]."""
    _check(logits, k, norm)
    if torch.is_grad_enabled() and logits.requires_grad:
        out = _MoeRouter.apply(logits, int(k), norm)
    else:
        out = _moe_router(logits, k, norm=norm)
    return out if return_lse else out[:2]


# ---- the dispatch plan --------------------------------------------------------------------------------------------------------------
def _check_plan(idx, num_experts):
    """-> (T, k, E)"""
    if not isinstance(idx, torch.Tensor) or idx.dim() < 1:
        raise TypeError("`idx` must be a tensor [..., k]")
    if not idx.is_cuda:
        raise NNopError("NNop moe_dispatch_plan is GPU-only: tensors must live on a HIP device "
                        "(there is no CPU or PyTorch fallback).")
    if idx.dtype != torch.int32:
        raise TypeError(f"`idx` must be int32, got {idx.dtype}")
    E = _int("num_experts", num_experts)
    if not 1 <= E <= MAX_EXPERTS:
        raise NNopError(f"num_experts must be in 1 ... {MAX_EXPERTS}, got {E}", _lib.NNOP_ERR_SHAPE)
    k = idx.shape[-1]
    T = idx.numel() // k if k else 0
    if T < 1 or k < 1:
        raise NNopError("moe_dispatch_plan needs a non-empty idx", _lib.NNOP_ERR_SHAPE)
    if T * k > 2 ** 31 - 1:
        raise NNopError("T * k must be below 2^31", _lib.NNOP_ERR_SHAPE)
    return T, k, E


def moe_dispatch_plan_into(counts, offsets, perm, slot, idx, num_experts, *, workspace=None):
    """Lowest-level plan: writes counts [E], offsets [E + 1], perm [T k] and slot (the shape of idx), all int32 and dense.
    `workspace`: a dense uint8 tensor of at least the library's workspace size, 16-byte aligned; by default one is allocated."""
    T, k, E = _check_plan(idx, num_experts)
    _check_buf("counts", counts, (E,), torch.int32, idx)
    _check_buf("offsets", offsets, (E + 1,), torch.int32, idx)
    _check_buf("perm", perm, (T * k,), torch.int32, idx)
    _check_buf("slot", slot, tuple(idx.shape), torch.int32, idx)
    idx = idx.contiguous()
    d = MoePlanDesc(tokens=T, topk=k, experts=E)
    lib = _lib_moe.load()
    nbytes = int(lib.nnop_moe_plan_workspace_bytes(C.byref(d)))
    if nbytes == 0:
        raise NNopError(_lib.strerror(_lib.NNOP_ERR_SHAPE), _lib.NNOP_ERR_SHAPE)
    if workspace is None:
        with _on_device(idx):
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=idx.device)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != idx.device
          or not workspace.is_contiguous() or workspace.numel() < nbytes):
        raise NNopError(f"`workspace` must be a dense uint8 tensor of at least {nbytes} bytes on the device of idx",
                        _lib.NNOP_ERR_WORKSPACE)
    with _on_device(idx):
        _raise(lib.nnop_moe_plan(C.byref(d), _ptr(counts), _ptr(offsets), _ptr(perm), _ptr(slot), _ptr(idx), _ptr(workspace),
                                 C.c_size_t(workspace.numel()), _stream(idx)))
    return counts, offsets, perm, slot


def moe_dispatch_plan(idx, num_experts):
    """(counts [E], offsets [E + 1], perm [T k], slot like idx), int32: the expert-sorted order of the assignments in idx [..., k]."""
    T, k, E = _check_plan(idx, num_experts)
    with _on_device(idx):
        new = lambda *s: torch.empty(s, dtype=torch.int32, device=idx.device)
        counts, offsets, perm, slot = new(E), new(E + 1), new(T * k), new(*idx.shape)
    return moe_dispatch_plan_into(counts, offsets, perm, slot, idx, num_experts)
