"""Fused QK-norm + RoPE over the C ABI of the extension library (include/nnop_hip_ext.h; no counterpart in the reference).

The per-head RMSNorm that Qwen3, Gemma 3 and OLMo 2 put on q and k, then the Llama rotary embedding, in one pass:

    q2, k2 = qk_norm_rope(q, k, wq, wk, cos=cos, sin=sin, eps=1e-6, offset=0.0)      # differentiable in q, k, wq, wk
    q2, k2 = _qk_norm_rope(q, k, wq, wk, cos, sin, eps=..., offset=...)
    dq, dk, dwq, dwk = grad_qk_norm_rope((dq2, dk2), q, k, wq, wk, cos, sin, eps=..., offset=...)   # dwq, dwk float32
    qk_norm_rope_into(q_out, k_out, q, k, wq, wk, cos, sin, eps=..., offset=...)     # q_out may be q, k_out may be k
    grad_qk_norm_rope_into(dq, dk, dwq, dwk, (dq2, dk2), q, k, wq, wk, cos, sin, ...)   # dq may be dq2, dk may be dk2

It replaces ``rms_norm(q.view(-1, D), wq)``, ``rms_norm(k.view(-1, D), wk)`` and ``llama_rope``.  Layout as for ``llama_rope``:
q [B, QH, L, D], k [B, KH, L, D], cos/sin [B, L, D]; wq, wk [D] in float32 or the dtype of q.  The forward saves nothing: the
pullback recomputes the row statistics from q and k.  GPU-only: no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib, _lib_ext
from ._common import NNopError, _DTYPES, _on_device, _ptr, _raise, _stream
from ._lib_ext import QknrDesc

__all__ = ["qk_norm_rope", "_qk_norm_rope", "grad_qk_norm_rope", "qk_norm_rope_into", "grad_qk_norm_rope_into"]


def _check(q, k, wq, wk, cos, sin, eps, offset):
    for name, t in (("q", q), ("k", k)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise TypeError(f"`{name}` must be a 4-D tensor [B, H, L, D]")
    if not q.is_cuda:
        raise NNopError("NNop qk_norm_rope is GPU-only: tensors must live on a HIP device "
                        "(there is no CPU or PyTorch fallback).")
    if q.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {q.dtype}; expected float32, float16 or bfloat16")
    if k.dtype != q.dtype or k.device != q.device:
        raise TypeError("q and k must share one dtype and device")
    B, QH, L, D = q.shape
    if k.shape[3] != D or k.shape[2] != L or k.shape[0] != B:
        raise NNopError(f"AssertionError: q {tuple(q.shape)} and k {tuple(k.shape)} must agree in head dim, "
                        "sequence length and batch.")
    if min(B, QH, k.shape[1], L, D) < 1:
        raise NNopError("qk_norm_rope needs non-empty q and k")
    if D % 2 or D > 512:
        raise NNopError("head dim must be even and at most 512")
    for name, t in (("wq", wq), ("wk", wk)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.device != q.device:
            raise TypeError(f"`{name}` must be a vector on the device of q")
        if t.shape[0] != D:
            raise NNopError(f"AssertionError: D == length({name}) ({D} vs {t.shape[0]})")
    if wq.dtype != wk.dtype or wq.dtype not in (torch.float32, q.dtype):
        raise TypeError("wq and wk must share one dtype: float32 or the dtype of q")
    for name, t in (("cos", cos), ("sin", sin)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, L, D) or t.device != q.device:
            raise NNopError(f"`{name}` must have shape [B, L, D] = {(B, L, D)} on the device of q")
    if cos.dtype != sin.dtype or cos.dtype not in (torch.float32, q.dtype):
        raise TypeError("cos and sin must share one dtype: float32 or the dtype of q")
    for name, v in (("eps", eps), ("offset", offset)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise TypeError(f"`{name}` must be a number, got {v!r}")
    if not math.isfinite(eps) or eps < 0 or not math.isfinite(offset):
        raise NNopError("eps must be finite and not negative, offset finite", _lib.NNOP_ERR_OPTS)


def _check_out(name, out, like, dtype=None):
    if (not isinstance(out, torch.Tensor) or out.shape != like.shape or out.dtype != (dtype or like.dtype)
            or out.device != like.device or not out.is_contiguous()):
        raise NNopError(f"`{name}` must be dense and match its input in shape, dtype and device")


def _desc(q, k, wq, cos, eps, offset):
    B, QH, L, D = q.shape
    return QknrDesc(dtype=_DTYPES[q.dtype], w_dtype=_DTYPES[wq.dtype], cs_dtype=_DTYPES[cos.dtype], dim=D, seq=L, qh=QH,
                    kh=k.shape[1], batch=B, eps=float(eps), offset=float(offset))


def _dense(*ts):
    return tuple(t if t.is_contiguous() else t.contiguous() for t in ts)


def qk_norm_rope_into(q_out, k_out, q, k, wq, wk, cos, sin, *, eps: float = 1e-6, offset: float = 0.0):
    """Lowest-level forward: writes into caller-owned buffers (q_out may be q, k_out may be k)."""
    _check(q, k, wq, wk, cos, sin, eps, offset)
    q, k, wq, wk, cos, sin = _dense(q, k, wq, wk, cos, sin)
    _check_out("q_out", q_out, q)
    _check_out("k_out", k_out, k)
    d = _desc(q, k, wq, cos, eps, offset)
    with _on_device(q):
        _raise(_lib_ext.load().nnop_qk_norm_rope(C.byref(d), _ptr(q_out), _ptr(k_out), _ptr(q), _ptr(k), _ptr(wq), _ptr(wk),
                                                 _ptr(cos), _ptr(sin), _stream(q)))
    return q_out, k_out


def _qk_norm_rope(q, k, wq, wk, cos, sin, *, eps: float = 1e-6, offset: float = 0.0):
    """(q2, k2) as new tensors."""
    _check(q, k, wq, wk, cos, sin, eps, offset)
    return qk_norm_rope_into(torch.empty_like(q, memory_format=torch.contiguous_format),
                             torch.empty_like(k, memory_format=torch.contiguous_format), q, k, wq, wk, cos, sin,
                             eps=eps, offset=offset)


def grad_qk_norm_rope_into(dq, dk, dwq, dwk, grads, q, k, wq, wk, cos, sin, *, eps: float = 1e-6, offset: float = 0.0,
                           workspace=None):
    """Lowest-level pullback: writes into caller-owned buffers (dq may be dq2, dk may be dk2; dwq, dwk float32 [D]).
    `workspace`: a dense uint8 tensor of at least the library's workspace size, 16-byte aligned; by default one is allocated."""
    _check(q, k, wq, wk, cos, sin, eps, offset)
    dq2, dk2 = grads
    for name, g, x in (("dq2", dq2, q), ("dk2", dk2, k)):
        if not isinstance(g, torch.Tensor) or g.shape != x.shape or g.dtype != x.dtype or g.device != x.device:
            raise TypeError(f"`{name}` must match its input in shape, dtype and device")
    q, k, wq, wk, cos, sin, dq2, dk2 = _dense(q, k, wq, wk, cos, sin, dq2, dk2)
    _check_out("dq", dq, q)
    _check_out("dk", dk, k)
    _check_out("dwq", dwq, wq, torch.float32)
    _check_out("dwk", dwk, wk, torch.float32)
    d = _desc(q, k, wq, cos, eps, offset)
    lib = _lib_ext.load()
    nbytes = int(lib.nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(d)))
    if nbytes == 0:
        raise NNopError(_lib.strerror(_lib.NNOP_ERR_SHAPE), _lib.NNOP_ERR_SHAPE)
    if workspace is None:
        with _on_device(q):
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != q.device
          or not workspace.is_contiguous() or workspace.numel() < nbytes):
        raise NNopError(f"`workspace` must be a dense uint8 tensor of at least {nbytes} bytes on the device of q",
                        _lib.NNOP_ERR_WORKSPACE)
    with _on_device(q):
        _raise(lib.nnop_qk_norm_rope_bwd(C.byref(d), _ptr(dq), _ptr(dk), _ptr(dwq), _ptr(dwk), _ptr(dq2), _ptr(dk2), _ptr(q),
                                         _ptr(k), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin), _ptr(workspace),
                                         C.c_size_t(workspace.numel()), _stream(q)))
    return dq, dk, dwq, dwk


def grad_qk_norm_rope(grads, q, k, wq, wk, cos, sin, *, eps: float = 1e-6, offset: float = 0.0):
    """Pullback of `_qk_norm_rope`: (dq2, dk2) -> (dq, dk, dwq, dwk), dwq and dwk in float32."""
    _check(q, k, wq, wk, cos, sin, eps, offset)
    D = q.shape[3]
    return grad_qk_norm_rope_into(torch.empty_like(q, memory_format=torch.contiguous_format),
                                  torch.empty_like(k, memory_format=torch.contiguous_format),
                                  torch.empty(D, dtype=torch.float32, device=q.device),
                                  torch.empty(D, dtype=torch.float32, device=q.device),
                                  grads, q, k, wq, wk, cos, sin, eps=eps, offset=offset)


class _QKNormRope(torch.autograd.Function):
    """q, k, wq, wk get the pullback's gradients (dwq, dwk cast to the dtype of the weights); cos, sin get no tangent."""

    @staticmethod
    def forward(ctx, q, k, wq, wk, cos, sin, eps, offset):
        ctx.save_for_backward(q, k, wq, wk, cos, sin)
        ctx.eps, ctx.offset = eps, offset
        return _qk_norm_rope(q, k, wq, wk, cos, sin, eps=eps, offset=offset)

    @staticmethod
    def backward(ctx, dq2, dk2):
        q, k, wq, wk, cos, sin = ctx.saved_tensors
        dq, dk, dwq, dwk = grad_qk_norm_rope((dq2, dk2), q, k, wq, wk, cos, sin, eps=ctx.eps, offset=ctx.offset)
        return dq, dk, dwq.to(wq.dtype), dwk.to(wk.dtype), None, None, None, None


def qk_norm_rope(q, k, wq, wk, *, cos, sin, eps: float = 1e-6, offset: float = 0.0):
    """(q2, k2) = llama_rope(rms_norm(q; wq), rms_norm(k; wk); cos, sin), the norm per head row, in one pass."""
    _check(q, k, wq, wk, cos, sin, eps, offset)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, wq, wk)):
        return _QKNormRope.apply(q, k, wq, wk, cos, sin, float(eps), float(offset))
    return _qk_norm_rope(q, k, wq, wk, cos, sin, eps=eps, offset=offset)
