"""Host-side mirror of NNop's RMSNorm and LayerNorm operators (src/rms_norm.jl, src/layer_norm.jl) over the C ABI.

    y = rms_norm(x, w, eps=1e-6, offset=0.0)                 # rms_norm.jl:171-176, differentiable (rrule :178-185)
    y, rms = _rms_norm(x, w, eps=..., offset=...)            # :117-137
    dx, dw = grad_rms_norm(dy, rms, x, w, offset=...)        # ∇rms_norm :139-169 (dw is float32, :146)
    y = layer_norm(x, w, b, eps=1e-6)                        # layer_norm.jl:206-211 (rrule :213-220)
    y, mu, sigma = _layer_norm(x, w, b, eps=...)             # :150-170
    dx, dw, db = grad_layer_norm(dy, mu, sigma, x, w, b)     # ∇layer_norm :172-204

Residual add fused into the norm (no counterpart in the reference; include/nnop_hip.h, nnop_add_rms_norm):

    y, h = add_rms_norm(x, residual, w, eps=1e-6, offset=0.0)            # h = x + residual, y = rms_norm(h); differentiable
    y, h, rms = _add_rms_norm(x, residual, w, eps=..., offset=..., h_out=None)
    dx, dw = grad_add_rms_norm(dy, dh, rms, h, w, offset=..., dx_out=None)   # dx = d/dx = d/dresidual, dh may be None
    y, h = add_layer_norm(x, residual, w, b, eps=1e-6)
    y, h, mu, sigma = _add_layer_norm(x, residual, w, b, eps=..., h_out=None)
    dx, dw, db = grad_add_layer_norm(dy, dh, mu, sigma, h, w, b, dx_out=None)

Layout: x [n, emb] == Julia (emb, n); w, b [emb] in float32 or the dtype of x.  GPU-only like the reference kernels.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._common import NNopError, _DTYPES, _on_device, _ptr, _raise, _stream
from ._lib import NormDesc

__all__ = ["rms_norm", "_rms_norm", "grad_rms_norm", "layer_norm", "_layer_norm", "grad_layer_norm",
           "add_rms_norm", "_add_rms_norm", "grad_add_rms_norm", "add_layer_norm", "_add_layer_norm", "grad_add_layer_norm"]


def _check(x, w, b=None):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise TypeError("`x` must be a matrix [n, emb]")
    if not x.is_cuda:
        raise NNopError("NNop norms are GPU-only: tensors must live on a HIP device "
                        "(there is no CPU or PyTorch fallback).")
    if x.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {x.dtype}; expected float32, float16 or bfloat16")
    if x.shape[0] == 0 or x.shape[1] == 0:
        raise NNopError("norms need a non-empty matrix")
    for name, t in (("w", w), ("b", b)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.device != x.device:
            raise TypeError(f"`{name}` must be a vector on the device of x")
        if t.shape[0] != x.shape[1]:
            # the reference: @assert emb == length(w), src/rms_norm.jl:119
            raise NNopError(f"AssertionError: emb == length({name}) ({x.shape[1]} vs {t.shape[0]})")
        if t.dtype not in (torch.float32, x.dtype):
            raise TypeError(f"`{name}` must be float32 or share the dtype of x")
    if b is not None and b.dtype != w.dtype:
        raise TypeError("w and b must share one dtype")


def _desc(x, w):
    return NormDesc(dtype=_DTYPES[x.dtype], w_dtype=_DTYPES[w.dtype], emb=x.shape[1], reserved=0, n=x.shape[0])


def _workspace(d, ln, device):
    nbytes = int(_lib.load().nnop_norm_bwd_workspace_bytes(C.byref(d), 1 if ln else 0))
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device), nbytes


def _rms_norm(x, w, *, eps: float = 1e-6, offset: float = 0.0):
    """``NNop._rms_norm(x, w; ϵ, offset)`` -> (y, rms)."""
    _check(x, w)
    x, w = x.contiguous(), w.contiguous()
    y = torch.empty_like(x)
    rms = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    with _on_device(x):
        _raise(_lib.load().nnop_rms_norm(C.byref(_desc(x, w)), _ptr(y), _ptr(rms), _ptr(x), _ptr(w),
                                         C.c_float(offset), C.c_float(eps), _stream(x)))
    return y, rms


def grad_rms_norm(dy, rms, x, w, *, offset: float = 0.0):
    """``∇rms_norm(Δ, rms, x, w; offset)`` -> (dx, dw) with dw in float32."""
    _check(x, w)
    if dy.shape != x.shape or dy.dtype != x.dtype or dy.device != x.device:
        raise TypeError("Δ must match x in shape, dtype and device")
    if rms.dtype != torch.float32 or tuple(rms.shape) != (x.shape[0],):
        raise TypeError("rms must be a float32 vector [n]")
    dy, x, w, rms = dy.contiguous(), x.contiguous(), w.contiguous(), rms.contiguous()
    d = _desc(x, w)
    dx = torch.empty_like(x)
    dw = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(d, False, x.device)
    with _on_device(x):
        _raise(_lib.load().nnop_rms_norm_bwd(C.byref(d), _ptr(dx), _ptr(dw), _ptr(dy), _ptr(rms), _ptr(x), _ptr(w),
                                             C.c_float(offset), _ptr(ws), C.c_size_t(nbytes), _stream(x)))
    return dx, dw


def _layer_norm(x, w, b, *, eps: float = 1e-6):
    """``NNop._layer_norm(x, w, b; ϵ)`` -> (y, μ, Σ)."""
    _check(x, w, b)
    x, w, b = x.contiguous(), w.contiguous(), b.contiguous()
    y = torch.empty_like(x)
    mu = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    sigma = torch.empty_like(mu)
    with _on_device(x):
        _raise(_lib.load().nnop_layer_norm(C.byref(_desc(x, w)), _ptr(y), _ptr(mu), _ptr(sigma), _ptr(x), _ptr(w),
                                           _ptr(b), C.c_float(eps), _stream(x)))
    return y, mu, sigma


def grad_layer_norm(dy, mu, sigma, x, w, b=None):
    """``∇layer_norm(Δ, μ, Σ, x, w, b)`` -> (dx, dw, db); dw, db in the dtype of w (src/layer_norm.jl:179-180)."""
    _check(x, w, b)
    if dy.shape != x.shape or dy.dtype != x.dtype or dy.device != x.device:
        raise TypeError("Δ must match x in shape, dtype and device")
    for s in (mu, sigma):
        if s.dtype != torch.float32 or tuple(s.shape) != (x.shape[0],):
            raise TypeError("μ and Σ must be float32 vectors [n]")
    dy, x, w, mu, sigma = dy.contiguous(), x.contiguous(), w.contiguous(), mu.contiguous(), sigma.contiguous()
    d = _desc(x, w)
    dx = torch.empty_like(x)
    dw, db = torch.empty_like(w), torch.empty_like(w)
    ws, nbytes = _workspace(d, True, x.device)
    with _on_device(x):
        _raise(_lib.load().nnop_layer_norm_bwd(C.byref(d), _ptr(dx), _ptr(dw), _ptr(db), _ptr(dy), _ptr(mu), _ptr(sigma),
                                               _ptr(x), _ptr(w), _ptr(ws), C.c_size_t(nbytes), _stream(x)))
    return dx, dw, db


class _RMSNorm(torch.autograd.Function):
    """rrule of src/rms_norm.jl:178-185."""

    @staticmethod
    def forward(ctx, x, w, eps, offset):
        y, rms = _rms_norm(x, w, eps=eps, offset=offset)
        ctx.save_for_backward(rms, x, w)
        ctx.offset = offset
        return y

    @staticmethod
    def backward(ctx, dy):
        rms, x, w = ctx.saved_tensors
        dx, dw = grad_rms_norm(dy, rms, x, w, offset=ctx.offset)
        return dx, dw.to(w.dtype), None, None


class _LayerNorm(torch.autograd.Function):
    """rrule of src/layer_norm.jl:213-220."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        y, mu, sigma = _layer_norm(x, w, b, eps=eps)
        ctx.save_for_backward(mu, sigma, x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        mu, sigma, x, w = ctx.saved_tensors
        dx, dw, db = grad_layer_norm(dy, mu, sigma, x, w)
        return dx, dw, db, None


def rms_norm(x, w, *, eps: float = 1e-6, offset: float = 0.0):
    """``NNop.rms_norm(x, w; ϵ=1f-6, offset=0f0)`` (src/rms_norm.jl:171-176)."""
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        _check(x, w)
        return _RMSNorm.apply(x, w, float(eps), float(offset))
    return _rms_norm(x, w, eps=eps, offset=offset)[0]


def layer_norm(x, w, b, *, eps: float = 1e-6):
    """``NNop.layer_norm(x, w, b; ϵ=1f-6)`` (src/layer_norm.jl:206-211)."""
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad):
        _check(x, w, b)
        return _LayerNorm.apply(x, w, b, float(eps))
    return _layer_norm(x, w, b, eps=eps)[0]


# ---- residual add fused into the norm ----------------------------------------------------------------------------------

def _check_like(x, **others):
    """`residual`, `dy`, `dh`: matrices that must match x in shape, dtype and device"""
    for name, t in others.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.shape != x.shape or t.dtype != x.dtype or t.device != x.device:
            raise TypeError(f"`{name}` must match x in shape, dtype and device")


def _check_out(name, out, x, may_be):
    """A caller's output buffer: contiguous, like x; it may be one of `may_be` itself (the in-place forms), and then that
    tensor must be contiguous too, since the library is handed its own storage."""
    if out is None:
        return
    _check_like(x, **{name: out})
    if not out.is_contiguous():
        raise TypeError(f"`{name}` must be contiguous")
    if not any(out is t for t in may_be) and any(t is not None and out.data_ptr() == t.data_ptr() for t in may_be):
        raise TypeError(f"`{name}` may alias an input only by being that very tensor")


def _add_rms_norm(x, residual, w, *, eps: float = 1e-6, offset: float = 0.0, h_out=None):
    """h = x + residual (rounded once to the dtype of x), y = rms_norm(h) -> (y, h, rms).  `h_out` may be `x` or `residual`
    (the in-place update of the residual stream) or any other matrix like x; by default h is a new tensor."""
    _check(x, w)
    _check_like(x, residual=residual)
    _check_out("h_out", h_out, x, (x, residual))
    x, residual, w = x.contiguous(), residual.contiguous(), w.contiguous()
    h = torch.empty_like(x) if h_out is None else h_out
    y = torch.empty_like(x)
    rms = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    with _on_device(x):
        _raise(_lib.load().nnop_add_rms_norm(C.byref(_desc(x, w)), _ptr(y), _ptr(h), _ptr(rms), _ptr(x), _ptr(residual),
                                             _ptr(w), C.c_float(offset), C.c_float(eps), _stream(x)))
    return y, h, rms


def grad_add_rms_norm(dy, dh, rms, h, w, *, offset: float = 0.0, dx_out=None):
    """Pullback of `_add_rms_norm`: dy, dh are the cotangents of y and of h (dh may be None) -> (dx, dw); dx is the gradient
    of x and of residual alike, dw is float32.  `dx_out` may be `dh` (accumulate into the stream's gradient)."""
    _check(h, w)
    _check_like(h, dy=dy, dh=dh)
    _check_out("dx_out", dx_out, h, (dh,))
    if rms.dtype != torch.float32 or tuple(rms.shape) != (h.shape[0],):
        raise TypeError("rms must be a float32 vector [n]")
    dy, h, w, rms = dy.contiguous(), h.contiguous(), w.contiguous(), rms.contiguous()
    dh = dh.contiguous() if dh is not None else None
    d = _desc(h, w)
    dx = torch.empty_like(h) if dx_out is None else dx_out
    dw = torch.empty(h.shape[1], dtype=torch.float32, device=h.device)
    ws, nbytes = _workspace(d, False, h.device)
    with _on_device(h):
        _raise(_lib.load().nnop_add_rms_norm_bwd(C.byref(d), _ptr(dx), _ptr(dw), _ptr(dy), _ptr(dh), _ptr(rms), _ptr(h),
                                                 _ptr(w), C.c_float(offset), _ptr(ws), C.c_size_t(nbytes), _stream(h)))
    return dx, dw


def _add_layer_norm(x, residual, w, b, *, eps: float = 1e-6, h_out=None):
    """h = x + residual (rounded once to the dtype of x), y = layer_norm(h) -> (y, h, mu, sigma); `h_out` as in `_add_rms_norm`."""
    _check(x, w, b)
    _check_like(x, residual=residual)
    _check_out("h_out", h_out, x, (x, residual))
    x, residual, w, b = x.contiguous(), residual.contiguous(), w.contiguous(), b.contiguous()
    h = torch.empty_like(x) if h_out is None else h_out
    y = torch.empty_like(x)
    mu = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    sigma = torch.empty_like(mu)
    with _on_device(x):
        _raise(_lib.load().nnop_add_layer_norm(C.byref(_desc(x, w)), _ptr(y), _ptr(h), _ptr(mu), _ptr(sigma), _ptr(x),
                                               _ptr(residual), _ptr(w), _ptr(b), C.c_float(eps), _stream(x)))
    return y, h, mu, sigma


def grad_add_layer_norm(dy, dh, mu, sigma, h, w, b=None, *, dx_out=None):
    """Pullback of `_add_layer_norm` -> (dx, dw, db); dh may be None, `dx_out` may be `dh`; dw, db in the dtype of w."""
    _check(h, w, b)
    _check_like(h, dy=dy, dh=dh)
    _check_out("dx_out", dx_out, h, (dh,))
    for s in (mu, sigma):
        if s.dtype != torch.float32 or tuple(s.shape) != (h.shape[0],):
            raise TypeError("μ and Σ must be float32 vectors [n]")
    dy, h, w, mu, sigma = dy.contiguous(), h.contiguous(), w.contiguous(), mu.contiguous(), sigma.contiguous()
    dh = dh.contiguous() if dh is not None else None
    d = _desc(h, w)
    dx = torch.empty_like(h) if dx_out is None else dx_out
    dw, db = torch.empty_like(w), torch.empty_like(w)
    ws, nbytes = _workspace(d, True, h.device)
    with _on_device(h):
        _raise(_lib.load().nnop_add_layer_norm_bwd(C.byref(d), _ptr(dx), _ptr(dw), _ptr(db), _ptr(dy), _ptr(dh), _ptr(mu),
                                                   _ptr(sigma), _ptr(h), _ptr(w), _ptr(ws), C.c_size_t(nbytes), _stream(h)))
    return dx, dw, db


class _AddRMSNorm(torch.autograd.Function):
    """Two outputs (y, h); one input gradient, shared by x and residual.  Never in place."""

    @staticmethod
    def forward(ctx, x, residual, w, eps, offset):
        y, h, rms = _add_rms_norm(x, residual, w, eps=eps, offset=offset)
        ctx.save_for_backward(rms, h, w)
        ctx.offset = offset
        ctx.set_materialize_grads(False)           # an unused h reaches the library as dh = NULL, not as zeros
        return y, h

    @staticmethod
    def backward(ctx, dy, dh):
        rms, h, w = ctx.saved_tensors
        if dy is None:                             # only h was used: the add alone
            return dh, dh, (torch.zeros_like(w) if dh is not None else None), None, None
        dx, dw = grad_add_rms_norm(dy, dh, rms, h, w, offset=ctx.offset)
        return dx, dx, dw.to(w.dtype), None, None


class _AddLayerNorm(torch.autograd.Function):
    """Two outputs (y, h); one input gradient, shared by x and residual.  Never in place."""

    @staticmethod
    def forward(ctx, x, residual, w, b, eps):
        y, h, mu, sigma = _add_layer_norm(x, residual, w, b, eps=eps)
        ctx.save_for_backward(mu, sigma, h, w)
        ctx.set_materialize_grads(False)
        return y, h

    @staticmethod
    def backward(ctx, dy, dh):
        mu, sigma, h, w = ctx.saved_tensors
        if dy is None:
            z = torch.zeros_like(w) if dh is not None else None
            return dh, dh, z, z, None
        dx, dw, db = grad_add_layer_norm(dy, dh, mu, sigma, h, w)
        return dx, dx, dw, db, None


def add_rms_norm(x, residual, w, *, eps: float = 1e-6, offset: float = 0.0):
    """(y, h) with h = x + residual and y = rms_norm(h; ϵ, offset): the pre-norm block's add and norm in one pass."""
    if torch.is_grad_enabled() and (x.requires_grad or residual.requires_grad or w.requires_grad):
        _check(x, w)
        _check_like(x, residual=residual)
        return _AddRMSNorm.apply(x, residual, w, float(eps), float(offset))
    return _add_rms_norm(x, residual, w, eps=eps, offset=offset)[:2]


def add_layer_norm(x, residual, w, b, *, eps: float = 1e-6):
    """(y, h) with h = x + residual and y = layer_norm(h; ϵ)."""
    if torch.is_grad_enabled() and (x.requires_grad or residual.requires_grad or w.requires_grad or b.requires_grad):
        _check(x, w, b)
        _check_like(x, residual=residual)
        return _AddLayerNorm.apply(x, residual, w, b, float(eps))
    return _add_layer_norm(x, residual, w, b, eps=eps)[:2]
