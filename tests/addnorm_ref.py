"""Reference of the residual add fused into RMSNorm / LayerNorm (test infrastructure, not a test file).

include/nnop_hip.h (nnop_add_rms_norm): h = T(fp32(x) + fp32(residual)), one rounding to the element type T; the statistics and y are
those of the plain operator on the ROUNDED h; the pullback writes one gradient dx = g + dh, g being the plain pullback's input gradient
at (dy, h, w), and dx is the gradient of x and of residual alike.  Here h is formed on the CPU exactly as the contract says and the fp64
formulas of oracle/naive_norms.py are applied to it, so the tolerances of tests/test_norms_gpu.py (calibrated on a kernel that rounds y
and dx once) carry over unchanged.
"""
import numpy as np
import torch

from oracle.naive_norms import naive_layer_norm, naive_layer_norm_grads, naive_rms_norm, naive_rms_norm_grads


def add_h(x, r):
    """h = T(fp32(x) + fp32(residual)) on the CPU, in the dtype of x (torch tensors in, torch tensor out)"""
    x, r = x.detach().cpu(), r.detach().cpu()
    if x.dtype == torch.float64:                 # the helper's own fp64 checks: nothing to round
        return x + r
    return (x.float() + r.float()).to(x.dtype)


def _f64(t):
    return t.detach().to(torch.float64).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def add_rms_norm_ref(x, r, w, *, offset=0.0, eps=1e-6):
    """-> (y, h, rstd) in fp64; x, r torch tensors of one dtype"""
    h = _f64(add_h(x, r))
    y, rstd = naive_rms_norm(h, _f64(w), offset=offset, eps=eps)
    return y, h, rstd


def add_rms_norm_grads_ref(dy, dh, h, w, *, offset=0.0, eps=1e-6):
    """-> (dx, dw) in fp64; dh may be None.  dx is the gradient of x and of residual."""
    dx, dw = naive_rms_norm_grads(_f64(dy), _f64(h), _f64(w), offset=offset, eps=eps)
    return (dx if dh is None else dx + _f64(dh)), dw


def add_layer_norm_ref(x, r, w, b, *, eps=1e-6):
    """-> (y, h, mu, rstd) in fp64"""
    h = _f64(add_h(x, r))
    y, mu, rstd = naive_layer_norm(h, _f64(w), _f64(b), eps=eps)
    return y, h, mu, rstd


def add_layer_norm_grads_ref(dy, dh, h, w, *, eps=1e-6):
    """-> (dx, dw, db) in fp64; dh may be None"""
    dx, dw, db = naive_layer_norm_grads(_f64(dy), _f64(h), _f64(w), eps=eps)
    return (dx if dh is None else dx + _f64(dh)), dw, db
