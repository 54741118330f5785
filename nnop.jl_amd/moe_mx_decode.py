"""The expert linear layer on MXFP4 weights for decode-sized batches, over the C ABI of the eighth library
(include/nnop_hip_moe_mx_decode.h; no counterpart in the reference): moe_mx.py's forward with a kernel made for few rows per expert.

    ys = moe_decode_linear_mxfp4(xs, blocks, scales, offsets, bias=None)             # differentiable in xs and bias
    ys = _moe_decode_linear_mxfp4(xs, blocks, scales, offsets, bias=None)            # no autograd
    moe_decode_linear_mxfp4_into(ys, xs, blocks, scales, offsets, bias=None)         # caller-owned buffers

    ys[s] = W_e xs[s] + bias[e]  for offsets[e] <= s < offsets[e+1],   W_e = mxfp4_dequantize(blocks[e], scales[e], xs.dtype)

Arguments, formats and checks are those of moe_grouped_linear_mxfp4 (moe_mx.py), whose helpers this module calls: xs [S, K], ys [S, N],
offsets [E+1] int32, bias [E, N], scales [E, N, K/32], blocks [E, N, K/32, 16] or [E, N, K/2]; rows and bias float16 or bfloat16;
`blocks` and `scales` uint8, contiguous, on the device of the rows, never copied.  What differs is the kernel.  moe_grouped_linear_mxfp4
runs the 128 x 128 tile, which waits for one trip to memory per reduction step however few rows an expert has; this call streams the
packed weights once, straight into the registers that feed the matrix cores, with many loads in flight.  Its contracts:

  - fp32 sums on the matrix cores, the bias added in fp32, one rounding; no atomics, no workspace, no sync, graph-capturable; two runs
    are bitwise equal; rows outside every expert are +0; nothing is touched out of bounds whatever `offsets` holds.
  - Batch invariance: the order in which the terms of an output element are added depends on K and the dtype alone, so a row's bits do
    not depend on the plan, on the row's place in it or on the other rows.
  - That order is not the tile's: the result is not promised bit-equal to moe_grouped_linear_mxfp4 (on data whose sums are exact the
    two agree exactly).
  - Correct for any plan, fast where experts hold few rows: up to 32 rows of an expert cost one pass over its weights, every further 32
    another.  Measured on an MI355X (bf16, E = 128, 2880 -> 5760 and 2880 -> 2880): 1.8 - 2.0 x faster than
    moe_grouped_linear_mxfp4 at S = 256 and 1024 slot rows, 1.6 x at S = 2048, level at S = 4096 (a mean of 32 rows per expert), where
    the tile path overtakes, and 1.6 x slower at S = 8192.  Call this one up to a mean of about 24 rows per expert (S / E), the
    tile beyond.

There is no decode pullback: the gradients are those of moe_grouped_linear_mxfp4 (grad_moe_grouped_linear_mxfp4_x_into of the seventh
library, grad_moe_grouped_linear_b_into of the sixth), and this operator never dispatches to or from that one.  GPU-only: no CPU or
PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib_moe_mx_decode
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream  # noqa: F401  (the shared plumbing)
from ._lib_moe_mx import BLOCK
from ._lib_moe_mx_decode import MoeMxDecodeDesc
from .moe import _rows
from .moe_data import _out_rows, _row_array, _same
from .moe_gemm import _offsets
from .moe_linear import _bias, grad_moe_grouped_linear_b_into
from .moe_mx import _check, grad_moe_grouped_linear_mxfp4_x_into

__all__ = ["moe_decode_linear_mxfp4", "_moe_decode_linear_mxfp4", "moe_decode_linear_mxfp4_into"]

FN = "moe_decode_linear_mxfp4"


def _desc(like, S, E, K, N, ld_x=None, ld_y=None, ld_b=None):
    """moe_mx._desc for the eighth library's descriptor: the packed strides are the dense ones"""
    return MoeMxDecodeDesc(dtype=_DTYPES[like.dtype], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=ld_x or K, ld_y=ld_y or N, ld_b=ld_b or N,
                           ld_q=K // 2, ld_s=K // BLOCK, flags=0)


def moe_decode_linear_mxfp4_into(ys, xs, blocks, scales, offsets, bias=None):
    """Lowest-level forward: writes ys [S, N] from xs [S, K], the packed weights, offsets [E+1] int32 and bias [E, N] or None.  ys dense,
    or 2-D with unit column stride."""
    S, E, N, K = _check(FN, "xs", xs, 2, blocks, scales)
    offsets = _offsets(FN, offsets, E, xs)
    if bias is not None:
        _bias(FN, "bias", bias, E, N, xs)
    _row_array(FN, "ys", ys, "[S, N]")
    _same("ys", ys, (S, N), xs)
    ys, ld_y = _out_rows("ys", ys, N)
    xr, ld_x = _rows(xs, K)
    br, ld_b = _rows(bias, N) if bias is not None else (None, N)
    d = _desc(xs, S, E, K, N, ld_x=ld_x, ld_y=ld_y, ld_b=ld_b)
    with _on_device(xs):
        _raise(_lib_moe_mx_decode.load().nnop_moe_mx_decode_linear(C.byref(d), _ptr(ys), _ptr(xr), _ptr(blocks), _ptr(scales), _ptr(br),
                                                                   _ptr(offsets), _stream(xs)))
    return ys


def _moe_decode_linear_mxfp4(xs, blocks, scales, offsets, bias=None):
    """ys [S, N] as a new tensor."""
    S, E, N, K = _check(FN, "xs", xs, 2, blocks, scales)
    _offsets(FN, offsets, E, xs)
    if bias is not None:
        _bias(FN, "bias", bias, E, N, xs)
    with _on_device(xs):
        ys = torch.empty((S, N), dtype=xs.dtype, device=xs.device)
    return moe_decode_linear_mxfp4_into(ys, xs, blocks, scales, offsets, bias)


class _MoeDecodeLinearMxfp4(torch.autograd.Function):
    """The decode forward with the pullbacks of moe_grouped_linear_mxfp4: dxs from the seventh library, db from the sixth's bias gradient,
    each only where asked for.  Saves blocks, scales, offsets."""

    @staticmethod
    def forward(ctx, xs, blocks, scales, offsets, bias):
        ys = _moe_decode_linear_mxfp4(xs, blocks, scales, offsets, bias)
        ctx.save_for_backward(blocks, scales, offsets)
        ctx.set_materialize_grads(False)
        return ys

    @staticmethod
    def backward(ctx, dys):
        if dys is None:
            return None, None, None, None, None
        blocks, scales, offsets = ctx.saved_tensors
        need = ctx.needs_input_grad
        (E, N), K = scales.shape[:2], scales.shape[2] * BLOCK
        dxs = db = None
        with _on_device(dys):
            if need[0]:
                dxs = torch.empty((dys.shape[0], K), dtype=dys.dtype, device=dys.device)
            if need[4]:
                db = torch.empty((E, N), dtype=dys.dtype, device=dys.device)
        if need[0]:
            grad_moe_grouped_linear_mxfp4_x_into(dxs, dys, blocks, scales, offsets)
        if need[4]:
            grad_moe_grouped_linear_b_into(db, dys, offsets)
        return dxs, None, None, None, db


def moe_decode_linear_mxfp4(xs, blocks, scales, offsets, bias=None):
    """ys [S, N]: row s of xs [S, K] through the linear layer (the MXFP4 weights of expert e, bias[e]) of the expert whose range
    offsets[e] ... offsets[e+1]-1 holds s, by the weight-streaming kernel."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    if torch.is_grad_enabled() and (needs(xs) or needs(bias)):
        S, E, N, K = _check(FN, "xs", xs, 2, blocks, scales)
        if bias is not None:
            _bias(FN, "bias", bias, E, N, xs)
        return _MoeDecodeLinearMxfp4.apply(xs, blocks, scales, offsets, bias)
    return _moe_decode_linear_mxfp4(xs, blocks, scales, offsets, bias)
