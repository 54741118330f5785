"""The expert linear layers of a mixture-of-experts layer on MXFP4 weights, over the C ABI of the seventh library
(include/nnop_hip_moe_mx.h; no counterpart in the reference): moe_linear.py's forward and pullback to the rows, reading the packed
blocks and scale bytes a gpt-oss checkpoint ships (gate_up_proj_blocks / _scales, down_proj_blocks / _scales) where they lie, and the
two conversions between that form and plain weights:

    blocks, scales = mxfp4_quantize(w)                                   # w [..., K] -> uint8 [..., K/32, 16], uint8 [..., K/32]
    w = mxfp4_dequantize(blocks, scales, dtype=torch.bfloat16)           # -> [..., K]
    ys = moe_grouped_linear_mxfp4(xs, blocks, scales, offsets, bias=None)            # differentiable in xs and bias
    ys = _moe_grouped_linear_mxfp4(xs, blocks, scales, offsets, bias=None)           # no autograd
    moe_grouped_linear_mxfp4_into(ys, xs, blocks, scales, offsets, bias=None)        # caller-owned buffers
    grad_moe_grouped_linear_mxfp4_x_into(dxs, dys, blocks, scales, offsets)

    ys[s] = W_e xs[s] + bias[e]  for offsets[e] <= s < offsets[e+1],   W_e = mxfp4_dequantize(blocks[e], scales[e], xs.dtype)

The format: 32 values along the last axis share one scale byte e (2^(e - 127); 255: NaN) and are 4-bit E2M1 codes (sign, then the
magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6), two to a byte, the even element in the low nibble -- as Hugging Face's gpt-oss conversion lays them
out.  xs is [S, K], ys [S, N], offsets [E+1] int32, bias [E, N]; scales is [E, N, K/32] and blocks [E, N, K/32, 16] or [E, N, K/2].
The rows and the bias are float16 or bfloat16.  The result equals moe_grouped_linear(xs, mxfp4_dequantize(blocks, scales, xs.dtype),
offsets, bias) bit for bit: the weights are expanded in the registers that stage them for the matrix cores, everything else is that
operator's code.  Packed weights are frozen: they get no gradient; the bias gradient is moe_linear's.  `blocks` and `scales` must be
uint8, contiguous and on the device of the rows -- a weight of many gigabytes is never copied silently.  Row arrays follow
moe_linear.py: a 2-D array with unit column stride is taken with its row stride.  `offsets` is read on the device: nothing is copied to
the host, nothing synchronises, and the calls can be captured in a graph.  GPU-only: no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_moe_mx
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_moe_mx import BLOCK, MAX_COLS, MAX_PIECES, MoeMxDesc, Mxfp4Desc
from .moe import _rows
from .moe_data import _out_rows, _row_array, _same, _tensor
from .moe_gemm import _geometry, _offsets
from .moe_linear import _bias, grad_moe_grouped_linear_b_into

__all__ = ["mxfp4_quantize", "mxfp4_dequantize", "moe_grouped_linear_mxfp4", "_moe_grouped_linear_mxfp4",
           "moe_grouped_linear_mxfp4_into", "grad_moe_grouped_linear_mxfp4_x_into"]


# ---- checks: everything raises before any device work ----------------------------------------------------------------------------------
def _packed(fn, blocks, scales, device=None):
    """blocks [..., K/32, 16] or [..., K/2] beside scales [..., K/32], as they lie -> (the leading shape, K)"""
    _tensor(fn, "blocks", blocks, "[..., K/32, 16]")
    _tensor(fn, "scales", scales, "[..., K/32]")
    for name, t in (("blocks", blocks), ("scales", scales)):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise NNopError(f"`{name}` must be a contiguous uint8 tensor (packed weights are read where they lie, never copied), got "
                            f"{_dtype_name(t.dtype)} with strides {tuple(t.stride())}")
        if t.device != (blocks.device if device is None else device):
            raise NNopError(f"`{name}` must be on the device of the other arrays")
    lead, nb = tuple(scales.shape[:-1]), scales.shape[-1]
    if nb < 1 or tuple(blocks.shape) not in (lead + (nb, BLOCK // 2), lead + (nb * (BLOCK // 2),)):
        raise NNopError(f"`blocks` must be a tensor of shape {lead + (nb, BLOCK // 2)} or {lead + (nb * (BLOCK // 2),)} beside scales "
                        f"{tuple(scales.shape)}, got {tuple(blocks.shape)}", _lib.NNOP_ERR_SHAPE)
    return lead, nb * BLOCK


def _conversion_geometry(fn, rows, K):
    if rows < 1 or not BLOCK <= K <= MAX_COLS or rows * (K // 8) > MAX_PIECES:
        raise NNopError(f"{fn}: needs at least one row of K = 32 ... {MAX_COLS} values and at most {MAX_PIECES} rows K / 8, got "
                        f"{rows} rows of {K}", _lib.NNOP_ERR_SHAPE)


def _check(fn, rows_name, rows, cols, blocks, scales):
    """the row array that fixes S (xs [S, K] for cols = 2, dys [S, N] for cols = 1) against the packed weights -> (S, E, N, K)"""
    _row_array(fn, rows_name, rows, "[S, K]" if cols == 2 else "[S, N]")
    if rows.dtype == torch.float32:
        raise NNopError(f"`{rows_name}` must be float16 or bfloat16 beside MXFP4 weights, got float32", _lib.NNOP_ERR_DTYPE)
    lead, K = _packed(fn, blocks, scales, rows.device)
    if len(lead) != 2:
        raise NNopError(f"`scales` must be a tensor of shape [E, N, K/32], got {tuple(scales.shape)}", _lib.NNOP_ERR_SHAPE)
    E, N = lead
    if rows.dim() != 2 or rows.shape[1] != (E, N, K)[cols]:
        raise NNopError(f"`{rows_name}` must be a tensor of shape (S, {(E, N, K)[cols]}) beside scales {tuple(scales.shape)}, "
                        f"got {tuple(rows.shape)}", _lib.NNOP_ERR_SHAPE)
    S = rows.shape[0]
    _geometry(fn, S, E, K, N)
    return S, E, N, K


def _desc(like, S, E, K, N, ld_x=None, ld_y=None, ld_b=None):
    """a stride a call does not use is the dense one, which passes the library's check of every field"""
    return MoeMxDesc(dtype=_DTYPES[like.dtype], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=ld_x or K, ld_y=ld_y or N, ld_b=ld_b or N,
                     ld_q=K // 2, ld_s=K // BLOCK, flags=0)


# ---- the conversions ---------------------------------------------------------------------------------------------------------------------
def mxfp4_quantize(w):
    """(blocks uint8 [..., K/32, 16], scales uint8 [..., K/32]) of w [..., K], float32, float16 or bfloat16, K a multiple of 32: per block
    the scale 2^(floor(log2(amax)) - 2), the nearest E2M1 magnitude with ties to the even code, saturation at 6; a block with an Inf or a
    NaN gets the scale byte 255."""
    fn = "mxfp4_quantize"
    _row_array(fn, "w", w, "[..., K]")
    K = w.shape[-1]
    if K < BLOCK or K % BLOCK != 0:
        raise NNopError(f"{fn}: the last axis must be a multiple of {BLOCK}, got {K}", _lib.NNOP_ERR_SHAPE)
    lead, rows = tuple(w.shape[:-1]), w.numel() // K
    _conversion_geometry(fn, rows, K)
    wr, ld = _rows(w, K) if w.dim() == 2 else (w.contiguous(), K)
    with _on_device(w):
        blocks = torch.empty(lead + (K // BLOCK, BLOCK // 2), dtype=torch.uint8, device=w.device)
        scales = torch.empty(lead + (K // BLOCK,), dtype=torch.uint8, device=w.device)
        d = Mxfp4Desc(dtype=_DTYPES[w.dtype], rows=rows, cols=K, ld=ld, ld_q=K // 2, ld_s=K // BLOCK)
        _raise(_lib_moe_mx.load().nnop_mxfp4_quant(C.byref(d), _ptr(blocks), _ptr(scales), _ptr(wr), _stream(w)))
    return blocks, scales


def mxfp4_dequantize(blocks, scales, dtype=torch.bfloat16):
    """w [..., K] of `dtype` (float32, float16 or bfloat16): magnitude(code) 2^(scale - 127) rounded to nearest even; the conversion the
    grouped linear applies to its weights."""
    fn = "mxfp4_dequantize"
    lead, K = _packed(fn, blocks, scales)
    if dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {dtype} of the result; expected float32, float16 or bfloat16")
    rows = scales.numel() // (K // BLOCK)
    _conversion_geometry(fn, rows, K)
    with _on_device(blocks):
        w = torch.empty(lead + (K,), dtype=dtype, device=blocks.device)
        d = Mxfp4Desc(dtype=_DTYPES[dtype], rows=rows, cols=K, ld=K, ld_q=K // 2, ld_s=K // BLOCK)
        _raise(_lib_moe_mx.load().nnop_mxfp4_dequant(C.byref(d), _ptr(w), _ptr(blocks), _ptr(scales), _stream(blocks)))
    return w


# ---- the two products ---------------------------------------------------------------------------------------------------------------------
def moe_grouped_linear_mxfp4_into(ys, xs, blocks, scales, offsets, bias=None):
    """Lowest-level forward: writes ys [S, N] from xs [S, K], the packed weights, offsets [E+1] int32 and bias [E, N] or None.  ys dense,
    or 2-D with unit column stride."""
    fn = "moe_grouped_linear_mxfp4"
    S, E, N, K = _check(fn, "xs", xs, 2, blocks, scales)
    offsets = _offsets(fn, offsets, E, xs)
    if bias is not None:
        _bias(fn, "bias", bias, E, N, xs)
    _row_array(fn, "ys", ys, "[S, N]")
    _same("ys", ys, (S, N), xs)
    ys, ld_y = _out_rows("ys", ys, N)
    xr, ld_x = _rows(xs, K)
    br, ld_b = _rows(bias, N) if bias is not None else (None, N)
    d = _desc(xs, S, E, K, N, ld_x=ld_x, ld_y=ld_y, ld_b=ld_b)
    with _on_device(xs):
        _raise(_lib_moe_mx.load().nnop_moe_mx_linear(C.byref(d), _ptr(ys), _ptr(xr), _ptr(blocks), _ptr(scales), _ptr(br), _ptr(offsets),
                                                     _stream(xs)))
    return ys


def _moe_grouped_linear_mxfp4(xs, blocks, scales, offsets, bias=None):
    """ys [S, N] as a new tensor."""
    fn = "moe_grouped_linear_mxfp4"
    S, E, N, K = _check(fn, "xs", xs, 2, blocks, scales)
    _offsets(fn, offsets, E, xs)
    if bias is not None:
        _bias(fn, "bias", bias, E, N, xs)
    with _on_device(xs):
        ys = torch.empty((S, N), dtype=xs.dtype, device=xs.device)
    return moe_grouped_linear_mxfp4_into(ys, xs, blocks, scales, offsets, bias)


def grad_moe_grouped_linear_mxfp4_x_into(dxs, dys, blocks, scales, offsets):
    """Lowest-level pullback to the rows: writes dxs [S, K] from dys [S, N] and the packed weights."""
    fn = "grad_moe_grouped_linear_mxfp4"
    S, E, N, K = _check(fn, "dys", dys, 1, blocks, scales)
    offsets = _offsets(fn, offsets, E, dys)
    _row_array(fn, "dxs", dxs, "[S, K]")
    _same("dxs", dxs, (S, K), dys)
    dxs, ld_x = _out_rows("dxs", dxs, K)
    g, ld_y = _rows(dys, N)
    d = _desc(dys, S, E, K, N, ld_x=ld_x, ld_y=ld_y)
    with _on_device(dys):
        _raise(_lib_moe_mx.load().nnop_moe_mx_linear_bwd_x(C.byref(d), _ptr(dxs), _ptr(g), _ptr(blocks), _ptr(scales), _ptr(offsets),
                                                           _stream(dys)))
    return dxs


class _MoeGroupedLinearMxfp4(torch.autograd.Function):
    """xs and bias get gradients, each only where asked for: dxs from the seventh library, db from the sixth's bias gradient.  The packed
    weights and offsets carry none.  Saves blocks, scales, offsets: neither pullback needs xs, the bias or the output."""

    @staticmethod
    def forward(ctx, xs, blocks, scales, offsets, bias):
        ys = _moe_grouped_linear_mxfp4(xs, blocks, scales, offsets, bias)
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


def moe_grouped_linear_mxfp4(xs, blocks, scales, offsets, bias=None):
    """ys [S, N]: row s of xs [S, K] through the linear layer (the MXFP4 weights of expert e, bias[e]) of the expert whose range
    offsets[e] ... offsets[e+1]-1 holds s."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    if torch.is_grad_enabled() and (needs(xs) or needs(bias)):
        S, E, N, K = _check("moe_grouped_linear_mxfp4", "xs", xs, 2, blocks, scales)
        if bias is not None:
            _bias("moe_grouped_linear_mxfp4", "bias", bias, E, N, xs)
        return _MoeGroupedLinearMxfp4.apply(xs, blocks, scales, offsets, bias)
    return _moe_grouped_linear_mxfp4(xs, blocks, scales, offsets, bias)
