"""The expert linear layers of a mixture-of-experts layer over the C ABI of the sixth library (include/nnop_hip_moe_linear.h; no
counterpart in the reference): the grouped GEMM of moe_gemm.py as a checkpoint ships its experts -- with a per-expert bias, with the
weights in either order, and with weight and bias gradients that accumulate, in float32 beside 16-bit operands:

    ys = moe_grouped_linear(xs, w, offsets, bias=None, layout="nk")     # differentiable in xs, w, bias
    ys = _moe_grouped_linear(xs, w, offsets, bias=None, layout="nk")    # no autograd
    dxs, dw, db = grad_moe_grouped_linear(dys, xs, w, offsets, layout="nk", needs=(True, True, True), out=None, accumulate=False)
    moe_grouped_linear_into(ys, xs, w, offsets, bias=None, layout="nk")                    # caller-owned buffers
    grad_moe_grouped_linear_x_into(dxs, dys, w, offsets, layout="nk")
    grad_moe_grouped_linear_w_into(dw, dys, xs, offsets, layout="nk", accumulate=False)    # dw.dtype: dys.dtype or float32
    grad_moe_grouped_linear_b_into(db, dys, offsets, accumulate=False)                     # db.dtype likewise

    ys[s] = W_e xs[s] + bias[e]  for offsets[e] <= s < offsets[e+1]     (fp32 accumulation, the bias added in fp32, one rounding)

xs is [S, K], ys [S, N], offsets [E+1] int32, bias [E, N].  layout="nk": w is [E, N, K] (stacked nn.Linear weights, as moe_grouped_gemm
takes them); layout="kn": w is [E, K, N] (input features in the rows, `x @ W`, as Hugging Face stores gate_up_proj and down_proj), read
where it lies: no transposed copy.  dw has the layout of w.  `offsets` is read on the device: nothing is copied to the host, nothing
synchronises, and the calls can be captured in a graph.  Rows outside every expert's range come back as +0 (no bias) and are never
read.  With accumulate=False dw and db of an expert without rows are +0 and every output element is written; with accumulate=True the
sums are added to what dw / db hold (new = round(float(old) + fp32 sum)) and an expert without rows keeps its bits.  Arrays are float32,
float16 or bfloat16, all of one type, except that dw and db may be float32 beside 16-bit operands (a float32 main gradient).  A 2-D array
with unit column stride is taken with its row stride, w as moe_gemm._w_layout takes it; anything else is made contiguous (outputs must
have such a layout).  moe_grouped_linear saves xs, w and offsets for its pullbacks, never the bias, and runs only the products that are
asked for; its gradients have the type of their inputs.  GPU-only: no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_moe_linear
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_moe_linear import ACCUMULATE, KN, MoeLinearDesc
from .moe import _rows
from .moe_data import _out_rows, _row_array, _same
from .moe_gemm import _geometry, _offsets, _w_layout

__all__ = ["moe_grouped_linear", "_moe_grouped_linear", "grad_moe_grouped_linear", "moe_grouped_linear_into",
           "grad_moe_grouped_linear_x_into", "grad_moe_grouped_linear_w_into", "grad_moe_grouped_linear_b_into"]


# ---- checks: everything raises before any device work ----------------------------------------------------------------------------------
def _kn(layout):
    if layout not in ("nk", "kn"):
        raise NNopError(f"`layout` must be \"nk\" (w [E, N, K]) or \"kn\" (w [E, K, N]), got {layout!r}", _lib.NNOP_ERR_OPTS)
    return layout == "kn"


def _grad_type(name, t, like):
    """a gradient array has the type of the operands, or is float32"""
    if t.dtype != like.dtype and t.dtype != torch.float32:
        raise NNopError(f"`{name}` must be {_dtype_name(like.dtype)} like the row arrays, or float32, got {_dtype_name(t.dtype)}")
    if t.device != like.device:
        raise NNopError(f"`{name}` must be on the device of the row arrays")


def _weights(fn, name, w, like, kn, grad=False):
    """w / dw of the layout's shape -> (E, N, K); the type of the rows (a gradient: or float32)"""
    what = "[E, K, N]" if kn else "[E, N, K]"
    _row_array(fn, name, w, what)
    if w.dim() != 3:
        raise NNopError(f"`{name}` must be a tensor of shape {what}, got {tuple(w.shape)}", _lib.NNOP_ERR_SHAPE)
    if grad:
        _grad_type(name, w, like)
    elif w.dtype != like.dtype or w.device != like.device:
        raise NNopError(f"`{name}` must have the element type and device of the row arrays, got {_dtype_name(w.dtype)}")
    E, a, b = w.shape
    return (E, b, a) if kn else (E, a, b)


def _bias(fn, name, b, E, N, like, grad=False):
    _row_array(fn, name, b, "[E, N]")
    if tuple(b.shape) != (E, N):
        raise NNopError(f"`{name}` must be a tensor of shape ({E}, {N}), got {tuple(b.shape)}", _lib.NNOP_ERR_SHAPE)
    if grad:
        _grad_type(name, b, like)
    elif b.dtype != like.dtype or b.device != like.device:
        raise NNopError(f"`{name}` must have the element type and device of the row arrays, got {_dtype_name(b.dtype)}")


def _check(fn, rows_name, rows, cols, w_name, w, kn, grad=False):
    """the row array that fixes S (xs [S, K] for cols = 2, dys [S, N] for cols = 1) against w -> (S, E, N, K)"""
    _row_array(fn, rows_name, rows, "[S, K]" if cols == 2 else "[S, N]")
    E, N, K = _weights(fn, w_name, w, rows, kn, grad)
    if rows.dim() != 2 or rows.shape[1] != (E, N, K)[cols]:
        raise NNopError(f"`{rows_name}` must be a tensor of shape (S, {(E, N, K)[cols]}) beside {w_name} {tuple(w.shape)}, "
                        f"got {tuple(rows.shape)}", _lib.NNOP_ERR_SHAPE)
    S = rows.shape[0]
    _geometry(fn, S, E, K, N)
    return S, E, N, K


def _desc(like, S, E, K, N, kn, ld_x=None, ld_y=None, ld_w=None, ld_dw=None, ld_b=None, ld_db=None, grad=None, accumulate=False):
    """a stride a call does not use is the dense one, which passes the library's check of every field"""
    wcols = N if kn else K
    return MoeLinearDesc(dtype=_DTYPES[like.dtype], grad_dtype=_DTYPES[like.dtype if grad is None else grad.dtype], rows=S, experts=E,
                         in_dim=K, out_dim=N, ld_x=ld_x or K, ld_y=ld_y or N, ld_w=ld_w or wcols, ld_dw=ld_dw or wcols, ld_b=ld_b or N,
                         ld_db=ld_db or N, flags=(KN if kn else 0) | (ACCUMULATE if accumulate else 0))


# ---- the four calls ----------------------------------------------------------------------------------------------------------------------
def moe_grouped_linear_into(ys, xs, w, offsets, bias=None, layout="nk"):
    """Lowest-level forward: writes ys [S, N] from xs [S, K], w, offsets [E+1] int32 and bias [E, N] or None.  ys dense, or 2-D with unit
    column stride."""
    fn = "moe_grouped_linear"
    kn = _kn(layout)
    S, E, N, K = _check(fn, "xs", xs, 2, "w", w, kn)
    offsets = _offsets(fn, offsets, E, xs)
    if bias is not None:
        _bias(fn, "bias", bias, E, N, xs)
    _row_array(fn, "ys", ys, "[S, N]")
    _same("ys", ys, (S, N), xs)
    ys, ld_y = _out_rows("ys", ys, N)
    xr, ld_x = _rows(xs, K)
    wr, ld_w = _w_layout("w", w)
    br, ld_b = _rows(bias, N) if bias is not None else (None, N)
    d = _desc(xs, S, E, K, N, kn, ld_x=ld_x, ld_y=ld_y, ld_w=ld_w, ld_b=ld_b)
    with _on_device(xs):
        _raise(_lib_moe_linear.load().nnop_moe_linear(C.byref(d), _ptr(ys), _ptr(xr), _ptr(wr), _ptr(br), _ptr(offsets), _stream(xs)))
    return ys


def _moe_grouped_linear(xs, w, offsets, bias=None, layout="nk"):
    """ys [S, N] as a new tensor."""
    fn = "moe_grouped_linear"
    kn = _kn(layout)
    S, E, N, K = _check(fn, "xs", xs, 2, "w", w, kn)
    _offsets(fn, offsets, E, xs)
    if bias is not None:
        _bias(fn, "bias", bias, E, N, xs)
    with _on_device(xs):
        ys = torch.empty((S, N), dtype=xs.dtype, device=xs.device)
    return moe_grouped_linear_into(ys, xs, w, offsets, bias, layout)


def grad_moe_grouped_linear_x_into(dxs, dys, w, offsets, layout="nk"):
    """Lowest-level pullback to the rows: writes dxs [S, K] from dys [S, N] and w."""
    fn = "grad_moe_grouped_linear"
    kn = _kn(layout)
    S, E, N, K = _check(fn, "dys", dys, 1, "w", w, kn)
    offsets = _offsets(fn, offsets, E, dys)
    _row_array(fn, "dxs", dxs, "[S, K]")
    _same("dxs", dxs, (S, K), dys)
    dxs, ld_x = _out_rows("dxs", dxs, K)
    g, ld_y = _rows(dys, N)
    wr, ld_w = _w_layout("w", w)
    d = _desc(dys, S, E, K, N, kn, ld_x=ld_x, ld_y=ld_y, ld_w=ld_w)
    with _on_device(dys):
        _raise(_lib_moe_linear.load().nnop_moe_linear_bwd_x(C.byref(d), _ptr(dxs), _ptr(g), _ptr(wr), _ptr(offsets), _stream(dys)))
    return dxs


def grad_moe_grouped_linear_w_into(dw, dys, xs, offsets, layout="nk", accumulate=False):
    """Lowest-level pullback to the weights: writes dw (the layout of w: dense, or laid out as w may be; the type of dys or float32) from
    dys [S, N], xs [S, K], or adds to it."""
    fn = "grad_moe_grouped_linear"
    kn = _kn(layout)
    S, E, N, K = _check(fn, "dys", dys, 1, "dw", dw, kn, grad=True)
    offsets = _offsets(fn, offsets, E, dys)
    _row_array(fn, "xs", xs, "[S, K]")
    _same("xs", xs, (S, K), dys)
    dw, ld_dw = _w_layout("dw", dw, out=True)
    g, ld_y = _rows(dys, N)
    xr, ld_x = _rows(xs, K)
    d = _desc(dys, S, E, K, N, kn, ld_x=ld_x, ld_y=ld_y, ld_dw=ld_dw, grad=dw, accumulate=accumulate)
    with _on_device(dys):
        _raise(_lib_moe_linear.load().nnop_moe_linear_bwd_w(C.byref(d), _ptr(dw), _ptr(g), _ptr(xr), _ptr(offsets), _stream(dys)))
    return dw


def grad_moe_grouped_linear_b_into(db, dys, offsets, accumulate=False):
    """Lowest-level pullback to the bias: writes db [E, N] (dense, or 2-D with unit column stride; the type of dys or float32) from
    dys [S, N], or adds to it."""
    fn = "grad_moe_grouped_linear"
    _row_array(fn, "dys", dys, "[S, N]")
    _row_array(fn, "db", db, "[E, N]")
    if dys.dim() != 2 or db.dim() != 2 or db.shape[1] != dys.shape[1]:
        raise NNopError(f"`dys` must be a tensor of shape (S, N) and `db` one of shape (E, N), got {tuple(dys.shape)} and "
                        f"{tuple(db.shape)}", _lib.NNOP_ERR_SHAPE)
    (S, N), E = dys.shape, db.shape[0]
    _geometry(fn, S, E, 1, N)
    _bias(fn, "db", db, E, N, dys, grad=True)
    offsets = _offsets(fn, offsets, E, dys)
    db, ld_db = _out_rows("db", db, N)
    g, ld_y = _rows(dys, N)
    d = _desc(dys, S, E, 1, N, False, ld_y=ld_y, ld_db=ld_db, grad=db, accumulate=accumulate)
    with _on_device(dys):
        _raise(_lib_moe_linear.load().nnop_moe_linear_bwd_b(C.byref(d), _ptr(db), _ptr(g), _ptr(offsets), _stream(dys)))
    return db


def grad_moe_grouped_linear(dys, xs, w, offsets, layout="nk", needs=(True, True, True), out=None, accumulate=False):
    """Pullback of `_moe_grouped_linear`: dys [S, N] -> (dxs [S, K], dw like w, db [E, N]).  `needs`: a False skips that product and
    returns None for it.  `out`: (dxs, dw, db) caller-owned, None where not needed; dw and db may be float32 beside 16-bit operands.
    `accumulate`: dw and db are added to (they must then be given in `out`); dxs is always stored."""
    fn = "grad_moe_grouped_linear"
    kn = _kn(layout)
    need_x, need_w, need_b = (bool(n) for n in needs)
    S, E, N, K = _check(fn, "dys", dys, 1, "w", w, kn)
    _offsets(fn, offsets, E, dys)
    _row_array(fn, "xs", xs, "[S, K]")
    _same("xs", xs, (S, K), dys)
    dxs, dw, db = out if out is not None else (None, None, None)
    if accumulate and ((need_w and dw is None) or (need_b and db is None)):
        raise NNopError("`accumulate` must come with the dw and db to add to, in `out`")
    with _on_device(dys):
        if need_x and dxs is None:
            dxs = torch.empty((S, K), dtype=dys.dtype, device=dys.device)
        if need_w and dw is None:
            dw = torch.empty((E, K, N) if kn else (E, N, K), dtype=dys.dtype, device=dys.device)
        if need_b and db is None:
            db = torch.empty((E, N), dtype=dys.dtype, device=dys.device)
    # every check of the three products before the first launch
    if need_x:
        _row_array(fn, "dxs", dxs, "[S, K]")
        _same("dxs", dxs, (S, K), dys)
        _out_rows("dxs", dxs, K)
    if need_w:
        if _weights(fn, "dw", dw, dys, kn, grad=True) != (E, N, K):
            raise NNopError(f"`dw` must be a tensor of shape {tuple(w.shape)}, got {tuple(dw.shape)}", _lib.NNOP_ERR_SHAPE)
        _w_layout("dw", dw, out=True)
    if need_b:
        _bias(fn, "db", db, E, N, dys, grad=True)
        _out_rows("db", db, N)
    return (grad_moe_grouped_linear_x_into(dxs, dys, w, offsets, layout) if need_x else None,
            grad_moe_grouped_linear_w_into(dw, dys, xs, offsets, layout, accumulate) if need_w else None,
            grad_moe_grouped_linear_b_into(db, dys, offsets, accumulate) if need_b else None)


class _MoeGroupedLinear(torch.autograd.Function):
    """xs, w and bias get the pullbacks' gradients, each only where asked for; offsets carries none.  Saves xs, w, offsets: the bias
    gradient needs neither the bias nor the output."""

    @staticmethod
    def forward(ctx, xs, w, offsets, bias, layout):
        ys = _moe_grouped_linear(xs, w, offsets, bias, layout)
        ctx.save_for_backward(xs, w, offsets)
        ctx.layout = layout
        ctx.set_materialize_grads(False)
        return ys

    @staticmethod
    def backward(ctx, dys):
        if dys is None:
            return None, None, None, None, None
        xs, w, offsets = ctx.saved_tensors
        need = ctx.needs_input_grad
        dxs, dw, db = grad_moe_grouped_linear(dys, xs, w, offsets, ctx.layout, needs=(need[0], need[1], need[3]))
        return dxs, dw, None, db, None


def moe_grouped_linear(xs, w, offsets, bias=None, layout="nk"):
    """ys [S, N]: row s of xs [S, K] through the linear layer (w[e], bias[e]) of the expert whose range offsets[e] ... offsets[e+1]-1
    holds s."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    if torch.is_grad_enabled() and (needs(xs) or needs(w) or needs(bias)):
        S, E, N, K = _check("moe_grouped_linear", "xs", xs, 2, "w", w, _kn(layout))
        if bias is not None:
            _bias("moe_grouped_linear", "bias", bias, E, N, xs)
        return _MoeGroupedLinear.apply(xs, w, offsets, bias, layout)
    return _moe_grouped_linear(xs, w, offsets, bias, layout)
