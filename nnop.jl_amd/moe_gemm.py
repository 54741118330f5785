"""The expert GEMMs of a mixture-of-experts layer over the C ABI of the fifth library (include/nnop_hip_moe_gemm.h; no counterpart in the
reference): one grouped GEMM over the row ranges of `moe_dispatch_plan` (moe.py), between `moe_permute` and `moe_combine` (moe_data.py):

    ys = moe_grouped_gemm(xs, w, offsets)            # xs [S, K], w [E, N, K], offsets [E+1] int32 -> ys [S, N]; differentiable in xs, w
    ys = _moe_grouped_gemm(xs, w, offsets)           # no autograd
    dxs, dw = grad_moe_grouped_gemm(dys, xs, w, offsets, out=None, needs=(True, True))   # a False skips that product: None for it
    moe_grouped_gemm_into(ys, xs, w, offsets)                                             # caller-owned buffers
    grad_moe_grouped_gemm_x_into(dxs, dys, w, offsets);  grad_moe_grouped_gemm_w_into(dw, dys, xs, offsets)

    ys[s] = w[e] xs[s]  for offsets[e] <= s < offsets[e+1]      (fp32 accumulation on the matrix cores, one rounding on the store)

`offsets` is read on the device: nothing is copied to the host, nothing synchronises, and the calls can be captured in a graph.  Rows
outside every expert's range (the rows behind offsets[E] of a plan with skipped entries) come back as +0 and are never read; dw of an
expert without rows is +0.  Every output element is written, so no buffer needs zeroing.  Arrays are float32, float16 or bfloat16, all of
one type; a 2-D row array with unit column stride is taken with its row stride (the padding columns are neither read nor written),
anything else is made contiguous; w is dense [E, N, K], or 3-D with unit column stride, row stride ld_w and expert stride N ld_w.
moe_grouped_gemm saves xs, w and offsets for its pullbacks and runs only the products that are asked for.  GPU-only: no CPU or PyTorch
fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_moe_gemm
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_moe_gemm import MoeGemmDesc, MAX_DIM, MAX_EXPERTS
from .moe import _rows
from .moe_data import _index_array, _out_rows, _row_array, _same

__all__ = ["moe_grouped_gemm", "_moe_grouped_gemm", "grad_moe_grouped_gemm", "moe_grouped_gemm_into", "grad_moe_grouped_gemm_x_into",
           "grad_moe_grouped_gemm_w_into"]


# ---- checks: everything raises before any device work ----------------------------------------------------------------------------------
def _weights(fn, name, w, like):
    """w / dw [E, N, K] of the type of the rows -> (E, N, K)"""
    _row_array(fn, name, w, "[E, N, K]")
    if w.dim() != 3:
        raise NNopError(f"`{name}` must be a tensor of shape (E, N, K), got {tuple(w.shape)}", _lib.NNOP_ERR_SHAPE)
    if w.dtype != like.dtype or w.device != like.device:
        raise NNopError(f"`{name}` must have the element type and device of the row arrays, got {_dtype_name(w.dtype)}")
    return tuple(w.shape)


def _geometry(fn, S, E, K, N):
    if S < 1:
        raise NNopError(f"{fn} needs at least one row", _lib.NNOP_ERR_SHAPE)
    if S > 2 ** 31 - 1:
        raise NNopError("the number of rows must be below 2^31", _lib.NNOP_ERR_SHAPE)
    if not 1 <= E <= MAX_EXPERTS:
        raise NNopError(f"{fn}: the number of experts must be in 1 ... {MAX_EXPERTS}, got {E}", _lib.NNOP_ERR_SHAPE)
    if not (1 <= K <= MAX_DIM and 1 <= N <= MAX_DIM):
        raise NNopError(f"{fn}: K and N must be in 1 ... {MAX_DIM}, got K = {K}, N = {N}", _lib.NNOP_ERR_SHAPE)


def _offsets(fn, offsets, E, like):
    _index_array(fn, "offsets", offsets, "[E + 1]")
    if tuple(offsets.shape) != (E + 1,) or offsets.device != like.device:
        raise NNopError(f"`offsets` must be a tensor of shape ({E + 1},) (E + 1 for the {E} experts of w) on the device of the other "
                        f"arrays, got {tuple(offsets.shape)}", _lib.NNOP_ERR_SHAPE)
    return offsets.contiguous()


def _w_layout(name, w, out=False):
    """w as the library reads it: (tensor, ld_w).  Dense, or unit column stride, row stride ld_w >= K, expert stride N ld_w."""
    E, N, K = w.shape
    ld = w.stride(1) if N > 1 else (w.stride(0) if E > 1 else K)
    ok = (K == 1 or w.stride(2) == 1) and K <= ld < 2 ** 31 and (N == 1 or w.stride(1) == ld) and (E == 1 or w.stride(0) == N * ld)
    if ok:
        return w, ld
    if out:
        raise NNopError(f"`{name}` must be dense, or 3-D with unit column stride, row stride ld_w and expert stride N ld_w")
    return w.contiguous(), K


def _desc(like, S, E, K, N, ld_x, ld_y, ld_w):
    return MoeGemmDesc(dtype=_DTYPES[like.dtype], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=ld_x, ld_y=ld_y, ld_w=ld_w)


def _check(fn, rows_name, rows, cols, w_name, w):
    """the row array that fixes S (xs [S, K] for cols = 2, dys [S, N] for cols = 1) against w -> (S, E, N, K)"""
    _row_array(fn, rows_name, rows, "[S, K]" if cols == 2 else "[S, N]")
    E, N, K = _weights(fn, w_name, w, rows)
    if rows.dim() != 2 or rows.shape[1] != (E, N, K)[cols]:
        raise NNopError(f"`{rows_name}` must be a tensor of shape (S, {(E, N, K)[cols]}) beside {w_name} {tuple(w.shape)}, "
                        f"got {tuple(rows.shape)}", _lib.NNOP_ERR_SHAPE)
    S = rows.shape[0]
    _geometry(fn, S, E, K, N)
    return S, E, N, K


# ---- the three products ------------------------------------------------------------------------------------------------------------------
def moe_grouped_gemm_into(ys, xs, w, offsets):
    """Lowest-level forward: writes ys [S, N] from xs [S, K], w [E, N, K], offsets [E+1] int32.  ys dense, or 2-D with unit column stride."""
    fn = "moe_grouped_gemm"
    S, E, N, K = _check(fn, "xs", xs, 2, "w", w)
    offsets = _offsets(fn, offsets, E, xs)
    _row_array(fn, "ys", ys, "[S, N]")
    _same("ys", ys, (S, N), xs)
    ys, ld_y = _out_rows("ys", ys, N)
    xr, ld_x = _rows(xs, K)
    wr, ld_w = _w_layout("w", w)
    d = _desc(xs, S, E, K, N, ld_x, ld_y, ld_w)
    with _on_device(xs):
        _raise(_lib_moe_gemm.load().nnop_moe_gemm(C.byref(d), _ptr(ys), _ptr(xr), _ptr(wr), _ptr(offsets), _stream(xs)))
    return ys


def _moe_grouped_gemm(xs, w, offsets):
    """ys [S, N] as a new tensor."""
    fn = "moe_grouped_gemm"
    S, E, N, K = _check(fn, "xs", xs, 2, "w", w)
    _offsets(fn, offsets, E, xs)
    with _on_device(xs):
        ys = torch.empty((S, N), dtype=xs.dtype, device=xs.device)
    return moe_grouped_gemm_into(ys, xs, w, offsets)


def grad_moe_grouped_gemm_x_into(dxs, dys, w, offsets):
    """Lowest-level pullback to the rows: writes dxs [S, K] from dys [S, N], w [E, N, K]."""
    fn = "grad_moe_grouped_gemm"
    S, E, N, K = _check(fn, "dys", dys, 1, "w", w)
    offsets = _offsets(fn, offsets, E, dys)
    _row_array(fn, "dxs", dxs, "[S, K]")
    _same("dxs", dxs, (S, K), dys)
    dxs, ld_x = _out_rows("dxs", dxs, K)
    g, ld_y = _rows(dys, N)
    wr, ld_w = _w_layout("w", w)
    d = _desc(dys, S, E, K, N, ld_x, ld_y, ld_w)
    with _on_device(dys):
        _raise(_lib_moe_gemm.load().nnop_moe_gemm_bwd_x(C.byref(d), _ptr(dxs), _ptr(g), _ptr(wr), _ptr(offsets), _stream(dys)))
    return dxs


def grad_moe_grouped_gemm_w_into(dw, dys, xs, offsets):
    """Lowest-level pullback to the weights: writes dw [E, N, K] (dense, or laid out as w may be) from dys [S, N], xs [S, K]."""
    fn = "grad_moe_grouped_gemm"
    S, E, N, K = _check(fn, "dys", dys, 1, "dw", dw)
    offsets = _offsets(fn, offsets, E, dys)
    _row_array(fn, "xs", xs, "[S, K]")
    _same("xs", xs, (S, K), dys)
    dw, ld_w = _w_layout("dw", dw, out=True)
    g, ld_y = _rows(dys, N)
    xr, ld_x = _rows(xs, K)
    d = _desc(dys, S, E, K, N, ld_x, ld_y, ld_w)
    with _on_device(dys):
        _raise(_lib_moe_gemm.load().nnop_moe_gemm_bwd_w(C.byref(d), _ptr(dw), _ptr(g), _ptr(xr), _ptr(offsets), _stream(dys)))
    return dw


def grad_moe_grouped_gemm(dys, xs, w, offsets, out=None, needs=(True, True)):
    """Pullback of `_moe_grouped_gemm`: dys [S, N] -> (dxs [S, K], dw [E, N, K]).  `needs`: a False skips that product and returns None
    for it.  `out`: (dxs, dw) caller-owned, None where not needed; see the two `_into` forms."""
    fn = "grad_moe_grouped_gemm"
    need_x, need_w = bool(needs[0]), bool(needs[1])
    S, E, N, K = _check(fn, "dys", dys, 1, "w", w)
    _offsets(fn, offsets, E, dys)
    _row_array(fn, "xs", xs, "[S, K]")
    _same("xs", xs, (S, K), dys)
    dxs, dw = out if out is not None else (None, None)
    with _on_device(dys):
        if need_x and dxs is None:
            dxs = torch.empty((S, K), dtype=dys.dtype, device=dys.device)
        if need_w and dw is None:
            dw = torch.empty((E, N, K), dtype=dys.dtype, device=dys.device)
    # every check of both products before the first launch
    if need_x:
        _row_array(fn, "dxs", dxs, "[S, K]")
        _same("dxs", dxs, (S, K), dys)
        _out_rows("dxs", dxs, K)
    if need_w:
        if _weights(fn, "dw", dw, dys) != (E, N, K):
            raise NNopError(f"`dw` must be a tensor of shape {(E, N, K)}, got {tuple(dw.shape)}", _lib.NNOP_ERR_SHAPE)
        _w_layout("dw", dw, out=True)
    return (grad_moe_grouped_gemm_x_into(dxs, dys, w, offsets) if need_x else None,
            grad_moe_grouped_gemm_w_into(dw, dys, xs, offsets) if need_w else None)


class _MoeGroupedGemm(torch.autograd.Function):
    """xs and w get the pullbacks' gradients, each only where asked for; offsets carries none.  Saves xs, w, offsets."""

    @staticmethod
    def forward(ctx, xs, w, offsets):
        ys = _moe_grouped_gemm(xs, w, offsets)
        ctx.save_for_backward(xs, w, offsets)
        ctx.set_materialize_grads(False)
        return ys

    @staticmethod
    def backward(ctx, dys):
        if dys is None:
            return None, None, None
        xs, w, offsets = ctx.saved_tensors
        dxs, dw = grad_moe_grouped_gemm(dys, xs, w, offsets, needs=ctx.needs_input_grad[:2])
        return dxs, dw, None


def moe_grouped_gemm(xs, w, offsets):
    """ys [S, N]: row s of xs [S, K] times the weights w[e] [N, K] of the expert whose range offsets[e] ... offsets[e+1]-1 holds s."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    if torch.is_grad_enabled() and (needs(xs) or needs(w)):
        _check("moe_grouped_gemm", "xs", xs, 2, "w", w)
        return _MoeGroupedGemm.apply(xs, w, offsets)
    return _moe_grouped_gemm(xs, w, offsets)
