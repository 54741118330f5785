"""The data movement of a mixture-of-experts layer over the C ABI of the fourth library (include/nnop_hip_moe_data.h; no counterpart in
the reference): the token permute in front of the expert GEMMs and the weighted combine behind them, each with its pullback.  They consume
the plan of `moe_dispatch_plan` (moe.py):

    xs = moe_permute(x, perm, slot)                 # x [..., D], slot [..., k] -> xs [T k, D], expert-sorted; differentiable in x
    y = moe_combine(ys, w, perm, slot)              # ys [T k, D], w [..., k] float32 -> y [..., D]; differentiable in ys and w
    xs = _moe_permute(x, perm, slot);  y = _moe_combine(ys, w, perm, slot)                        # no autograd
    dx = grad_moe_permute(dxs, slot, out=None)
    dys, dw = grad_moe_combine(dy, ys, w, perm, slot, out=None)                                   # out: (dys, dw)
    moe_permute_into(xs, x, perm);  grad_moe_permute_into(dx, dxs, slot)                          # caller-owned buffers
    moe_combine_into(y, ys, w, slot);  grad_moe_combine_into(dys, dw, dy, ys, w, perm, slot)

    xs[s] = x[perm[s] // k]        y[t] = sum_j w[t, j] ys[slot[t, j]]        (fp32 sums in ascending j, one rounding on the store)

An entry of perm / slot outside [0, T k) -- the -1 the plan writes for an assignment it skipped -- is skipped here too: its row of xs /
dys is +0, it adds nothing to y / dx, its dw is +0.  Every output element is written, so no buffer needs zeroing.  Row arrays are float32,
float16 or bfloat16; a 2-D row array with unit column stride is taken with its row stride (the padding columns are neither read nor
written), anything else is made contiguous.  w and dw are float32, as the gate returns them: the caller decides when to round.
moe_combine saves ys, w, perm, slot for its pullback, nothing of size [T, k, D]; moe_permute saves slot.  GPU-only: no CPU or PyTorch
fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_moe_data
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream
from ._lib_moe_data import MoeRowsDesc, MAX_DIM, MAX_TOPK
from .moe import _rows

__all__ = ["moe_permute", "_moe_permute", "grad_moe_permute", "moe_permute_into", "grad_moe_permute_into", "moe_combine", "_moe_combine",
           "grad_moe_combine", "moe_combine_into", "grad_moe_combine_into"]


# ---- checks: everything raises before any device work ----------------------------------------------------------------------------------
def _tensor(fn, name, t, what):
    if not isinstance(t, torch.Tensor) or t.dim() < 1:
        raise TypeError(f"`{name}` must be a tensor {what}")
    if not t.is_cuda:
        raise NNopError(f"NNop {fn} is GPU-only: tensors must live on a HIP device (there is no CPU or PyTorch fallback).")


def _row_array(fn, name, t, what="[..., D]"):
    _tensor(fn, name, t, what)
    if t.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {t.dtype} of `{name}`; expected float32, float16 or bfloat16")


def _index_array(fn, name, t, what):
    _tensor(fn, name, t, what)
    if t.dtype != torch.int32:
        raise TypeError(f"`{name}` must be int32, got {t.dtype}")


def _weights(fn, name, t):
    _tensor(fn, name, t, "[..., k]")
    if t.dtype != torch.float32:
        raise TypeError(f"`{name}` must be float32 (the gate returns float32; round where you decide to), got {t.dtype}")


def _geometry(fn, T, k, D):
    if not 1 <= D <= MAX_DIM:
        raise NNopError(f"{fn}: the row length must be in 1 ... {MAX_DIM}, got {D}", _lib.NNOP_ERR_SHAPE)
    if T < 1:
        raise NNopError(f"{fn} needs at least one token", _lib.NNOP_ERR_SHAPE)
    if not 1 <= k <= MAX_TOPK:
        raise NNopError(f"{fn}: k must be in 1 ... {MAX_TOPK}, got {k}", _lib.NNOP_ERR_SHAPE)
    if T * k > 2 ** 31 - 1:
        raise NNopError("T * k must be below 2^31", _lib.NNOP_ERR_SHAPE)


def _same(name, t, shape, like):
    """a row array of the shape `shape`, in the dtype and on the device of `like`"""
    if tuple(t.shape) != tuple(shape) or t.dtype != like.dtype or t.device != like.device:
        raise NNopError(f"`{name}` must be a {_dtype_name(like.dtype)} tensor of shape {tuple(shape)} on the device of the "
                        f"other arrays, got {_dtype_name(t.dtype)} {tuple(t.shape)}")


def _side(name, t, shape, like, out=False):
    """an int32 / float32 side array: its dtype is checked already; outputs must be dense, inputs are made so"""
    if tuple(t.shape) != tuple(shape) or t.device != like.device or (out and not t.is_contiguous()):
        raise NNopError(f"`{name}` must be a{' dense' if out else ''} tensor of shape {tuple(shape)} on the device of the other arrays, "
                        f"got {tuple(t.shape)}")
    return t.contiguous()


def _out_rows(name, t, D):
    """a caller-owned row array as the library writes it: (tensor, ld)"""
    r, ld = _rows(t, D)
    if r is not t:
        raise NNopError(f"`{name}` must be dense, or 2-D with unit column stride")
    return t, ld


def _desc(like, T, k, D, ld_tok, ld_slot):
    return MoeRowsDesc(dtype=_DTYPES[like.dtype], tokens=T, topk=k, dim=D, ld_tok=ld_tok, ld_slot=ld_slot)


def _from_slot(fn, slot):
    """slot [..., k] -> (lead, T, k)"""
    _index_array(fn, "slot", slot, "[..., k]")
    k = slot.shape[-1]
    return tuple(slot.shape[:-1]), (slot.numel() // k if k else 0), k


# ---- permute --------------------------------------------------------------------------------------------------------------------------
def moe_permute_into(xs, x, perm):
    """Lowest-level forward: writes xs [T k, D] in the dtype of x [..., D]; k = len(perm) / T.  xs dense, or 2-D with unit column stride."""
    fn = "moe_permute"
    _row_array(fn, "x", x)
    _index_array(fn, "perm", perm, "[T k]")
    _row_array(fn, "xs", xs, "[T k, D]")
    D = x.shape[-1]
    T = x.numel() // D if D else 0
    S = perm.numel()
    if perm.dim() != 1 or T < 1 or S % T != 0:
        raise NNopError(f"`perm` must be a tensor of shape (T k,) with T = {T} tokens, got {tuple(perm.shape)}", _lib.NNOP_ERR_SHAPE)
    k = S // T
    _geometry(fn, T, k, D)
    _same("xs", xs, (S, D), x)
    perm = _side("perm", perm, (S,), x)
    xs, ld_slot = _out_rows("xs", xs, D)
    xr, ld_tok = _rows(x, D)
    d = _desc(x, T, k, D, ld_tok, ld_slot)
    with _on_device(x):
        _raise(_lib_moe_data.load().nnop_moe_permute(C.byref(d), _ptr(xs), _ptr(xr), _ptr(perm), _stream(x)))
    return xs


def _moe_permute(x, perm, slot):
    """xs [T k, D] as a new tensor.  slot [..., k] gives k and must have the leading dimensions of x."""
    fn = "moe_permute"
    _row_array(fn, "x", x)
    _index_array(fn, "perm", perm, "[T k]")
    lead, T, k = _from_slot(fn, slot)
    D = x.shape[-1]
    _geometry(fn, T, k, D)
    if tuple(x.shape[:-1]) != lead:
        raise NNopError(f"`slot` must have the leading dimensions of x, {tuple(x.shape[:-1])} + (k,), got {tuple(slot.shape)}")
    _side("perm", perm, (T * k,), x)
    _side("slot", slot, slot.shape, x)
    with _on_device(x):
        xs = torch.empty((T * k, D), dtype=x.dtype, device=x.device)
    return moe_permute_into(xs, x, perm)


def grad_moe_permute_into(dx, dxs, slot):
    """Lowest-level pullback: writes dx [..., D] (the leading dimensions of slot) from dxs [T k, D]."""
    fn = "grad_moe_permute"
    _row_array(fn, "dxs", dxs, "[T k, D]")
    lead, T, k = _from_slot(fn, slot)
    _row_array(fn, "dx", dx)
    D = dxs.shape[-1]
    _geometry(fn, T, k, D)
    _same("dxs", dxs, (T * k, D), dxs)
    _same("dx", dx, lead + (D,), dxs)
    slot = _side("slot", slot, slot.shape, dxs)
    dx, ld_tok = _out_rows("dx", dx, D)
    rows, ld_slot = _rows(dxs, D)
    d = _desc(dxs, T, k, D, ld_tok, ld_slot)
    with _on_device(dxs):
        _raise(_lib_moe_data.load().nnop_moe_permute_bwd(C.byref(d), _ptr(dx), _ptr(rows), _ptr(slot), _stream(dxs)))
    return dx


def grad_moe_permute(dxs, slot, out=None):
    """Pullback of `_moe_permute`: dxs [T k, D] -> dx [..., D] with the leading dimensions of slot.  `out`: see grad_moe_permute_into."""
    if out is None:
        fn = "grad_moe_permute"
        _row_array(fn, "dxs", dxs, "[T k, D]")
        lead, T, k = _from_slot(fn, slot)
        _geometry(fn, T, k, dxs.shape[-1])
        with _on_device(dxs):
            out = torch.empty(lead + (dxs.shape[-1],), dtype=dxs.dtype, device=dxs.device)
    return grad_moe_permute_into(out, dxs, slot)


class _MoePermute(torch.autograd.Function):
    """x gets the pullback's gradient; perm and slot carry none.  Saves slot alone."""

    @staticmethod
    def forward(ctx, x, perm, slot):
        xs = _moe_permute(x, perm, slot)
        ctx.save_for_backward(slot)
        ctx.set_materialize_grads(False)
        return xs

    @staticmethod
    def backward(ctx, dxs):
        if dxs is None:
            return None, None, None
        (slot,) = ctx.saved_tensors
        return grad_moe_permute(dxs, slot), None, None


def moe_permute(x, perm, slot):
    """xs [T k, D]: the rows of x [..., D] in the expert-sorted order of the plan (perm [T k], slot [..., k])."""
    if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
        _row_array("moe_permute", "x", x)
        return _MoePermute.apply(x, perm, slot)
    return _moe_permute(x, perm, slot)


# ---- combine --------------------------------------------------------------------------------------------------------------------------
def _check_combine(fn, ys, w, slot):
    """-> (lead, T, k, D)"""
    _row_array(fn, "ys", ys, "[T k, D]")
    _weights(fn, "w", w)
    lead, T, k = _from_slot(fn, slot)
    D = ys.shape[-1]
    _geometry(fn, T, k, D)
    _same("ys", ys, (T * k, D), ys)
    return lead, T, k, D


def moe_combine_into(y, ys, w, slot):
    """Lowest-level forward: writes y [..., D] (the leading dimensions of slot) from ys [T k, D], w [..., k] float32, slot [..., k]."""
    fn = "moe_combine"
    lead, T, k, D = _check_combine(fn, ys, w, slot)
    _row_array(fn, "y", y)
    _same("y", y, lead + (D,), ys)
    w = _side("w", w, slot.shape, ys)
    slot = _side("slot", slot, slot.shape, ys)
    y, ld_tok = _out_rows("y", y, D)
    rows, ld_slot = _rows(ys, D)
    d = _desc(ys, T, k, D, ld_tok, ld_slot)
    with _on_device(ys):
        _raise(_lib_moe_data.load().nnop_moe_combine(C.byref(d), _ptr(y), _ptr(rows), _ptr(w), _ptr(slot), _stream(ys)))
    return y


def _moe_combine(ys, w, perm, slot):
    """y [..., D] as a new tensor.  perm is the pullback's; here only its shape is checked."""
    fn = "moe_combine"
    lead, T, k, D = _check_combine(fn, ys, w, slot)
    _index_array(fn, "perm", perm, "[T k]")
    _side("perm", perm, (T * k,), ys)
    _side("w", w, slot.shape, ys)
    with _on_device(ys):
        y = torch.empty(lead + (D,), dtype=ys.dtype, device=ys.device)
    return moe_combine_into(y, ys, w, slot)


def grad_moe_combine_into(dys, dw, dy, ys, w, perm, slot):
    """Lowest-level pullback: writes dys [T k, D] (dense, or 2-D with the row stride of ys) and dw [..., k] float32 (dense)."""
    fn = "grad_moe_combine"
    _row_array(fn, "dy", dy)
    lead, T, k, D = _check_combine(fn, ys, w, slot)
    _index_array(fn, "perm", perm, "[T k]")
    _row_array(fn, "dys", dys, "[T k, D]")
    _weights(fn, "dw", dw)
    _same("dy", dy, lead + (D,), ys)
    _same("dys", dys, (T * k, D), ys)
    w = _side("w", w, slot.shape, ys)
    dw = _side("dw", dw, slot.shape, ys, out=True)
    perm = _side("perm", perm, (T * k,), ys)
    slot = _side("slot", slot, slot.shape, ys)
    rows, ld_slot = _rows(ys, D)
    dys, ld_out = _out_rows("dys", dys, D)
    if T * k > 1 and ld_out != ld_slot:
        raise NNopError("`dys` must be dense like ys, or 2-D with the row stride of ys")
    g, ld_tok = _rows(dy, D)
    d = _desc(ys, T, k, D, ld_tok, ld_slot)
    with _on_device(ys):
        _raise(_lib_moe_data.load().nnop_moe_combine_bwd(C.byref(d), _ptr(dys), _ptr(dw), _ptr(g), _ptr(rows), _ptr(w), _ptr(perm),
                                                         _ptr(slot), _stream(ys)))
    return dys, dw


def grad_moe_combine(dy, ys, w, perm, slot, out=None):
    """Pullback of `_moe_combine`: dy [..., D] -> (dys [T k, D] in the dtype of ys, dw [..., k] float32).  `out`: (dys, dw), see
    grad_moe_combine_into."""
    if out is None:
        _row_array("grad_moe_combine", "dy", dy)
        _check_combine("grad_moe_combine", ys, w, slot)
        ys = ys.contiguous()
        with _on_device(ys):
            out = (torch.empty_like(ys), torch.empty(tuple(slot.shape), dtype=torch.float32, device=ys.device))
    dys, dw = out
    return grad_moe_combine_into(dys, dw, dy, ys, w, perm, slot)


class _MoeCombine(torch.autograd.Function):
    """ys and w get the pullback's gradients; perm and slot carry none.  Saves ys, w, perm, slot: nothing of size [T, k, D]."""

    @staticmethod
    def forward(ctx, ys, w, perm, slot):
        y = _moe_combine(ys, w, perm, slot)
        ctx.save_for_backward(ys, w, perm, slot)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None, None
        ys, w, perm, slot = ctx.saved_tensors
        dys, dw = grad_moe_combine(dy, ys, w, perm, slot)
        return dys, dw, None, None


def moe_combine(ys, w, perm, slot):
    """y [..., D] = sum_j w[..., j] ys[slot[..., j]]: the expert outputs ys [T k, D] back in token order, weighted by the gate."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    if torch.is_grad_enabled() and (needs(ys) or needs(w)):
        _check_combine("moe_combine", ys, w, slot)
        return _MoeCombine.apply(ys, w, perm, slot)
    return _moe_combine(ys, w, perm, slot)
