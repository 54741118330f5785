"""Cross-entropy loss over the last axis of the logits, over the C ABI (include/nnop_hip.h, nnop_cross_entropy / nnop_cross_entropy_bwd):
the loss of an LM head, forward and pullback in one pass over the logits each.  No counterpart in the reference.

    loss = cross_entropy(logits, targets, ignore_index=-100, reduction="mean", label_smoothing=0.0, z_loss=0.0, softcap=0.0,
                         inplace_grad=False)                                   # differentiable in logits; fp32
    loss_rows, lse = _cross_entropy(logits, targets, ...)                      # per-row fp32 losses and log-sum-exp; no autograd
    dlogits = grad_cross_entropy(dloss_rows, lse, logits, targets, ..., out=None)          # out=logits: in place

For a row x of n logits with target t:  z = x, or softcap * tanh(x / softcap) (Gemma-2 caps its final logits with 30);
lse = logsumexp(z);  loss = (1 - label_smoothing) (lse - z_t) + label_smoothing (lse - mean z) + z_loss lse^2  -- label_smoothing as
in torch.nn.functional.cross_entropy, z_loss the PaLM auxiliary term.  Rows whose target equals `ignore_index` have loss 0 and a zero
gradient; a target outside [0, n) that is not `ignore_index` gives a NaN loss and a NaN gradient row (nothing asserts and nothing
synchronises to look at the targets).

`logits` is [..., n] in float32, float16 or bfloat16; `targets` is int32 or int64 with the leading shape.  The leading dims are flattened
to rows; a view whose rows lie one common stride apart -- a [B, L, n] tensor, the [:, :n] slice of a vocabulary padded to a multiple
of 64 -- is handed to the library by stride, not copied; anything else is made contiguous.  The losses and the reductions are float32
and run on the device: "mean" divides by the number of rows that are not ignored (NaN when every row is, as in torch).
The forward keeps `logits`, `targets` and one float per row; nothing of the size of the logits is allocated.  `inplace_grad=True` writes
the gradient over `logits` in the backward: `logits` is dead after backward(), and must not be needed by any other node of the graph.
GPU-only like every operator here.
"""
from __future__ import annotations

import torch

from ._common import NNopError, _DTYPES, _launch, _on_device
from ._lib import XentDesc
from .activations import _row_stride

__all__ = ["cross_entropy", "_cross_entropy", "grad_cross_entropy"]

_REDUCTIONS = ("mean", "sum", "none")
_INDEX = {torch.int32: 4, torch.int64: 8}


def _check(logits, targets):
    """every check of the arguments, before any device work: TypeError for a wrong type, rank, dtype or shape, NNopError for CPU
    tensors and empty input"""
    if not isinstance(logits, torch.Tensor) or logits.dim() < 1:
        raise TypeError("`logits` must be a tensor [..., n]")
    if logits.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {logits.dtype}; expected float32, float16 or bfloat16")
    if not isinstance(targets, torch.Tensor) or targets.dtype not in _INDEX:
        raise TypeError("`targets` must be an int32 or int64 tensor")
    if tuple(targets.shape) != tuple(logits.shape[:-1]):
        raise TypeError(f"`targets` must have the leading shape {tuple(logits.shape[:-1])} of `logits`, got {tuple(targets.shape)}")
    if not logits.is_cuda or not targets.is_cuda:
        raise NNopError("NNop cross_entropy is GPU-only: tensors must live on a HIP device (there is no CPU or PyTorch fallback).")
    if targets.device != logits.device:
        raise TypeError("`targets` must live on the device of `logits`")
    if logits.numel() == 0:
        raise NNopError("cross_entropy needs a non-empty tensor")


def _check_reduction(reduction):
    if reduction not in _REDUCTIONS:
        raise NNopError(f"unknown reduction {reduction!r}; expected one of {', '.join(_REDUCTIONS)}")


def _as_rows(logits):
    """(tensor, rows, n, ld): `logits` as rows of n elements ld apart -- itself when one row stride expresses the view, else a
    contiguous copy"""
    n = logits.shape[-1]
    rows = logits.numel() // n if n else 0
    ld = _row_stride(logits)
    if ld is None:
        logits, ld = logits.contiguous(), n
    return logits, rows, n, ld


def _desc(t, rows, n, ld, ld_grad, targets, ignore_index, label_smoothing, z_loss, softcap, index_base=0):
    return XentDesc(dtype=_DTYPES[t.dtype], index_bytes=_INDEX[targets.dtype], rows=rows, n=n, ld=ld, ld_grad=ld_grad,
                    ignore_index=int(ignore_index), index_base=index_base, reserved=0, label_smoothing=float(label_smoothing),
                    z_loss=float(z_loss), softcap=float(softcap), reserved_f=0.0)


def _cross_entropy(logits, targets, *, ignore_index=-100, label_smoothing=0.0, z_loss=0.0, softcap=0.0):
    """-> (loss_rows, lse), float32 with the leading shape of `logits`; no autograd."""
    _check(logits, targets)
    x, rows, n, ld = _as_rows(logits)
    targets = targets.contiguous()
    with _on_device(x):
        loss = torch.empty(logits.shape[:-1], dtype=torch.float32, device=x.device)
        lse = torch.empty_like(loss)
    d = _desc(x, rows, n, ld, ld, targets, ignore_index, label_smoothing, z_loss, softcap)
    _launch("nnop_cross_entropy", d, x, loss.data_ptr(), lse.data_ptr(), x.data_ptr(), targets.data_ptr())
    return loss, lse


def grad_cross_entropy(dloss_rows, lse, logits, targets, *, ignore_index=-100, label_smoothing=0.0, z_loss=0.0, softcap=0.0, out=None):
    """Pullback of `_cross_entropy` -> dlogits with the shape of `logits`.  `dloss_rows` (the cotangent of every row's loss) and `lse`
    are float32 with the leading shape.  `out`: where to write -- a tensor like `logits` whose rows lie one stride apart; `out=logits`
    writes the gradient over the logits (in place).  The elements between n and the row stride of `out` are not written."""
    _check(logits, targets)
    lead = tuple(logits.shape[:-1])
    for name, t in (("dloss_rows", dloss_rows), ("lse", lse)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != lead or t.device != logits.device:
            raise TypeError(f"`{name}` must be a float32 tensor of shape {lead} on the device of `logits`")
    x, rows, n, ld = _as_rows(logits)
    if out is None:
        with _on_device(x):
            out = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        ld_grad = n
    else:
        if not isinstance(out, torch.Tensor) or out.shape != logits.shape or out.dtype != logits.dtype or out.device != logits.device:
            raise TypeError("`out` must match `logits` in shape, dtype and device")
        ld_grad = _row_stride(out)
        if ld_grad is None:
            raise TypeError("`out` must be rows of unit element stride that lie one common stride apart")
        if out is logits and x is not logits:
            raise TypeError("in place needs `logits` as rows that lie one common stride apart")
        if out is not logits and out.data_ptr() == x.data_ptr():
            raise TypeError("`out` may alias `logits` only by being that very tensor")
    targets, dloss_rows, lse = targets.contiguous(), dloss_rows.contiguous(), lse.contiguous()
    d = _desc(x, rows, n, ld, ld_grad, targets, ignore_index, label_smoothing, z_loss, softcap)
    _launch("nnop_cross_entropy_bwd", d, x, out.data_ptr(), dloss_rows.data_ptr(), lse.data_ptr(), x.data_ptr(), targets.data_ptr())
    return out


def _reduce(loss_rows, targets, ignore_index, reduction):
    """(reduced loss, count): on the device, float32; count (a 0-dim tensor) only for "mean" """
    if reduction == "none":
        return loss_rows, None
    if reduction == "sum":
        return loss_rows.sum(), None
    count = (targets != ignore_index).sum().to(torch.float32)
    return loss_rows.sum() / count, count


class _CrossEntropy(torch.autograd.Function):
    """Saves logits, targets and lse (one float per row); the probabilities are recomputed in the pullback."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index, reduction, label_smoothing, z_loss, softcap, inplace_grad):
        opts = dict(ignore_index=ignore_index, label_smoothing=label_smoothing, z_loss=z_loss, softcap=softcap)
        x = _as_rows(logits)[0]                                  # a copy only when no row stride expresses the view
        loss_rows, lse = _cross_entropy(x, targets, **opts)
        out, count = _reduce(loss_rows, targets, ignore_index, reduction)
        ctx.save_for_backward(x, targets, lse, *(() if count is None else (count,)))
        ctx.opts, ctx.reduction, ctx.inplace = opts, reduction, inplace_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        x, targets, lse, *rest = ctx.saved_tensors
        g = dout.to(torch.float32)
        if ctx.reduction == "mean":
            g = g / rest[0]
        g = g.expand(lse.shape).contiguous()
        dx = grad_cross_entropy(g, lse, x, targets, out=x if ctx.inplace else None, **ctx.opts)
        return dx, None, None, None, None, None, None, None


def cross_entropy(logits, targets, *, ignore_index=-100, reduction="mean", label_smoothing=0.0, z_loss=0.0, softcap=0.0,
                  inplace_grad=False):
    """Cross-entropy of logits [..., n] against class indices `targets` [...] -> float32: a scalar for reduction "mean" (over the
    rows that are not ignored) or "sum", the per-row losses for "none".  Differentiable in `logits`.  With `inplace_grad=True` the
    backward writes the gradient over `logits`, which is dead after backward()."""
    _check(logits, targets)
    _check_reduction(reduction)
    if torch.is_grad_enabled() and logits.requires_grad:
        return _CrossEntropy.apply(logits, targets, int(ignore_index), reduction, float(label_smoothing), float(z_loss),
                                   float(softcap), bool(inplace_grad))
    loss_rows, _ = _cross_entropy(logits, targets, ignore_index=ignore_index, label_smoothing=label_smoothing, z_loss=z_loss,
                                  softcap=softcap)
    return _reduce(loss_rows, targets, ignore_index, reduction)[0]
