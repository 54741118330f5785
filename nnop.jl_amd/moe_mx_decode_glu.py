"""The first half of an expert MLP at decode sizes in one launch, over the C ABI of the ninth library
(include/nnop_hip_moe_mx_decode_glu.h; no counterpart in the reference): moe_mx_decode.py's weight-streaming forward on the MXFP4 weights
of a fused gate-up projection, with activations.py's gated activation in its epilogue and, optionally, moe_data.py's token gather in
front.

    h = moe_decode_glu_mxfp4(x, blocks, scales, offsets, bias=None, act="swiglu_oai", layout="interleaved",
                             alpha=1.702, limit=7.0, perm=None, k=None)        # differentiable in x and bias when perm is None
    h = _moe_decode_glu_mxfp4(...)                                             # no autograd
    moe_decode_glu_mxfp4_into(h, ...)                                          # caller-owned buffer

    p[s] = W_e xrow(s) + bias[e]  in fp32, for offsets[e] <= s < offsets[e+1],  W_e = mxfp4_dequantize(blocks[e], scales[e], x.dtype)
    h[s, j] = act(gate) * upside(up)    gate, up = p[s, 2j], p[s, 2j+1] ("interleaved", gpt-oss)  or  p[s, j], p[s, I+j] ("halves")
    xrow(s) = x[s] without perm;  x[perm[s] // k] with perm (an entry outside [0, T k): a row of zeros, as moe_permute has it)

It computes what glu_packed(moe_decode_linear_mxfp4(moe_permute(x, perm, slot), blocks, scales, offsets, bias), act, layout) computes, in
one launch instead of three, and without rounding the [S, 2 I] pre-activations to 16 bits: they stay in the accumulators.  x [S, K]
(with perm: [T, K] and perm [T k] int32, k = `k`), h [S, I], offsets [E+1] int32, bias [E, 2 I], scales [E, 2 I, K/32], blocks
[E, 2 I, K/32, 16] or [E, 2 I, K/2]; rows and bias float16 or bfloat16; `blocks` and `scales` uint8, contiguous, never copied.  `act`
names and `alpha`, `limit` are those of activations.py.  Contracts:

  - fp32 sums on the matrix cores, the bias added in fp32, the activation in fp32, one rounding; no atomics, no workspace, no sync,
    graph-capturable; two runs are bitwise equal; rows outside every expert are +0; nothing is touched out of bounds whatever `offsets`
    or `perm` hold.
  - The pre-activations are summed in moe_decode_linear_mxfp4's order (a function of K and the dtype alone) and the activation code is
    glu's: a row's bits do not depend on the plan, on its slot, on its neighbours or on whether it came through `perm`; the two layouts
    give the same bits for the same weights laid out either way; and wherever every pre-activation is exactly representable in the
    dtype, h equals glu_packed(moe_decode_linear_mxfp4(...)) bit for bit.  Elsewhere h carries one rounding where that carries two.
  - Measured on an MI355X (bf16, E = 128, k = 4, 2880 -> 2 x 2880, swiglu_oai, a bias; DESIGN.md section 4.17,
    tools/perf_moe_mx_decode_glu.py) against the launches it replaces: with `perm` 1.12 / 1.08 / 1.03 x faster at S = 4 / 16 / 64 slot
    rows (37.9 against 42.6 us at S = 4) and 1.03 x at S = 256 and 1024; without `perm` 1.05 / 1.03 / 1.01 x, inside the spread of the two
    arms from S = 16 on.  Never slower; the gain is the one or two launches saved, the kernel's own time is moe_decode_linear_mxfp4's.

Autograd (without `perm`) is by recomputation through kernels that exist: the pre-activations are recomputed by
_moe_decode_linear_mxfp4, grad_glu_packed gives their gradient, grad_moe_grouped_linear_mxfp4_x_into and grad_moe_grouped_linear_b_into
the gradients of x and bias -- bit for bit the gradients of glu_packed(moe_decode_linear_mxfp4(x, ..., bias)).  Saved: blocks, scales,
offsets, x, and the bias where there is one (the recomputation adds it).  With `perm` and a tensor that requires a gradient the call
raises: a decode step has no use for that case and the permute's pullback needs `slot`; compose moe_permute, moe_decode_linear_mxfp4 and
glu_packed there.  GPU-only: no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _lib_moe_mx_decode_glu
from ._common import NNopError, _DTYPES, _dtype_name, _on_device, _ptr, _raise, _stream  # noqa: F401  (the shared plumbing)
from ._lib_moe_mx import BLOCK
from ._lib_moe_mx_decode_glu import LAYOUTS, MAX_TOPK, MoeMxDecodeGluDesc
from .activations import OAI_ALPHA, OAI_LIMIT, _act, grad_glu_packed
from .moe import _rows
from .moe_data import _index_array, _out_rows, _row_array, _same, _side
from .moe_gemm import _offsets
from .moe_linear import _bias, grad_moe_grouped_linear_b_into
from .moe_mx import _check, grad_moe_grouped_linear_mxfp4_x_into
from .moe_mx_decode import _moe_decode_linear_mxfp4

__all__ = ["moe_decode_glu_mxfp4", "_moe_decode_glu_mxfp4", "moe_decode_glu_mxfp4_into"]

FN = "moe_decode_glu_mxfp4"


def _layout(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}; expected 'interleaved' or 'halves'")
    return LAYOUTS[layout]


def _geometry(x, blocks, scales, offsets, bias, perm, k):
    """every host check of the inputs -> (S, E, I, K, T, k, offsets, perm); T = k = 0 without perm"""
    T, E, N, K = _check(FN, "x", x, 2, blocks, scales)
    if N % 2:
        raise NNopError(f"{FN}: the packed weights must hold 2 I rows per expert (gate and up), got {N}", _lib.NNOP_ERR_SHAPE)
    offsets = _offsets(FN, offsets, E, x)
    if bias is not None:
        _bias(FN, "bias", bias, E, N, x)
    if perm is None:
        if k is not None:
            raise NNopError(f"{FN}: `k` is given without `perm`", _lib.NNOP_ERR_SHAPE)
        return T, E, N // 2, K, 0, 0, offsets, None
    _index_array(FN, "perm", perm, "[T k]")
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_TOPK:
        raise NNopError(f"{FN}: with `perm`, `k` must be an integer in 1 ... {MAX_TOPK}, got {k!r}", _lib.NNOP_ERR_SHAPE)
    if T * k > 2 ** 31 - 1:
        raise NNopError("T * k must be below 2^31", _lib.NNOP_ERR_SHAPE)
    perm = _side("perm", perm, (T * k,), x)
    return T * k, E, N // 2, K, T, k, offsets, perm


def _desc(like, S, E, K, I, act, layout, alpha, limit, T=0, k=0, ld_x=None, ld_h=None, ld_b=None):
    """moe_mx_decode._desc for the ninth library's descriptor: the packed strides are the dense ones"""
    return MoeMxDecodeGluDesc(dtype=_DTYPES[like.dtype], rows=S, experts=E, in_dim=K, inter_dim=I, ld_x=ld_x or K, ld_h=ld_h or I,
                              ld_b=ld_b or 2 * I, ld_q=K // 2, ld_s=K // BLOCK, act=act, layout=layout, tokens=T, topk=k,
                              alpha=float(alpha), limit=float(limit), flags=0)


def moe_decode_glu_mxfp4_into(h, x, blocks, scales, offsets, bias=None, act="swiglu_oai", layout="interleaved", alpha=OAI_ALPHA,
                              limit=OAI_LIMIT, perm=None, k=None):
    """Lowest-level forward: writes h [S, I] (S = len(perm) with perm, else the rows of x).  h dense, or 2-D with unit column stride."""
    a, lay = _act(act), _layout(layout)
    S, E, I, K, T, k, offsets, perm = _geometry(x, blocks, scales, offsets, bias, perm, k)
    _row_array(FN, "h", h, "[S, I]")
    _same("h", h, (S, I), x)
    h, ld_h = _out_rows("h", h, I)
    xr, ld_x = _rows(x, K)
    br, ld_b = _rows(bias, 2 * I) if bias is not None else (None, 2 * I)
    d = _desc(x, S, E, K, I, a, lay, alpha, limit, T, k, ld_x=ld_x, ld_h=ld_h, ld_b=ld_b)
    with _on_device(x):
        _raise(_lib_moe_mx_decode_glu.load().nnop_moe_mx_decode_glu(C.byref(d), _ptr(h), _ptr(xr), _ptr(blocks), _ptr(scales), _ptr(br),
                                                                    _ptr(offsets), _ptr(perm), _stream(x)))
    return h


def _moe_decode_glu_mxfp4(x, blocks, scales, offsets, bias=None, act="swiglu_oai", layout="interleaved", alpha=OAI_ALPHA, limit=OAI_LIMIT,
                          perm=None, k=None):
    """h [S, I] as a new tensor."""
    _act(act), _layout(layout)
    S, _, I, *_ = _geometry(x, blocks, scales, offsets, bias, perm, k)
    with _on_device(x):
        h = torch.empty((S, I), dtype=x.dtype, device=x.device)
    return moe_decode_glu_mxfp4_into(h, x, blocks, scales, offsets, bias, act, layout, alpha, limit, perm, k)


class _MoeDecodeGluMxfp4(torch.autograd.Function):
    """The fused forward with the pullbacks of the calls it replaces, on recomputed pre-activations: _moe_decode_linear_mxfp4,
    grad_glu_packed, then dx from the seventh library and db from the sixth's bias gradient, each only where asked for.  Saves blocks,
    scales, offsets, x, and the bias where there is one."""

    @staticmethod
    def forward(ctx, x, blocks, scales, offsets, bias, act, layout, alpha, limit):
        h = _moe_decode_glu_mxfp4(x, blocks, scales, offsets, bias, act, layout, alpha, limit)
        ctx.save_for_backward(*((blocks, scales, offsets, x) + (() if bias is None else (bias,))))
        ctx.opts = (act, layout, alpha, limit)
        ctx.set_materialize_grads(False)
        return h

    @staticmethod
    def backward(ctx, dh):
        if dh is None:
            return (None,) * 9
        blocks, scales, offsets, x, *rest = ctx.saved_tensors
        bias = rest[0] if rest else None
        act, layout, alpha, limit = ctx.opts
        need = ctx.needs_input_grad
        gu = _moe_decode_linear_mxfp4(x.detach(), blocks, scales, offsets, None if bias is None else bias.detach())
        dgu = grad_glu_packed(dh, gu, act=act, layout=layout, alpha=alpha, limit=limit, dgu_out=gu)
        dx = db = None
        with _on_device(dh):
            if need[0]:
                dx = torch.empty(x.shape, dtype=dh.dtype, device=dh.device)
            if need[4]:
                db = torch.empty(bias.shape, dtype=dh.dtype, device=dh.device)
        if need[0]:
            grad_moe_grouped_linear_mxfp4_x_into(dx, dgu, blocks, scales, offsets)
        if need[4]:
            grad_moe_grouped_linear_b_into(db, dgu, offsets)
        return dx, None, None, None, db, None, None, None, None


def moe_decode_glu_mxfp4(x, blocks, scales, offsets, bias=None, act="swiglu_oai", layout="interleaved", alpha=OAI_ALPHA, limit=OAI_LIMIT,
                         perm=None, k=None):
    """h [S, I]: row s (with perm: token perm[s] // k) of x through the fused gate-up projection (the MXFP4 weights of expert e, bias[e]) of
    the expert whose range offsets[e] ... offsets[e+1]-1 holds s and through the gated activation, by the weight-streaming kernel."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    if torch.is_grad_enabled() and (needs(x) or needs(bias)):
        _act(act), _layout(layout)
        _geometry(x, blocks, scales, offsets, bias, perm, k)
        if perm is not None:
            raise NNopError(f"{FN}: no gradient with `perm` (the permute's pullback needs `slot`): compose moe_permute, "
                            "moe_decode_linear_mxfp4 and glu_packed for that")
        return _MoeDecodeGluMxfp4.apply(x, blocks, scales, offsets, bias, act, layout, float(alpha), float(limit))
    return _moe_decode_glu_mxfp4(x, blocks, scales, offsets, bias, act, layout, alpha, limit, perm, k)
