"""Gated MLP activations over the C ABI (include/nnop_hip.h, nnop_glu / nnop_glu_bwd): y = act(gate) * up, the element-wise step of
a Llama / Gemma / gpt-oss MLP, forward and pullback in one pass over memory each.  No counterpart in the reference.

    y = glu(gate, up, act="silu", alpha=1.702, limit=7.0)          # differentiable; act: silu | gelu_tanh | gelu_erf | swiglu_oai
    y = swiglu(gate, up)                                            # act="silu"
    y = geglu(gate, up, approximate="tanh")                         # "tanh" | "none" (the exact GELU)
    y = glu_packed(gu, act=..., layout="halves" | "interleaved")    # gu [..., 2n]: one fused gate-up projection; differentiable
    y = _glu(gate, up, act=...)                                     # no autograd
    dgate, dup = grad_glu(dy, gate, up, act=...)                    # a and a' are recomputed: only gate and up are needed
    dgu = grad_glu_packed(dy, gu, act=..., layout=..., dgu_out=None)    # dgu_out may be gu itself (in place)
    glu_into(y, gate, up, act=...)                                  # y may be gate or up themselves (contiguous)
    grad_glu_into(dgate, dup, dy, gate, up, act=...)                # dgate may be gate, dup may be up

Tensors are [..., n]; leading dims are flattened.  `gate` and `up` that are views with unit last stride and one common row stride -- the
halves `gu.chunk(2, -1)` of a fused projection -- are handed to the library by stride, not copied; anything else is made contiguous.
`layout="halves"`: gate = gu[..., :n], up = gu[..., n:];  "interleaved": gate = gu[..., 0::2], up = gu[..., 1::2] (gpt-oss), and `act="swiglu_oai"`
picks it by default.  GPU-only like every operator here.
"""
from __future__ import annotations

import torch

from . import _lib
from ._common import NNopError, _DTYPES, _launch
from ._lib import GluDesc

__all__ = ["glu", "swiglu", "geglu", "glu_packed", "_glu", "grad_glu", "grad_glu_packed", "glu_into", "grad_glu_into"]

OAI_ALPHA, OAI_LIMIT = 1.702, 7.0          # gpt-oss


def _act(act):
    if act not in _lib.GLU_ACTS:
        raise ValueError(f"unknown act {act!r}; expected one of {', '.join(_lib.GLU_ACTS)}")
    return _lib.GLU_ACTS[act]


def _layout(layout, act):
    if layout is None:
        layout = "interleaved" if act == "swiglu_oai" else "halves"
    if layout not in ("halves", "interleaved"):
        raise ValueError(f"unknown layout {layout!r}; expected 'halves' or 'interleaved'")
    return layout


def _check(gate, name="gate"):
    if not isinstance(gate, torch.Tensor) or gate.dim() < 1:
        raise TypeError(f"`{name}` must be a tensor [..., n]")
    if not gate.is_cuda:
        raise NNopError("NNop gated activations are GPU-only: tensors must live on a HIP device "
                        "(there is no CPU or PyTorch fallback).")
    if gate.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {gate.dtype}; expected float32, float16 or bfloat16")
    if gate.numel() == 0:
        raise NNopError("gated activations need a non-empty tensor")


def _check_like(x, shape=None, **others):
    """tensors that must match x in dtype and device and have x's shape (or `shape`)"""
    shape = tuple(x.shape) if shape is None else tuple(shape)
    for name, t in others.items():
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != x.dtype or t.device != x.device:
            raise TypeError(f"`{name}` must have shape {shape} and the dtype and device of the gate")


def _row_stride(t):
    """ld when t [..., n] is rows of unit element stride that lie one common stride ld >= n apart once the leading dims are
    flattened (a contiguous tensor: ld = n), else None"""
    n = t.shape[-1]
    if n != 1 and t.stride(-1) != 1:
        return None
    ld = expect = None
    for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
        if size == 1:
            continue
        if expect is None:
            ld = stride
        elif stride != expect:
            return None
        expect = stride * size
    if ld is None:                          # one row
        return n
    return ld if ld >= n else None


def _by_stride(gate, up):
    """(gate, up, ld): the tensors as the library takes them -- themselves when both are rows with one common stride, else
    contiguous copies"""
    lg, lu = _row_stride(gate), _row_stride(up)
    if lg is not None and lg == lu:
        return gate, up, lg
    return gate.contiguous(), up.contiguous(), gate.shape[-1]


def _desc(t, act, layout, n, ld, alpha, limit):
    return GluDesc(dtype=_DTYPES[t.dtype], act=act, layout=layout, reserved=0, rows=t.numel() // t.shape[-1], n=n, ld=ld,
                   alpha=float(alpha), limit=float(limit))


def glu_into(y, gate, up, *, act="silu", alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """y[...] = act(gate) * up into the caller's `y` (contiguous).  `y` may be `gate` or `up` themselves when they are contiguous."""
    a = _act(act)
    _check(gate)
    _check_like(gate, up=up, y=y)
    if not y.is_contiguous():
        raise TypeError("`y` must be contiguous")
    if not (y is gate or y is up) and y.data_ptr() in (gate.data_ptr(), up.data_ptr()):
        raise TypeError("`y` may alias an input only by being that very tensor")
    g, u, ld = _by_stride(gate, up)
    _launch("nnop_glu", _desc(g, a, _lib.GLU_SPLIT, g.shape[-1], ld, alpha, limit), g, y.data_ptr(), g.data_ptr(), u.data_ptr())
    return y


def _glu(gate, up, *, act="silu", alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """act(gate) * up -> y (new, contiguous); no autograd."""
    _act(act)
    _check(gate)
    _check_like(gate, up=up)
    return glu_into(torch.empty(gate.shape, dtype=gate.dtype, device=gate.device), gate, up, act=act, alpha=alpha, limit=limit)


def grad_glu_into(dgate, dup, dy, gate, up, *, act="silu", alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """Pullback into the caller's `dgate`, `dup`, which must be laid out like `gate`, `up` (same strides).  `dgate` may be `gate`
    and `dup` may be `up` themselves (in place).  The padding between n and the row stride is not written."""
    a = _act(act)
    _check(gate)
    _check_like(gate, up=up, dy=dy, dgate=dgate, dup=dup)
    lg = _row_stride(gate)
    if lg is None or _row_stride(up) != lg:
        if dgate is gate or dup is up:
            raise TypeError("in place needs `gate` and `up` as rows with one common stride")
        gate, up, lg = gate.contiguous(), up.contiguous(), gate.shape[-1]
    if _row_stride(dgate) != lg or _row_stride(dup) != lg:
        raise TypeError("`dgate` and `dup` must have the row stride of `gate` and `up`")
    for out, inp, name in ((dgate, gate, "dgate"), (dup, up, "dup")):
        if out is not inp and out.data_ptr() in (gate.data_ptr(), up.data_ptr(), dy.data_ptr()):
            raise TypeError(f"`{name}` may alias an input only by being that very tensor")
    dy = dy.contiguous()
    _launch("nnop_glu_bwd", _desc(gate, a, _lib.GLU_SPLIT, gate.shape[-1], lg, alpha, limit), gate,
            dgate.data_ptr(), dup.data_ptr(), dy.data_ptr(), gate.data_ptr(), up.data_ptr())
    return dgate, dup


def grad_glu(dy, gate, up, *, act="silu", alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """Pullback of `_glu` -> (dgate, dup), laid out like gate and up (strided views get strided gradients)."""
    _act(act)
    _check(gate)
    _check_like(gate, up=up, dy=dy)
    gate, up, _ = _by_stride(gate, up)
    dgate = torch.empty_strided(gate.shape, gate.stride(), dtype=gate.dtype, device=gate.device)
    dup = torch.empty_strided(up.shape, up.stride(), dtype=up.dtype, device=up.device)
    return grad_glu_into(dgate, dup, dy, gate, up, act=act, alpha=alpha, limit=limit)


def _check_packed(gu):
    _check(gu, "gu")
    if gu.shape[-1] % 2:
        raise TypeError(f"`gu` must be [..., 2n]; its last dim is {gu.shape[-1]}")
    return gu.shape[-1] // 2


def _packed_ptrs(t, n, layout):
    """(gate, up) addresses inside a contiguous [..., 2n] tensor"""
    return (t.data_ptr(), 0) if layout == "interleaved" else (t.data_ptr(), t.data_ptr() + n * t.element_size())


def _glu_packed(gu, *, act="silu", layout=None, alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """glu of one fused projection gu [..., 2n] -> y [..., n]; no autograd, no copy of a contiguous gu."""
    a, layout = _act(act), _layout(layout, act)
    n = _check_packed(gu)
    gu = gu.contiguous()
    y = torch.empty(gu.shape[:-1] + (n,), dtype=gu.dtype, device=gu.device)
    d = _desc(gu, a, _lib.GLU_INTERLEAVED if layout == "interleaved" else _lib.GLU_SPLIT, n, 2 * n, alpha, limit)
    _launch("nnop_glu", d, gu, y.data_ptr(), *_packed_ptrs(gu, n, layout))
    return y


def grad_glu_packed(dy, gu, *, act="silu", layout=None, alpha=OAI_ALPHA, limit=OAI_LIMIT, dgu_out=None):
    """Pullback of `_glu_packed` -> dgu, laid out like gu.  `dgu_out` may be `gu` itself (contiguous): the gradient replaces it."""
    a, layout = _act(act), _layout(layout, act)
    n = _check_packed(gu)
    _check_like(gu, gu.shape[:-1] + (n,), dy=dy)
    if dgu_out is not None:
        _check_like(gu, dgu_out=dgu_out)
        if not dgu_out.is_contiguous():
            raise TypeError("`dgu_out` must be contiguous")
        if dgu_out is not gu and dgu_out.data_ptr() in (gu.data_ptr(), dy.data_ptr()):
            raise TypeError("`dgu_out` may alias an input only by being that very tensor")
    gu, dy = gu.contiguous(), dy.contiguous()
    dgu = torch.empty_like(gu) if dgu_out is None else dgu_out
    d = _desc(gu, a, _lib.GLU_INTERLEAVED if layout == "interleaved" else _lib.GLU_SPLIT, n, 2 * n, alpha, limit)
    _launch("nnop_glu_bwd", d, gu, *_packed_ptrs(dgu, n, layout), dy.data_ptr(), *_packed_ptrs(gu, n, layout))
    return dgu


class _Glu(torch.autograd.Function):
    """Saves gate and up only (as given: views keep their storage); a and a' are recomputed in the pullback."""

    @staticmethod
    def forward(ctx, gate, up, act, alpha, limit):
        y = _glu(gate, up, act=act, alpha=alpha, limit=limit)
        ctx.save_for_backward(gate, up)
        ctx.opts = (act, alpha, limit)
        return y

    @staticmethod
    def backward(ctx, dy):
        gate, up = ctx.saved_tensors
        act, alpha, limit = ctx.opts
        dgate, dup = grad_glu(dy, gate, up, act=act, alpha=alpha, limit=limit)
        return dgate, dup, None, None, None


class _GluPacked(torch.autograd.Function):
    """Saves gu only; one gradient dgu."""

    @staticmethod
    def forward(ctx, gu, act, layout, alpha, limit):
        y = _glu_packed(gu, act=act, layout=layout, alpha=alpha, limit=limit)
        ctx.save_for_backward(gu)
        ctx.opts = (act, layout, alpha, limit)
        return y

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        act, layout, alpha, limit = ctx.opts
        return grad_glu_packed(dy, gu, act=act, layout=layout, alpha=alpha, limit=limit), None, None, None, None


def glu(gate, up, act="silu", alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """y = act(gate) * up for gate, up [..., n]; act: "silu" (SwiGLU), "gelu_tanh", "gelu_erf" (GeGLU), "swiglu_oai" (gpt-oss:
    min(g, limit) * sigmoid(alpha * min(g, limit)) * (clamp(u, -limit, limit) + 1)).  Differentiable."""
    if torch.is_grad_enabled() and (gate.requires_grad or up.requires_grad):
        _act(act)
        _check(gate)
        _check_like(gate, up=up)
        return _Glu.apply(gate, up, act, float(alpha), float(limit))
    return _glu(gate, up, act=act, alpha=alpha, limit=limit)


def swiglu(gate, up):
    """silu(gate) * up"""
    return glu(gate, up, "silu")


def geglu(gate, up, approximate="tanh"):
    """gelu(gate) * up; approximate: "tanh" (Gemma) or "none" (the exact, erf GELU), as torch.nn.functional.gelu names them"""
    if approximate not in ("tanh", "none"):
        raise ValueError(f"approximate must be 'tanh' or 'none', got {approximate!r}")
    return glu(gate, up, "gelu_tanh" if approximate == "tanh" else "gelu_erf")


def glu_packed(gu, act="silu", layout=None, alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """glu of one fused gate-up projection gu [..., 2n] -> y [..., n].  layout: "halves" (gate = gu[..., :n], up = gu[..., n:]) or
    "interleaved" (gate = gu[..., 0::2], up = gu[..., 1::2]); None: "interleaved" for act="swiglu_oai" (gpt-oss), else "halves".
    Differentiable, with one gradient dgu."""
    if torch.is_grad_enabled() and gu.requires_grad:
        _act(act)
        layout = _layout(layout, act)
        _check_packed(gu)
        return _GluPacked.apply(gu, act, layout, float(alpha), float(limit))
    return _glu_packed(gu, act=act, layout=layout, alpha=alpha, limit=limit)
