"""Host-side mirror of NNop.jl's Flash-Attention operator interface over the C ABI.

Same names, argument meaning and error behaviour as the reference (``src/attention_crc.jl:4-31``,
``src/attention.jl:133-177``, ``src/attention_bwd.jl:199-275``), with torch-ROCm tensors standing
in for ``ROCArray`` (device memory + streams only -- every FLOP runs in libnnop_hip.so):

    reference (Julia, column-major)          here (torch, row-major, same bytes)
    q,o     (E, QL, QH, B)                   [B, QH, QL, E]
    k,v     (E, KL, KH, B)                   [B, KH, KL, E]
    ms,ls   (QL, QH, B)                      [B, QH, QL]
    pair    (QH, QL, KL, B)                  [B, KL, QL, QH]
    kpad_mask (KL, B) Bool                   [B, KL] torch.bool

The Julia shim that a maintainer of the reference would load instead is
``nnop.jl_amd/julia/NNopHIPExt.jl``; it makes the identical calls with ``ccall``.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._common import NNopError, _DTYPES, _on_device, _ptr, _raise, _stream
from ._lib import FaDesc

__all__ = [
    "NNopError", "flash_attention", "_flash_attention", "grad_flash_attention",
    "shared_memory", "bwd_workspace_bytes", "fa_fwd_into", "fa_bwd_into",
]


def _jl_shape(t):
    """Shape printed the way the reference prints it (Julia order)."""
    return "(" + ", ".join(str(int(x)) for x in reversed(t.shape)) + ")"


def _raise_status(st, q, k, v):
    """Re-raise a C status with the reference's message (src/attention.jl:141-144)."""
    QE, KE = q.shape[-1], k.shape[-1]
    QH, KH = q.shape[1], k.shape[1]
    if st == _lib.NNOP_ERR_EMB_MISMATCH:
        raise NNopError(f"Embedding dim of Q `{QE}` must be the same as of K `{KE}`.", st)
    if st == _lib.NNOP_ERR_KV_SHAPE:
        raise NNopError(f"Shapes of K `{_jl_shape(k)}` and V `{_jl_shape(v)}` must be the same.", st)
    if st == _lib.NNOP_ERR_EMB_NOT_POW2:
        raise NNopError("Only power-of-2 embedding dims are supported.", st)
    if st == _lib.NNOP_ERR_HEADS:
        raise NNopError(
            f"Number of query heads `{QH}` must be divisible by number of KV heads `{KH}`.", st)
    if st == _lib.NNOP_ERR_EMB_UNSUPPORTED:
        # the reference's counterpart: "Failed to find groupsize ..." (src/attention.jl:204)
        raise NNopError("Failed to find groupsize for Flash Attention that satisfies Shared Memory "
                        f"constraint. ({_lib.strerror(st)})", st)
    raise NNopError(_lib.strerror(st), st)


def _check_inputs(q, k, v, pair, kpad_mask):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise TypeError(f"`{name}` must be a 4-D tensor [B, H, L, E]")
    if not q.is_cuda:
        # the reference's kernels are declared cpu=false (src/attention.jl:1) and its tests
        # refuse to run without a GPU backend (test/runtests.jl:15-17); same here, no fallback.
        raise NNopError("NNop flash attention is GPU-only: tensors must live on a HIP device "
                        "(there is no CPU or PyTorch fallback).")
    if q.dtype not in _DTYPES:
        raise TypeError(f"unsupported element type {q.dtype}; expected float32, float16 or bfloat16")
    others = [k, v] + ([pair] if pair is not None else [])
    for t in others:
        # all of q,k,v,pair share one T in the reference (src/attention.jl:134-137): MethodError
        if t.dtype != q.dtype or t.device != q.device:
            raise TypeError("q, k, v (and pair) must share one dtype and device")
    if pair is not None:
        B, QH, QL, _ = q.shape
        KL = k.shape[2]
        if tuple(pair.shape) != (B, KL, QL, QH):
            raise NNopError(f"pair must have shape [B, KL, QL, QH] = {(B, KL, QL, QH)}, got {tuple(pair.shape)}")
    if kpad_mask is not None:
        if kpad_mask.dtype != torch.bool or kpad_mask.dim() != 2 or kpad_mask.device != q.device:
            raise TypeError("kpad_mask must be a torch.bool matrix [B, KL] on the same device")
        if tuple(kpad_mask.shape) != (q.shape[0], k.shape[2]):
            raise NNopError(f"kpad_mask must have shape [B, KL] = {(q.shape[0], k.shape[2])}")


def _desc(q, k, v, causal):
    B, QH, QL, E = q.shape
    _, KH, KL, KE = k.shape
    return FaDesc(dtype=_DTYPES[q.dtype], emb=E, ql=QL, kl=KL, qh=QH, kh=KH, batch=B,
                  causal=1 if causal else 0, emb_k=KE, emb_v=v.shape[3], kl_v=v.shape[2], kh_v=v.shape[1])


def shared_memory(device_id: int = 0) -> int:
    """``NNop._shared_memory(::ROCBackend, device_id)`` (ext/NNopAMDGPUExt.jl:6-9)."""
    out = C.c_uint64(0)
    _raise(_lib.load().nnop_shared_memory(int(device_id), C.byref(out)))
    return int(out.value)


def bwd_workspace_bytes(q, k, v, *, causal: bool, pair: bool = False) -> int:
    """``nnop_fa_bwd_workspace_bytes``; ``pair=True``: ``nnop_fa_bwd_workspace_bytes_pair`` -- the scratch with which the
    backward of a call WITH a pair bias runs on 16-byte accesses (the small size still works, through the slow direct path)."""
    lib = _lib.load()
    f = lib.nnop_fa_bwd_workspace_bytes_pair if pair else lib.nnop_fa_bwd_workspace_bytes
    return int(f(C.byref(_desc(q, k, v, causal))))


def _softcap(softcap):
    """The cap as the library takes it (0.0 = none).  A negative or non-finite cap raises what the library would answer,
    NNOP_ERR_OPTS, before anything touches the GPU; a non-number is a TypeError."""
    c = _lib.fa_softcap(softcap)
    if not (c >= 0.0 and math.isfinite(c)):
        raise NNopError(f"softcap must be a finite number >= 0 (0 or None: no cap), got {softcap!r}. "
                        f"({_lib.strerror(_lib.NNOP_ERR_OPTS)})", _lib.NNOP_ERR_OPTS)
    return c


def _fwd_call(lib, opts, d, *args, sinks=None, softcap=0.0):
    """nnop_fa_fwd, or nnop_fa_fwd_ex when there are per-call options (window=None issues exactly the old call), or
    nnop_fa_fwd_sinks with sinks (a fp32 tensor; sinks=None issues exactly the call without them), or nnop_fa_fwd_softcap
    with a cap (softcap=0.0 issues exactly the call without one)"""
    if softcap != 0.0:
        return lib.nnop_fa_fwd_softcap(C.byref(d), C.byref(opts) if opts is not None else None, _ptr(sinks),
                                       C.c_float(softcap), *args)
    if sinks is not None:
        return lib.nnop_fa_fwd_sinks(C.byref(d), C.byref(opts) if opts is not None else None, _ptr(sinks), *args)
    if opts is None:
        return lib.nnop_fa_fwd(C.byref(d), *args)
    return lib.nnop_fa_fwd_ex(C.byref(d), C.byref(opts), *args)


def _bwd_call(lib, opts, d, *args, sinks=None, dsinks=None, softcap=0.0):
    if softcap != 0.0:
        return lib.nnop_fa_bwd_softcap(C.byref(d), C.byref(opts) if opts is not None else None, _ptr(sinks), _ptr(dsinks),
                                       C.c_float(softcap), *args)
    if sinks is not None:
        return lib.nnop_fa_bwd_sinks(C.byref(d), C.byref(opts) if opts is not None else None, _ptr(sinks), _ptr(dsinks),
                                     *args)
    if opts is None:
        return lib.nnop_fa_bwd(C.byref(d), *args)
    return lib.nnop_fa_bwd_ex(C.byref(d), C.byref(opts), *args)


def _sinks_f32(sinks, q):
    """Learned attention sinks as the library takes them: a contiguous fp32 [QH] tensor on q's device (None stays None)."""
    if sinks is None:
        return None
    if not isinstance(sinks, torch.Tensor) or sinks.dim() != 1 or sinks.shape[0] != q.shape[1]:
        raise TypeError(f"sinks must be a 1-D tensor [QH] = [{q.shape[1]}], got "
                        f"{tuple(sinks.shape) if isinstance(sinks, torch.Tensor) else type(sinks).__name__}")
    if sinks.dtype not in _DTYPES:
        raise TypeError(f"sinks must be float32, float16 or bfloat16, got {sinks.dtype}")
    if sinks.device != q.device:
        raise TypeError("sinks must live on q's device")
    return sinks.detach().to(torch.float32).contiguous()


def fa_fwd_into(o, ms, ls, q, k, v, pair=None, *, causal: bool, kpad_mask=None, window=None, sinks=None, softcap=None):
    """Raw ``nnop_fa_fwd`` into caller-owned, preallocated outputs (the C ABI's ownership model:
    the caller allocates everything).  No checks beyond the library's own; contiguous tensors only.
    Used by bench.py so that a timed step is exactly one library call.  ``window``, ``sinks``, ``softcap``: see flash_attention
    (``sinks`` here: a contiguous fp32 [QH] tensor, passed as it is)."""
    d = _desc(q, k, v, causal)
    st = _fwd_call(_lib.load(), _lib.fa_opts(window, d), d, _ptr(o), _ptr(ms), _ptr(ls), _ptr(q), _ptr(k), _ptr(v),
                   _ptr(pair), _ptr(kpad_mask), _stream(q), sinks=sinks, softcap=_softcap(softcap))
    if st != _lib.NNOP_OK:
        _raise_status(st, q, k, v)


def fa_bwd_into(dq, dk, dv, dpair, ws, dO, o, ms, ls, q, k, v, pair=None, *, causal: bool, kpad_mask=None, window=None,
                sinks=None, dsinks=None, softcap=None):
    """Raw ``nnop_fa_bwd`` into caller-owned outputs and workspace (see fa_fwd_into).  With ``sinks``, ``dsinks`` is a
    caller-owned fp32 [QH] tensor that receives their gradient."""
    d = _desc(q, k, v, causal)
    st = _bwd_call(_lib.load(), _lib.fa_opts(window, d), d, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dpair), _ptr(dO), _ptr(o),
                   _ptr(ms), _ptr(ls), _ptr(q), _ptr(k), _ptr(v), _ptr(pair), _ptr(kpad_mask),
                   _ptr(ws), C.c_size_t(ws.numel() * ws.element_size()), _stream(q), sinks=sinks, dsinks=dsinks,
                   softcap=_softcap(softcap))
    if st != _lib.NNOP_OK:
        _raise_status(st, q, k, v)


def _flash_attention(q, k, v, pair=None, *, causal: bool, kpad_mask=None, window=None, sinks=None, softcap=None):
    """``NNop._flash_attention`` (src/attention.jl:133-177): returns ``(o, ms, ls)``.

    Asynchronous on the current torch stream, like the reference's KA launch.  ``window``, ``sinks``, ``softcap``: see
    flash_attention (with sinks, ``ms`` and ``ls`` include the sink column; with a cap they are those of the capped logits).
    """
    softcap = _softcap(softcap)
    lib = _lib.load()
    opts = _lib.fa_opts(window)
    _check_inputs(q, k, v, pair, kpad_mask)
    sinks = _sinks_f32(sinks, q)
    if k.shape[0] != q.shape[0]:
        raise NNopError(f"Batch of K `{k.shape[0]}` must be the same as of Q `{q.shape[0]}`.")
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    pair = pair.contiguous() if pair is not None else None
    kpad_mask = kpad_mask.contiguous() if kpad_mask is not None else None
    d = _desc(q, k, v, causal)
    opts = _lib.fa_opts(window, d)            # a window that removes no key: exactly the call without one
    B, QH, QL, E = q.shape
    with _on_device(q):
        o = torch.empty_like(q)                                           # similar(q)      :166
        ms = torch.empty((B, QH, QL), dtype=q.dtype, device=q.device)     # KA.allocate     :167
        ls = torch.empty((B, QH, QL), dtype=q.dtype, device=q.device)     # KA.allocate     :168
        st = _fwd_call(lib, opts, d, _ptr(o), _ptr(ms), _ptr(ls), _ptr(q), _ptr(k), _ptr(v),
                       _ptr(pair), _ptr(kpad_mask), _stream(q), sinks=sinks, softcap=softcap)
    if st != _lib.NNOP_OK:
        _raise_status(st, q, k, v)
    return o, ms, ls


def grad_flash_attention(dO, o, ms, ls, q, k, v, pair=None, *, causal: bool, kpad_mask=None, window=None, sinks=None,
                         softcap=None):
    """``NNop.∇flash_attention`` (src/attention_bwd.jl:199-275): returns ``(dq, dk, dv, dpair|None)``, and with ``sinks``
    ``(dq, dk, dv, dpair|None, dsinks)`` (dsinks: fp32 [QH]).  ``window``, ``sinks``, ``softcap``: the forward's (see
    flash_attention)."""
    softcap = _softcap(softcap)
    lib = _lib.load()
    opts = _lib.fa_opts(window)
    _check_inputs(q, k, v, pair, kpad_mask)
    sinks = _sinks_f32(sinks, q)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    dO, o, ms, ls = dO.contiguous(), o.contiguous(), ms.contiguous(), ls.contiguous()
    if dO.dtype != q.dtype or dO.shape != q.shape:
        raise TypeError("cotangent must have the dtype and shape of the output")
    # residuals of the forward: typed like the reference's signature (o::AbstractArray{T,4}, ms/ls::AbstractArray{T,3},
    # src/attention_bwd.jl:199-207) -- the kernels read them as T with these shapes
    B, QH, QL, _ = q.shape
    if o.dtype != q.dtype or o.shape != q.shape or o.device != q.device:
        raise TypeError("`o` must have the dtype, shape and device of `q`")
    for name, t in (("ms", ms), ("ls", ls)):
        if t.dtype != q.dtype or tuple(t.shape) != (B, QH, QL) or t.device != q.device:
            raise TypeError(f"`{name}` must be a [B, QH, QL] = {(B, QH, QL)} tensor of q's dtype on q's device, "
                            f"got {tuple(t.shape)} {t.dtype}")
    if dO.device != q.device:
        raise TypeError("cotangent must live on q's device")
    pair = pair.contiguous() if pair is not None else None
    kpad_mask = kpad_mask.contiguous() if kpad_mask is not None else None
    d = _desc(q, k, v, causal)
    opts = _lib.fa_opts(window, d)            # a window that removes no key: exactly the call without one
    with _on_device(q):
        dq = torch.empty_like(q)
        dk = torch.empty_like(k)
        dv = torch.empty_like(v)
        dpair = torch.empty_like(pair) if pair is not None else None
        dsinks = torch.empty_like(sinks) if sinks is not None else None
        nbytes = small = int(lib.nnop_fa_bwd_workspace_bytes(C.byref(d)))
        if nbytes != 0 and pair is not None and opts is None and softcap == 0.0:
            # staged pair-bias path: two head-major bias-sized scratch matrices on top (the library returns the small size
            # where that path does not exist: plain-HIP embedding dims, too many heads for its LDS block)
            nbytes = max(nbytes, int(lib.nnop_fa_bwd_workspace_bytes_pair(C.byref(d))))
        if nbytes == 0:
            st = _bwd_call(lib, opts, d, *([C.c_void_p(0)] * 13), C.c_void_p(0), 0, C.c_void_p(0))
            _raise_status(st, q, k, v)
        try:
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        except torch.cuda.OutOfMemoryError:
            if nbytes == small:
                raise
            nbytes = small                     # no room for the scratch: the direct (element-wise) pair path needs none
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        st = _bwd_call(lib, opts, d, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dpair), _ptr(dO), _ptr(o),
                       _ptr(ms), _ptr(ls), _ptr(q), _ptr(k), _ptr(v), _ptr(pair), _ptr(kpad_mask),
                       _ptr(ws), C.c_size_t(nbytes), _stream(q), sinks=sinks, dsinks=dsinks, softcap=softcap)
    if st != _lib.NNOP_OK:
        _raise_status(st, q, k, v)
    if sinks is not None:
        return dq, dk, dv, dpair, dsinks
    return dq, dk, dv, dpair


class _FlashAttentionFn(torch.autograd.Function):
    """``CRC.rrule(::typeof(_flash_attention), ...)`` (src/attention_crc.jl:16-31): the forward
    closes over (o, ms, ls, q, k, v, pair); the pullback maps Δ to (dq, dk, dv, dpair) and gives
    no tangent for kpad_mask."""

    @staticmethod
    def forward(ctx, q, k, v, pair, kpad_mask, causal, window=None, sinks=None, softcap=None):
        o, ms, ls = _flash_attention(q, k, v, pair, causal=causal, kpad_mask=kpad_mask, window=window, sinks=sinks,
                                     softcap=softcap)
        ctx.save_for_backward(o, ms, ls, q, k, v, pair if pair is not None else torch.empty(0),
                              kpad_mask if kpad_mask is not None else torch.empty(0),
                              sinks if sinks is not None else torch.empty(0))
        ctx.has_pair, ctx.has_mask, ctx.causal, ctx.window = pair is not None, kpad_mask is not None, bool(causal), window
        ctx.has_sinks = sinks is not None
        ctx.softcap = softcap                    # a plain float (or None): not differentiable
        return o

    @staticmethod
    def backward(ctx, dO):
        o, ms, ls, q, k, v, pair, mask, sinks = ctx.saved_tensors
        grads = grad_flash_attention(
            dO, o, ms, ls, q, k, v, pair if ctx.has_pair else None,
            causal=ctx.causal, kpad_mask=mask if ctx.has_mask else None, window=ctx.window,
            sinks=sinks if ctx.has_sinks else None, softcap=ctx.softcap)
        dq, dk, dv, dpair = grads[:4]
        dsinks = grads[4].to(sinks.dtype) if ctx.has_sinks else None     # in the sinks tensor's dtype
        return dq, dk, dv, dpair, None, None, None, dsinks, None


def flash_attention(q, k, v, pair=None, *, causal: bool, kpad_mask=None, window=None, sinks=None, softcap=None):
    """``NNop.flash_attention(q, k, v, pair=nothing; causal, kpad_mask=nothing)``
    (src/attention_crc.jl:4-14).  ``causal`` is a required keyword, as in the reference.
    Returns ``o``; differentiable w.r.t. q, k, v, pair through the rrule above.

    ``window=(left, right)``: sliding-window (local) attention in flash-attn's ``window_size`` convention -- query i
    sees key j only if ``i - left <= j <= i + right`` (on top of ``causal`` and ``kpad_mask``); ``-1`` leaves a side
    unbounded.  Top-left aligned (query i lines up with key i) whatever QL and KL are.  ``None``: no window.

    ``sinks``: learned per-head attention sinks (gpt-oss), a 1-D ``[QH]`` float tensor on q's device, one logit per
    query head in the units of the scaled logits.  Each row's softmax gets one more column of logit ``sinks[h]`` and no
    value vector (concatenate, softmax, drop that column); causal, window, kpad_mask and pair act on the real keys only.
    ``-inf`` means no sink for that head.  Differentiable: ``sinks.requires_grad`` gets a gradient in its own dtype.

    ``softcap``: logit soft-capping (Gemma-2: 50, Grok-1: 30; flash-attn's ``softcap``), a float ``c > 0``: the scaled scores
    become ``c * tanh(scale * q.k / c)`` before the pair bias is added (the bias and the sinks are not capped) and before the
    masks and the softmax; fp32 arithmetic for every element type, differentiated through in the backward.  ``None`` or ``0``:
    no cap, exactly the call without the argument.  A negative or non-finite value raises ``NNopError`` (NNOP_ERR_OPTS)."""
    softcap = _softcap(softcap) or None
    if window is not None:
        window = tuple(window)
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (q, k, v, pair, sinks)):
        return _FlashAttentionFn.apply(q, k, v, pair, kpad_mask, bool(causal), window, sinks, softcap)
    return _flash_attention(q, k, v, pair, causal=causal, kpad_mask=kpad_mask, window=window, sinks=sinks, softcap=softcap)[0]
