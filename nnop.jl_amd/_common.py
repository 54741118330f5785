"""The call plumbing every operator module shares: the error type, the dtype codes, how a tensor becomes a pointer, a stream and a
device guard, and the check of a returned status.  Argument checks are not here: their wording and order are each operator's API.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import _lib


class NNopError(RuntimeError):
    """Counterpart of the ``ErrorException`` raised by the reference's ``error(...)`` calls."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


_DTYPES = {torch.float32: _lib.NNOP_F32, torch.float16: _lib.NNOP_F16, torch.bfloat16: _lib.NNOP_BF16}


def _dtype_name(dtype):
    """torch.float32 -> "float32", for messages"""
    return str(dtype).replace("torch.", "")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# Per-call host cost matters for launch-bound shapes (a norm over 1024 x 1024 runs 4 us on the GPU): take the raw stream
# handle without building a torch.cuda.Stream object, and skip the device guard when the tensor's device is current.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_NO_GUARD = contextlib.nullcontext()


def _stream(t):
    if _raw_stream is not None:
        idx = t.device.index
        return C.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _on_device(t):
    """Context that makes t's device current for allocations and the launch (a no-op when it already is)."""
    idx = t.device.index
    return _NO_GUARD if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(t.device)


def _raise(st):
    """NNopError with the library's message for any status but NNOP_OK"""
    if st != _lib.NNOP_OK:
        raise NNopError(_lib.strerror(st), st)


def _launch(name, d, t, *ptrs):
    """Call entry point `name` of the main library as (desc, pointers ..., stream): `ptrs` are raw addresses (0 = NULL), `t` a
    tensor on the target device"""
    with _on_device(t):
        st = getattr(_lib.load(), name)(C.byref(d), *(C.c_void_p(p) for p in ptrs), _stream(t))
    _raise(st)
