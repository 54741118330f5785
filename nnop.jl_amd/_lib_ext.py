"""ctypes binding of libnnop_hip_ext.so (the C ABI of include/nnop_hip_ext.h): operators beyond the NNop drop-in boundary.

The second library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``), and so is
the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another ext-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_ext.so")

# NNOP_HIP_EXT_ABI_VERSION of the header this binding was written against; load() refuses another library
EXT_ABI_VERSION = 1


class QknrDesc(C.Structure):
    """struct nnop_qknr_desc"""
    _fields_ = [("dtype", C.c_int32), ("w_dtype", C.c_int32), ("cs_dtype", C.c_int32), ("dim", C.c_int32), ("seq", C.c_int32),
                ("qh", C.c_int32), ("kh", C.c_int32), ("batch", C.c_int32), ("eps", C.c_float), ("offset", C.c_float),
                ("reserved", C.c_int32 * 2)]


_vp, _qd = C.c_void_p, C.POINTER(QknrDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_ext_abi_version": (C.c_int, []),
    "nnop_qk_norm_rope": (C.c_int, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nnop_qk_norm_rope_bwd_workspace_bytes": (C.c_size_t, [_qd]),
    "nnop_qk_norm_rope_bwd": (C.c_int, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "ext-ABI version", "EXT_ABI_VERSION", "nnop_ext_abi_version")
