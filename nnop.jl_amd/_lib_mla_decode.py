"""ctypes binding of libnnop_hip_mla_decode.so (the C ABI of include/nnop_hip_mla_decode.h): the decode step of multi-head latent attention
(DeepSeek's MLA in its weight-absorbed form) over a paged latent cache -- one 576-wide row per key that is the key and the value of every
query head.

The eighteenth library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``), and so is
the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another mla-decode-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_mla_decode.so")

# NNOP_HIP_MLA_DECODE_ABI_VERSION of the header this binding was written against; load() refuses another library
MLA_DECODE_ABI_VERSION = 1

# NNOP_MLA_DECODE_WIDTH, _LATENT, _MAX_HEADS, _MAX_QL, _MAX_SPLITS, _MIN_PAGE_SIZE
WIDTH, LATENT, MAX_HEADS, MAX_QL, MAX_SPLITS, MIN_PAGE_SIZE = 576, 512, 128, 8, 64, 16


class MlaDecodeDesc(C.Structure):
    """struct nnop_mla_decode_desc"""
    _fields_ = [("dtype", C.c_int32), ("ql", C.c_int32), ("qh", C.c_int32), ("batch", C.c_int32), ("max_pages", C.c_int32),
                ("page_size", C.c_int32), ("num_pages", C.c_int32), ("splits", C.c_int32), ("flags", C.c_uint32),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32), ("softmax_scale", C.c_float),
                ("q_stride_b", C.c_int64), ("q_stride_h", C.c_int64), ("q_stride_l", C.c_int64),
                ("kv_stride_p", C.c_int64), ("kv_stride_l", C.c_int64), ("table_stride", C.c_int64)]


_vp, _ld = C.c_void_p, C.POINTER(MlaDecodeDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_mla_decode_abi_version": (C.c_int, []),
    "nnop_mla_decode_plan": (C.c_int, [_ld, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "nnop_mla_decode": (C.c_int, [_ld, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "mla-decode-ABI version", "MLA_DECODE_ABI_VERSION", "nnop_mla_decode_abi_version")
