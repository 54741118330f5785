"""ctypes binding of libnnop_hip_moe_mx_decode_glu.so (the C ABI of include/nnop_hip_moe_mx_decode_glu.h): the weight-streaming forward
on MXFP4 weights of a fused gate-up projection with the gated activation in its epilogue and, optionally, the token gather in front.

The ninth library has an ABI version of its own; dtypes, status codes, activation codes and their messages are the main library's
(``_lib``), and so is the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another moe-mx-decode-glu-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_moe_mx_decode_glu.so")

# NNOP_HIP_MOE_MX_DECODE_GLU_ABI_VERSION of the header this binding was written against; load() refuses another library
MOE_MX_DECODE_GLU_ABI_VERSION = 1

MAX_EXPERTS, MAX_IN, MAX_INTER, MAX_TOPK = 1024, 65536, 32768, 64
BLOCK = 32                                    # elements that share a scale byte
LAYOUTS = {"interleaved": 0, "halves": 1}     # NNOP_MOE_GLU_INTERLEAVED, NNOP_MOE_GLU_HALVES


class MoeMxDecodeGluDesc(C.Structure):
    """struct nnop_moe_mx_decode_glu_desc"""
    _fields_ = [("dtype", C.c_int32), ("rows", C.c_int32), ("experts", C.c_int32), ("in_dim", C.c_int32), ("inter_dim", C.c_int32),
                ("ld_x", C.c_int32), ("ld_h", C.c_int32), ("ld_b", C.c_int32), ("ld_q", C.c_int32), ("ld_s", C.c_int32),
                ("act", C.c_int32), ("layout", C.c_int32), ("tokens", C.c_int32), ("topk", C.c_int32),
                ("alpha", C.c_float), ("limit", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_int32 * 3)]


_vp, _ld = C.c_void_p, C.POINTER(MoeMxDecodeGluDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_moe_mx_decode_glu_abi_version": (C.c_int, []),
    "nnop_moe_mx_decode_glu": (C.c_int, [_ld, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "moe-mx-decode-glu-ABI version", "MOE_MX_DECODE_GLU_ABI_VERSION",
                        "nnop_moe_mx_decode_glu_abi_version")
