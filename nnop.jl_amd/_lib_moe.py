"""ctypes binding of libnnop_hip_moe.so (the C ABI of include/nnop_hip_moe.h): mixture-of-experts routing.

The third library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``), and so is
the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another moe-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_moe.so")

# NNOP_HIP_MOE_ABI_VERSION of the header this binding was written against; load() refuses another library
MOE_ABI_VERSION = 1

# enum nnop_moe_norm
NNOP_MOE_NORM_TOPK, NNOP_MOE_NORM_ALL = 0, 1
NORMS = {"topk": NNOP_MOE_NORM_TOPK, "all": NNOP_MOE_NORM_ALL}
MAX_EXPERTS, MAX_TOPK = 1024, 16


class MoeRouterDesc(C.Structure):
    """struct nnop_moe_router_desc"""
    _fields_ = [("dtype", C.c_int32), ("tokens", C.c_int32), ("experts", C.c_int32), ("topk", C.c_int32), ("ld", C.c_int32),
                ("norm", C.c_int32), ("reserved", C.c_int32 * 2)]


class MoePlanDesc(C.Structure):
    """struct nnop_moe_plan_desc"""
    _fields_ = [("tokens", C.c_int32), ("topk", C.c_int32), ("experts", C.c_int32), ("reserved", C.c_int32 * 1)]


_vp, _rd, _pd = C.c_void_p, C.POINTER(MoeRouterDesc), C.POINTER(MoePlanDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_moe_abi_version": (C.c_int, []),
    "nnop_moe_router": (C.c_int, [_rd, _vp, _vp, _vp, _vp, _vp]),
    "nnop_moe_router_bwd": (C.c_int, [_rd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nnop_moe_plan_workspace_bytes": (C.c_size_t, [_pd]),
    "nnop_moe_plan": (C.c_int, [_pd, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "moe-ABI version", "MOE_ABI_VERSION", "nnop_moe_abi_version")
