"""ctypes binding of libnnop_hip_moe_data.so (the C ABI of include/nnop_hip_moe_data.h): the MoE token permute and weighted combine.

The fourth library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``), and so is
the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another moe-data-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_moe_data.so")

# NNOP_HIP_MOE_DATA_ABI_VERSION of the header this binding was written against; load() refuses another library
MOE_DATA_ABI_VERSION = 1

MAX_TOPK, MAX_DIM = 64, 65536


class MoeRowsDesc(C.Structure):
    """struct nnop_moe_rows_desc"""
    _fields_ = [("dtype", C.c_int32), ("tokens", C.c_int32), ("topk", C.c_int32), ("dim", C.c_int32), ("ld_tok", C.c_int32),
                ("ld_slot", C.c_int32), ("reserved", C.c_int32 * 2)]


_vp, _rd = C.c_void_p, C.POINTER(MoeRowsDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_moe_data_abi_version": (C.c_int, []),
    "nnop_moe_permute": (C.c_int, [_rd, _vp, _vp, _vp, _vp]),
    "nnop_moe_permute_bwd": (C.c_int, [_rd, _vp, _vp, _vp, _vp]),
    "nnop_moe_combine": (C.c_int, [_rd, _vp, _vp, _vp, _vp, _vp]),
    "nnop_moe_combine_bwd": (C.c_int, [_rd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "moe-data-ABI version", "MOE_DATA_ABI_VERSION", "nnop_moe_data_abi_version")
