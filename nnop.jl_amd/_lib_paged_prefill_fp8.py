"""ctypes binding of libnnop_hip_paged_prefill_fp8.so (the C ABI of include/nnop_hip_paged_prefill_fp8.h): attention of a prefill step --
a variable number of new tokens per sequence, packed token-major -- over the fourteenth library's paged KV cache of one-byte E4M3 codes
with a scale per KV head, expanded in the registers that stage a tile; the thirteenth library's kernel behind another staging path.

The fifteenth library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``), and so
is the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another paged-prefill-fp8-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_paged_prefill_fp8.so")

# NNOP_HIP_PAGED_PREFILL_FP8_ABI_VERSION of the header this binding was written against; load() refuses another library
PAGED_PREFILL_FP8_ABI_VERSION = 1

BLOCK_ROWS, MAX_GROUP, MIN_PAGE_SIZE = 128, 16, 16     # NNOP_PAGED_PREFILL_FP8_BLOCK_ROWS, _MAX_GROUP, _MIN_PAGE_SIZE
EMBS = (64, 128)
KV_E4M3 = 0                                            # NNOP_PAGED_PREFILL_FP8_E4M3: OCP E4M3, torch.float8_e4m3fn


class PagedPrefillFp8Desc(C.Structure):
    """struct nnop_paged_prefill_fp8_desc"""
    _fields_ = [("dtype", C.c_int32), ("emb", C.c_int32), ("tokens", C.c_int32), ("qh", C.c_int32), ("kh", C.c_int32), ("batch", C.c_int32),
                ("max_pages", C.c_int32), ("window_left", C.c_int32), ("reserved", C.c_int32), ("flags", C.c_uint32),
                ("page_size", C.c_int32), ("num_pages", C.c_int32), ("kv_format", C.c_int32), ("reserved2", C.c_int32),
                ("k_stride_p", C.c_int64), ("k_stride_h", C.c_int64), ("k_stride_l", C.c_int64),
                ("v_stride_p", C.c_int64), ("v_stride_h", C.c_int64), ("v_stride_l", C.c_int64), ("table_stride", C.c_int64),
                ("q_stride_t", C.c_int64), ("q_stride_h", C.c_int64), ("o_stride_t", C.c_int64), ("o_stride_h", C.c_int64)]


_vp, _ld = C.c_void_p, C.POINTER(PagedPrefillFp8Desc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_paged_prefill_fp8_abi_version": (C.c_int, []),
    "nnop_paged_prefill_fp8_plan": (C.c_int, [_ld, C.POINTER(C.c_size_t)]),
    "nnop_paged_prefill_fp8": (C.c_int, [_ld, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "paged-prefill-fp8-ABI version", "PAGED_PREFILL_FP8_ABI_VERSION",
                        "nnop_paged_prefill_fp8_abi_version")
