"""ctypes binding of libnnop_hip_paged_prefill_split.so (the C ABI of include/nnop_hip_paged_prefill_split.h): the thirteenth library's
prefill attention over a paged KV cache with every block's key range cut into chunks and a merge kernel behind them.

The sixteenth library has an ABI version of its own and takes the thirteenth's descriptor (``_lib_paged_prefill.PagedPrefillDesc``) with
``reserved`` read as the split count; dtypes, status codes and their messages are the main library's (``_lib``), and so is the load
sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library
from ._lib_paged_prefill import PagedPrefillDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_paged_prefill_split.so")

# NNOP_HIP_PAGED_PREFILL_SPLIT_ABI_VERSION of the header this binding was written against; load() refuses another library
PAGED_PREFILL_SPLIT_ABI_VERSION = 1

MAX_SPLITS, MIN_CHUNK_TILES = 64, 8                    # NNOP_PAGED_PREFILL_SPLIT_MAX_SPLITS, _MIN_CHUNK_TILES

_vp, _ld = C.c_void_p, C.POINTER(PagedPrefillDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_paged_prefill_split_abi_version": (C.c_int, []),
    "nnop_paged_prefill_split_plan": (C.c_int, [_ld, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "nnop_paged_prefill_split": (C.c_int, [_ld, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "paged-prefill-split-ABI version", "PAGED_PREFILL_SPLIT_ABI_VERSION",
                        "nnop_paged_prefill_split_abi_version")
