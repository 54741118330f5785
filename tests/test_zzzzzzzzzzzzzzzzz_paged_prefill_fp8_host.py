"""CPU tests of the C boundary and wrappers of prefill attention over a paged FP8 KV cache (include/nnop_hip_paged_prefill_fp8.h): the
fifteenth library exports exactly its header's three functions and links none of the other fourteen, its descriptor matches the ctypes
one, the entry points validate in the header's order and return before any launch, and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_paged_prefill_fp8.h")
NAMES = {"nnop_paged_prefill_fp8_abi_version", "nnop_paged_prefill_fp8_plan", "nnop_paged_prefill_fp8"}
FIELDS = ["dtype", "emb", "tokens", "qh", "kh", "batch", "max_pages", "window_left", "reserved", "flags", "page_size", "num_pages", "kv_format",
          "reserved2", "k_stride_p", "k_stride_h", "k_stride_l", "v_stride_p", "v_stride_h", "v_stride_l", "table_stride",
          "q_stride_t", "q_stride_h", "o_stride_t", "o_stride_h"]
# o lse q k v k_scale v_scale block_table cu_seqlens_q seqlens sinks workspace; lse, the scales, sinks and the workspace are optional
ALIGNS, OPTIONAL = (16, 4, 16, 16, 16, 4, 4, 4, 4, 4, 4, 4), (1, 5, 6, 10, 11)
OK, NULL = C.c_void_p(0x7f0000001000), C.c_void_p(0)         # never dereferenced: every call in this file returns before a launch
at = lambda off: C.c_void_p(0x7f0000001000 + off)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_paged_prefill_fp8
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_paged_prefill_fp8.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_paged_prefill_fp8_abi_version() == M.PAGED_PREFILL_FP8_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_paged_prefill_fp8_desc \{(.*?)\} nnop_paged_prefill_fp8_desc;", header, re.S).group(1)
    names = [re.match(r"\w+", n.strip()).group(0) for _, ns in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body) for n in ns.split(",")]
    D, D13 = M.PagedPrefillFp8Desc, pkg._lib_paged_prefill.PagedPrefillDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == 144 == C.sizeof(D13) + 8
    # the thirteenth library's fields in its order, kv_format and reserved2 between num_pages and the strides
    assert [n for n in FIELDS if n not in ("kv_format", "reserved2")] == [n for n, _ in D13._fields_]
    assert all(getattr(D, n).offset == 4 * i for i, n in enumerate(FIELDS[:14])) and all(getattr(D, n).offset == 56 + 8 * i for i, n in enumerate(FIELDS[14:]))
    want = tuple(int(re.search(rf"#define NNOP_PAGED_PREFILL_FP8_{n}\s+(\d+)", header).group(1)) for n in ("BLOCK_ROWS", "MAX_GROUP", "MIN_PAGE_SIZE", "E4M3"))
    assert (M.BLOCK_ROWS, M.MAX_GROUP, M.MIN_PAGE_SIZE, M.KV_E4M3) == want
    for name in ("paged_prefill_attention_fp8", "paged_prefill_attention_fp8_into", "paged_prefill_attention_fp8_plan", "paged_prefill_fp8",
                 "_lib_paged_prefill_fp8"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.paged_prefill_fp8._ptr is pkg._common._ptr and pkg.paged_prefill_fp8._raise is pkg._common._raise


def _kw(**kw):
    base = dict(dtype=2, emb=64, tokens=1000, qh=64, kh=8, batch=4, max_pages=256, window_left=-1, reserved=0, flags=0, page_size=16,
                num_pages=1024, kv_format=0, reserved2=0, table_stride=256, q_stride_t=64 * 64, q_stride_h=64, o_stride_t=64 * 64, o_stride_h=64)
    base.update({f"{t}_stride_{a}": s for t in "kv" for a, s in (("p", 8 * 16 * 64), ("h", 16 * 64), ("l", 64))})
    base.update(kw)
    return base


def _call(lib, d, ptrs, nbytes=0):
    return lib.nnop_paged_prefill_fp8(C.byref(d), *ptrs, nbytes, None)


def _plan(lib, d):
    n = C.c_size_t(1)
    return lib.nnop_paged_prefill_fp8_plan(C.byref(d), C.byref(n)), n.value


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # no fp32
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(kv_format=1), "NNOP_ERR_OPTS"),                            # no E5M2
    (dict(reserved=3), "NNOP_ERR_OPTS"),
    (dict(reserved2=1), "NNOP_ERR_OPTS"),
    (dict(window_left=-2), "NNOP_ERR_OPTS"),
    (dict(emb=32), "NNOP_ERR_SHAPE"),
    (dict(tokens=0), "NNOP_ERR_SHAPE"),
    (dict(qh=136, q_stride_t=136 * 64, o_stride_t=136 * 64), "NNOP_ERR_SHAPE"),   # G = 17
    (dict(qh=60), "NNOP_ERR_SHAPE"),                                 # no multiple of KH
    (dict(page_size=8), "NNOP_ERR_SHAPE"),                           # a 16-key block would span two pages
    (dict(page_size=48), "NNOP_ERR_SHAPE"),                          # no power of two
    (dict(num_pages=0), "NNOP_ERR_SHAPE"),
    (dict(max_pages=0), "NNOP_ERR_SHAPE"),
    (dict(max_pages=2 ** 27), "NNOP_ERR_SHAPE"),                     # 2^31 keys
    (dict(k_stride_l=48), "NNOP_ERR_SHAPE"),                         # below a row
    (dict(v_stride_p=8 * 16 * 64 + 8), "NNOP_ERR_SHAPE"),            # no multiple of 16 bytes
    (dict(q_stride_t=64 * 64 - 8), "NNOP_ERR_SHAPE"),                # tokens of q overlap
    (dict(o_stride_h=68), "NNOP_ERR_SHAPE"),                         # no multiple of 8 elements
    (dict(table_stride=255), "NNOP_ERR_SHAPE"),                      # below max_pages
    (dict(batch=2 ** 29), "NNOP_ERR_SHAPE"),                         # 2^32 workgroups
    (dict(tokens=2 ** 26), "NNOP_ERR_SHAPE"),                        # 2^32 rows of lse
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, kv_format=1, page_size=8), "NNOP_ERR_DTYPE"),
    (dict(kv_format=1, page_size=8), "NNOP_ERR_OPTS"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    M, want = pkg._lib_paged_prefill_fp8, getattr(pkg._lib, status)
    lib, d = M.load(), M.PagedPrefillFp8Desc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 12) == want
    assert _plan(lib, d) == (want, 1)
    assert lib.nnop_paged_prefill_fp8(None, *[OK] * 12, 0, None) == pkg._lib.NNOP_ERR_NULL == lib.nnop_paged_prefill_fp8_plan(C.byref(d), None)


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_paged_prefill_fp8, pkg._lib
    lib, d = M.load(), M.PagedPrefillFp8Desc(**_kw())
    assert _plan(lib, d) == (L.NNOP_OK, 0)                           # the block of a workgroup is searched, not listed
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 12, [at(1)] * 12                               # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos in OPTIONAL else L.NNOP_ERR_NULL), pos
        if pos not in OPTIONAL:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 12
        c[pos] = at(a // 2)                                          # aligned to half of what is needed: a scale at 2 bytes among them
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    i32, bf = dict(dt=torch.int32), dict(dt=torch.bfloat16)
    q, k, v, tab = mk(7, 16, 64, **bf), mk(9, 2, 16, 64, dt=torch.float8_e4m3fn), mk(9, 2, 16, 64), mk(2, 3, **i32)
    cu, lens = mk(3, **i32), mk(2, **i32)
    A, E = pkg.paged_prefill_attention_fp8, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        A(q, k, v, torch.zeros(2, 3, dtype=torch.int32), cu, lens)
    with pytest.raises(E, match="paged_prefill_attention takes 16-bit pages") as e:      # a 16-bit pool belongs to the thirteenth library
        A(q, mk(9, 2, 16, 64, **bf), mk(9, 2, 16, 64, **bf), tab, cu, lens)
    assert e.value.status == pkg._lib.NNOP_ERR_DTYPE
    for bad, status in ((lambda: A(q, mk(9, 2, 16, 64, dt=torch.float8_e5m2), v, tab, cu, lens), "NNOP_ERR_DTYPE"),   # a wrong pool dtype
                        (lambda: A(mk(7, 16, 64, dt=torch.float32), k, v, tab, cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, k, v, mk(2, 3, dt=torch.int64), cu, lens), "NNOP_ERR_DTYPE"),              # the table's dtype
                        (lambda: A(mk(1, 7, 16, 64, **bf), k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),              # rank: decode's q
                        (lambda: A(q, mk(9, 2, 8, 64), mk(9, 2, 8, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),       # page sizes 8 and 48
                        (lambda: A(q, mk(9, 2, 48, 64), mk(9, 2, 48, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, mk(9, 2, 16, 72)[..., :64], v, tab, cu, lens), "NNOP_ERR_SHAPE"),          # a row stride of 72 bytes: no multiple of 16
                        (lambda: A(mk(7, 16, 68, **bf)[..., :64], k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),       # a head stride of 68 elements
                        (lambda: A(mk(7, 34, 64, **bf), k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),                 # G = 17
                        (lambda: A(q, k, v, tab, cu, lens, k_scale=mk(3, dt=torch.float32)), "NNOP_ERR_SHAPE"),  # a scale per KV head
                        (lambda: A(q, k, v, tab, cu, lens, v_scale=mk(2, **bf)), "NNOP_ERR_SHAPE"),              # ... in float32
                        (lambda: A(q, k, v, tab, mk(2, **i32), lens), "NNOP_ERR_SHAPE"),                         # cu_seqlens_q is [B + 1]
                        (lambda: pkg.paged_prefill_attention_fp8_into(mk(7, 16, 64, dt=torch.float16), None, q, k, v, tab, cu, lens), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    with pytest.raises(ValueError):
        A(q, k, v, tab, cu, lens, window_left=-1)
    # both pool layouts become byte strides, a slice of a larger table and a q inside a fused projection element strides, never a copy
    d = pkg.paged_prefill_fp8._desc(mk(7, 48, 64, **bf)[:, :16], mk(9, 16, 2, 64).transpose(1, 2), v, mk(2, 8, **i32)[:, 2:5], 128, mk(7, 16, 64, **bf))
    assert (d.k_stride_p, d.k_stride_h, d.k_stride_l, d.v_stride_p, d.v_stride_h, d.v_stride_l, d.table_stride) == (2048, 64, 128, 2048, 1024, 64, 8)
    assert (d.q_stride_t, d.q_stride_h, d.o_stride_t, d.o_stride_h, d.tokens, d.batch) == (48 * 64, 64, 16 * 64, 64, 7, 2)
    assert (d.window_left, d.max_pages, d.page_size, d.num_pages, d.qh, d.kh, d.kv_format, d.reserved2) == (48, 3, 16, 9, 16, 2, 0, 0)
    assert pkg.paged_prefill_attention_fp8_plan(q, k, v, tab) == 0 == pkg.paged_prefill_attention_fp8_plan(q[:0], k, v, tab, window_left=5)
