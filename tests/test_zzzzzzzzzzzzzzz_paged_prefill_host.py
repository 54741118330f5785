"""CPU tests of the C boundary and wrappers of prefill attention over a paged KV cache (include/nnop_hip_paged_prefill.h): the thirteenth
library exports exactly its header's three functions and links none of the other twelve, its descriptor matches the ctypes one, the
entry points validate in the header's order and return before any launch, the plan reports the documented 0 bytes after the same
checks, and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_paged_prefill.h")
NAMES = {"nnop_paged_prefill_abi_version", "nnop_paged_prefill_plan", "nnop_paged_prefill"}
FIELDS = ["dtype", "emb", "tokens", "qh", "kh", "batch", "max_pages", "window_left", "reserved", "flags", "page_size", "num_pages",
          "k_stride_p", "k_stride_h", "k_stride_l", "v_stride_p", "v_stride_h", "v_stride_l", "table_stride",
          "q_stride_t", "q_stride_h", "o_stride_t", "o_stride_h"]
# o lse q k v block_table cu_seqlens_q seqlens sinks workspace; lse, sinks and the workspace are optional
ALIGNS, OPTIONAL = (16, 4, 16, 16, 16, 4, 4, 4, 4, 4), (1, 8, 9)
OK, NULL = C.c_void_p(0x7f0000001000), C.c_void_p(0)         # never dereferenced: every call in this file returns before a launch
at = lambda off: C.c_void_p(0x7f0000001000 + off)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_paged_prefill
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_paged_prefill.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_paged_prefill_abi_version() == M.PAGED_PREFILL_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_paged_prefill_desc \{(.*?)\} nnop_paged_prefill_desc;", header, re.S).group(1)
    names = [re.match(r"\w+", n.strip()).group(0) for _, ns in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body) for n in ns.split(",")]
    D = M.PagedPrefillDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == 136
    assert all(getattr(D, n).offset == 4 * i for i, n in enumerate(FIELDS[:12])) and all(getattr(D, n).offset == 48 + 8 * i for i, n in enumerate(FIELDS[12:]))
    assert (M.BLOCK_ROWS, M.MAX_GROUP, M.MIN_PAGE_SIZE) == tuple(int(re.search(rf"#define NNOP_PAGED_PREFILL_{n}\s+(\d+)", header).group(1))
                                                                 for n in ("BLOCK_ROWS", "MAX_GROUP", "MIN_PAGE_SIZE"))
    for name in ("paged_prefill_attention", "paged_prefill_attention_into", "paged_prefill_attention_plan", "paged_prefill", "_lib_paged_prefill"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.paged_prefill._ptr is pkg._common._ptr and pkg.paged_prefill._raise is pkg._common._raise


def _kw(**kw):
    base = dict(dtype=2, emb=64, tokens=1000, qh=64, kh=8, batch=4, max_pages=256, window_left=-1, reserved=0, flags=0, page_size=16,
                num_pages=1024, table_stride=256, q_stride_t=64 * 64, q_stride_h=64, o_stride_t=64 * 64, o_stride_h=64)
    base.update({f"{t}_stride_{a}": s for t in "kv" for a, s in (("p", 8 * 16 * 64), ("h", 16 * 64), ("l", 64))})
    base.update(kw)
    return base


def _call(lib, d, ptrs, nbytes=0):
    return lib.nnop_paged_prefill(C.byref(d), *ptrs, nbytes, None)


def _plan(lib, d):
    n = C.c_size_t(1)
    return lib.nnop_paged_prefill_plan(C.byref(d), C.byref(n)), n.value


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # no fp32
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(reserved=3), "NNOP_ERR_OPTS"),                             # where the decode descriptor keeps its split count
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
    (dict(k_stride_l=24), "NNOP_ERR_SHAPE"),                         # below a row
    (dict(v_stride_p=8 * 16 * 64 + 4), "NNOP_ERR_SHAPE"),            # no multiple of 8
    (dict(q_stride_t=64 * 64 - 8), "NNOP_ERR_SHAPE"),                # tokens of q overlap
    (dict(o_stride_h=68), "NNOP_ERR_SHAPE"),
    (dict(table_stride=255), "NNOP_ERR_SHAPE"),                      # below max_pages
    (dict(batch=2 ** 29), "NNOP_ERR_SHAPE"),                         # 2^32 workgroups
    (dict(tokens=2 ** 26), "NNOP_ERR_SHAPE"),                        # 2^32 rows of lse
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, flags=1, page_size=8), "NNOP_ERR_DTYPE"),
    (dict(flags=1, page_size=8), "NNOP_ERR_OPTS"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    M, want = pkg._lib_paged_prefill, getattr(pkg._lib, status)
    lib, d = M.load(), M.PagedPrefillDesc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 10) == want
    assert _plan(lib, d) == (want, 1)
    assert lib.nnop_paged_prefill(None, *[OK] * 10, 0, None) == pkg._lib.NNOP_ERR_NULL == lib.nnop_paged_prefill_plan(C.byref(d), None)


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_paged_prefill, pkg._lib
    lib, d = M.load(), M.PagedPrefillDesc(**_kw())
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 10, [at(1)] * 10                               # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos in OPTIONAL else L.NNOP_ERR_NULL), pos
        if pos not in OPTIONAL:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 10
        c[pos] = at(a // 2)                                          # aligned to half of what is needed
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos


@pytest.mark.parametrize("kw", [dict(), dict(batch=1, tokens=1), dict(emb=128, qh=8, kh=8, tokens=2 ** 20, **{f"{t}_stride_{a}": 8 * 128 for t in "qo" for a in "th"},
                                                                      **{f"{t}_stride_{a}": 128 for t in "kv" for a in "phl"}),
                                dict(window_left=7, page_size=128), dict(qh=40, kh=8, batch=2 ** 20)])
def test_the_plan_reports_no_workspace(pkg, kw):
    M = pkg._lib_paged_prefill
    assert _plan(M.load(), M.PagedPrefillDesc(**_kw(**kw))) == (pkg._lib.NNOP_OK, 0)      # the block of a workgroup is searched, not listed


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    q, k, v, tab = mk(7, 16, 64), mk(9, 2, 16, 64), mk(9, 2, 16, 64), mk(2, 3, dt=torch.int32)
    cu, lens = mk(3, dt=torch.int32), mk(2, dt=torch.int32)
    A, E = pkg.paged_prefill_attention, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        A(q, k, v, torch.zeros(2, 3, dtype=torch.int32), cu, lens)
    with pytest.raises(E, match="flash_attention"):
        A(mk(7, 16, 64, dt=torch.float32).requires_grad_(True).to(torch.bfloat16).as_subclass(OnGpu), k, v, tab, cu, lens)
    for bad, status in ((lambda: A(q, mk(9, 2, 16, 64, dt=torch.float16), v, tab, cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(mk(7, 16, 64, dt=torch.float32), k, v, tab, cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, k, v, mk(2, 3, dt=torch.int64), cu, lens), "NNOP_ERR_DTYPE"),       # the table's dtype
                        (lambda: A(mk(1, 7, 16, 64), k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),             # rank: decode's q
                        (lambda: A(q, k, v, tab[0], cu, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, mk(9, 2, 8, 64), mk(9, 2, 8, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),  # page sizes 8 and 48
                        (lambda: A(q, mk(9, 2, 48, 64), mk(9, 2, 48, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, mk(2, 6, dt=torch.int32)[:, ::2], cu, lens), "NNOP_ERR_SHAPE"),  # a table with a last stride of 2
                        (lambda: A(q, mk(9, 2, 16, 68)[..., :64], v, tab, cu, lens), "NNOP_ERR_SHAPE"),   # a row stride of 68: no multiple of 8
                        (lambda: A(mk(7, 16, 68)[..., :64], k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),      # the same of q
                        (lambda: A(mk(7, 34, 64), k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),                # G = 17
                        (lambda: A(q, k, v, tab, mk(2, dt=torch.int32), lens), "NNOP_ERR_SHAPE"),         # cu_seqlens_q is [B + 1]
                        (lambda: A(q, k, v, tab, cu, mk(3, dt=torch.int32)), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, tab, cu.long().as_subclass(OnGpu), lens), "NNOP_ERR_SHAPE"),
                        (lambda: pkg.paged_prefill_attention_into(mk(7, 16, 64, dt=torch.float16), None, q, k, v, tab, cu, lens), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    with pytest.raises(ValueError):
        A(q, k, v, tab, cu, lens, window_left=-1)
    # both pool layouts, a slice of a larger table and a q inside a fused projection become strides, never a copy; the plan needs no device
    d = pkg.paged_prefill._desc(mk(7, 48, 64)[:, :16], mk(9, 16, 2, 64).transpose(1, 2), v, mk(2, 8, dt=torch.int32)[:, 2:5], 128, mk(7, 16, 64))
    assert (d.k_stride_p, d.k_stride_h, d.k_stride_l, d.v_stride_p, d.v_stride_h, d.v_stride_l, d.table_stride) == (2048, 64, 128, 2048, 1024, 64, 8)
    assert (d.q_stride_t, d.q_stride_h, d.o_stride_t, d.o_stride_h, d.tokens, d.batch) == (48 * 64, 64, 16 * 64, 64, 7, 2)
    assert (d.window_left, d.max_pages, d.page_size, d.num_pages, d.qh, d.kh) == (48, 3, 16, 9, 16, 2)
    assert pkg.paged_prefill_attention_plan(q, k, v, tab) == 0 == pkg.paged_prefill_attention_plan(q[:0], k, v, tab, window_left=5)
