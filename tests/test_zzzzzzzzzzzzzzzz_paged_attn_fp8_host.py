"""CPU tests of the C boundary and wrappers of decode attention over a paged FP8 KV cache (include/nnop_hip_paged_attn_fp8.h): the
fourteenth library exports exactly its header's three functions and links none of the other thirteen, its descriptor matches the ctypes
one, the entry points validate in the header's order and return before any launch, the plan is the eleventh library's at a capacity of
max_pages page_size, and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_paged_attn_fp8.h")
NAMES = {"nnop_paged_attn_fp8_abi_version", "nnop_paged_attn_fp8_plan", "nnop_paged_attn_fp8"}
FIELDS = ["dtype", "emb", "ql", "qh", "kh", "batch", "max_pages", "window_left", "splits", "flags", "page_size", "num_pages", "kv_format",
          "reserved", "k_stride_p", "k_stride_h", "k_stride_l", "v_stride_p", "v_stride_h", "v_stride_l", "table_stride"]
# o lse q k v k_scale v_scale block_table seqlens sinks workspace; the workspace is optional at one split
ALIGNS, OPTIONAL = (16, 4, 16, 16, 16, 4, 4, 4, 4, 4, 4), (1, 5, 6, 9, 10)
OK, NULL = C.c_void_p(0x7f0000001000), C.c_void_p(0)         # never dereferenced: every call in this file returns before a launch
at = lambda off: C.c_void_p(0x7f0000001000 + off)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_paged_attn_fp8
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_paged_attn_fp8.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_paged_attn_fp8_abi_version() == M.PAGED_ATTN_FP8_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_paged_attn_fp8_desc \{(.*?)\} nnop_paged_attn_fp8_desc;", header, re.S).group(1)
    names = [re.match(r"\w+", n.strip()).group(0) for _, ns in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body) for n in ns.split(",")]
    D, D12 = M.PagedAttnFp8Desc, pkg._lib_paged_attn.PagedAttnDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == 112 == C.sizeof(D12) + 8
    # the twelfth library's fields in its order, kv_format and reserved between num_pages and the strides
    assert [n for n in FIELDS if n not in ("kv_format", "reserved")] == [n for n, _ in D12._fields_]
    assert all(getattr(D, n).offset == 4 * i for i, n in enumerate(FIELDS[:14])) and all(getattr(D, n).offset == 56 + 8 * i for i, n in enumerate(FIELDS[14:]))
    want = tuple(int(re.search(rf"#define NNOP_PAGED_ATTN_FP8_{n}\s+(\d+)", header).group(1)) for n in ("MAX_ROWS", "MAX_SPLITS", "MIN_PAGE_SIZE", "E4M3"))
    assert (M.MAX_ROWS, M.MAX_SPLITS, M.MIN_PAGE_SIZE, M.KV_E4M3) == want
    for name in ("paged_decode_attention_fp8", "paged_decode_attention_fp8_into", "paged_decode_attention_fp8_plan", "paged_attn_fp8", "_lib_paged_attn_fp8"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.paged_attn_fp8._ptr is pkg._common._ptr and pkg.paged_attn_fp8._raise is pkg._common._raise


def _kw(**kw):
    base = dict(dtype=2, emb=64, ql=1, qh=64, kh=8, batch=4, max_pages=256, window_left=-1, splits=0, flags=0, page_size=16, num_pages=1024,
                kv_format=0, reserved=0, table_stride=256)
    base.update({f"{t}_stride_{a}": s for t in "kv" for a, s in (("p", 8 * 16 * 64), ("h", 16 * 64), ("l", 64))})
    base.update(kw)
    return base


def _call(lib, d, ptrs, nbytes=1 << 40):
    return lib.nnop_paged_attn_fp8(C.byref(d), *ptrs, nbytes, None)


def _plan(lib, fn, d):
    s, n = C.c_int32(-1), C.c_size_t(1)
    st = getattr(lib, fn)(C.byref(d), C.byref(s), C.byref(n))
    return st, s.value, n.value


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # no fp32
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(kv_format=1), "NNOP_ERR_OPTS"),                            # no E5M2
    (dict(reserved=1), "NNOP_ERR_OPTS"),
    (dict(window_left=-2), "NNOP_ERR_OPTS"),
    (dict(splits=65), "NNOP_ERR_OPTS"),
    (dict(emb=32), "NNOP_ERR_SHAPE"),
    (dict(qh=136), "NNOP_ERR_SHAPE"),                                # G = 17
    (dict(ql=3), "NNOP_ERR_SHAPE"),                                  # G QL = 24
    (dict(page_size=8), "NNOP_ERR_SHAPE"),                           # a 16-key block would span two pages
    (dict(page_size=48), "NNOP_ERR_SHAPE"),                          # no power of two
    (dict(page_size=0), "NNOP_ERR_SHAPE"),
    (dict(num_pages=0), "NNOP_ERR_SHAPE"),
    (dict(max_pages=0), "NNOP_ERR_SHAPE"),
    (dict(max_pages=2 ** 27), "NNOP_ERR_SHAPE"),                     # 2^31 keys
    (dict(k_stride_l=48), "NNOP_ERR_SHAPE"),                         # below a row
    (dict(v_stride_p=8 * 16 * 64 + 8), "NNOP_ERR_SHAPE"),            # no multiple of 16 bytes
    (dict(v_stride_l=2 ** 32 // 15 - 1), "NNOP_ERR_SHAPE"),          # a multiple of 16; the page's last row ends 2^32 + 48 bytes in
    (dict(table_stride=255), "NNOP_ERR_SHAPE"),                      # below max_pages
    (dict(batch=2 ** 26, splits=8), "NNOP_ERR_SHAPE"),               # 2^32 workgroups
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, kv_format=1, page_size=8), "NNOP_ERR_DTYPE"),
    (dict(kv_format=1, page_size=8), "NNOP_ERR_OPTS"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    M, want = pkg._lib_paged_attn_fp8, getattr(pkg._lib, status)
    lib, d = M.load(), M.PagedAttnFp8Desc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 11) == want
    assert _plan(lib, "nnop_paged_attn_fp8_plan", d)[0] == want
    assert lib.nnop_paged_attn_fp8(None, *[OK] * 11, 0, None) == pkg._lib.NNOP_ERR_NULL == lib.nnop_paged_attn_fp8_plan(C.byref(d), None, None)


def test_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_paged_attn_fp8, pkg._lib
    lib, d = M.load(), M.PagedAttnFp8Desc(**_kw(splits=4))           # a workspace is needed, so every pointer is judged
    need = _plan(lib, "nnop_paged_attn_fp8_plan", d)[2]
    assert need == 4 * 4 * 64 * 1 * 4 * 66
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 11, [at(1)] * 11                               # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos in OPTIONAL[:4] else L.NNOP_ERR_NULL), pos
        if pos not in OPTIONAL[:4]:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 11
        c[pos] = at(a // 2)                                          # aligned to half of what is needed: a scale at 2 bytes among them
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos
    assert _call(lib, d, [OK] * 11, need - 1) == L.NNOP_ERR_WORKSPACE
    one = M.PagedAttnFp8Desc(**_kw(splits=1))                        # one split: a NULL workspace of 0 bytes passes on to the alignment check
    assert _call(lib, one, [at(1)] * 10 + [NULL], 0) == L.NNOP_ERR_ALIGN and _call(lib, one, [NULL] * 11, 0) == L.NNOP_ERR_NULL
    # the largest row stride a page of 16 may have is judged a shape that passes: the next check, the pointers, answers
    assert _call(lib, M.PagedAttnFp8Desc(**_kw(k_stride_l=2 ** 32 // 15 - 17)), [NULL] * 11, 0) == L.NNOP_ERR_NULL


@pytest.mark.parametrize("kw", [dict(batch=1, max_pages=4096), dict(batch=8, max_pages=64, page_size=128), dict(batch=64), dict(batch=1, max_pages=19),
                                dict(batch=1, max_pages=4096, window_left=128), dict(batch=1, max_pages=7, splits=7),
                                dict(batch=1, emb=128, splits=2, k_stride_l=128, v_stride_l=128), dict(qh=8, ql=2, window_left=1000, page_size=32)])
def test_the_plan_is_the_eleventh_librarys_at_max_pages_times_page_size(pkg, kw):
    MP, M8 = pkg._lib_paged_attn_fp8, pkg._lib_decode_attn_fp8
    d = MP.PagedAttnFp8Desc(**_kw(table_stride=kw.get("max_pages", 256), **kw))
    dense = M8.DecodeAttnFp8Desc(**{n: getattr(d, n) for n in ("dtype", "emb", "ql", "qh", "kh", "batch", "window_left", "splits")},
                                 capacity=d.max_pages * d.page_size, **{f"{t}_stride_{a}": d.emb for t in "kv" for a in "bhl"})
    got = _plan(MP.load(), "nnop_paged_attn_fp8_plan", d)
    assert got[0] == pkg._lib.NNOP_OK and got == _plan(M8.load(), "nnop_decode_attn_fp8_plan", dense)


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    i32, bf = dict(dt=torch.int32), dict(dt=torch.bfloat16)
    q, k, v, tab, lens = mk(2, 16, 1, 64, **bf), mk(9, 2, 16, 64, dt=torch.float8_e4m3fn), mk(9, 2, 16, 64), mk(2, 3, **i32), mk(2, **i32)
    A, E = pkg.paged_decode_attention_fp8, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        A(q, k, v, torch.zeros(2, 3, dtype=torch.int32), lens)
    with pytest.raises(E, match="paged_decode_attention takes 16-bit pages") as e:       # a 16-bit pool belongs to the twelfth library
        A(q, mk(9, 2, 16, 64, **bf), mk(9, 2, 16, 64, **bf), tab, lens)
    assert e.value.status == pkg._lib.NNOP_ERR_DTYPE
    for bad, status in ((lambda: A(q, mk(9, 2, 16, 64, dt=torch.float8_e5m2), v, tab, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(mk(2, 16, 1, 64, dt=torch.float32), k, v, tab, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, k, v, mk(2, 3, dt=torch.int64), lens), "NNOP_ERR_DTYPE"),         # the table's dtype
                        (lambda: A(q, k[0], v[0], tab, lens), "NNOP_ERR_SHAPE"),                        # rank
                        (lambda: A(q, k, v, tab[0], lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, mk(9, 2, 8, 64), mk(9, 2, 8, 64), tab, lens), "NNOP_ERR_SHAPE"),  # page sizes 8 and 48
                        (lambda: A(q, mk(9, 2, 48, 64), mk(9, 2, 48, 64), tab, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, mk(2, 6, **i32)[:, ::2], lens), "NNOP_ERR_SHAPE"),          # a table with a last stride of 2
                        (lambda: A(q, k, v, mk(3, 2, **i32).t(), lens), "NNOP_ERR_SHAPE"),              # a row stride below max_pages
                        (lambda: A(q, mk(9, 2, 16, 72)[..., :64], v, tab, lens), "NNOP_ERR_SHAPE"),     # a row stride of 72 bytes: no multiple of 16
                        (lambda: A(mk(2, 34, 1, 64, **bf), k, v, tab, lens), "NNOP_ERR_SHAPE"),         # G = 17
                        (lambda: A(q, k, v, mk(3, 3, **i32), lens), "NNOP_ERR_SHAPE"),                  # a table of another batch
                        (lambda: A(q, k, v, tab, lens, k_scale=mk(3, dt=torch.float32)), "NNOP_ERR_SHAPE"),  # a scale per KV head
                        (lambda: A(q, k, v, tab, mk(3, **i32)), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    with pytest.raises(ValueError):
        A(q, k, v, tab, lens, num_splits=65)
    # both pool layouts and a slice of a larger table become byte strides, never a copy; K and V may differ; the plan needs no device
    d = pkg.paged_attn_fp8._desc(q, mk(9, 16, 2, 64).transpose(1, 2), v, mk(2, 8, **i32)[:, 2:5], 128, 3)
    assert (d.k_stride_p, d.k_stride_h, d.k_stride_l, d.v_stride_p, d.v_stride_h, d.v_stride_l, d.table_stride) == (2048, 64, 128, 2048, 1024, 64, 8)
    assert (d.window_left, d.splits, d.max_pages, d.page_size, d.num_pages, d.qh, d.kh, d.kv_format, d.reserved) == (48, 3, 3, 16, 9, 16, 2, 0, 0)
    assert pkg.paged_decode_attention_fp8_plan(q, k, v, tab, num_splits=3) == (3, 4 * 2 * 16 * 3 * 66) == pkg.decode_attention_fp8_plan(q, mk(2, 2, 48, 64), mk(2, 2, 48, 64), num_splits=3)
    assert pkg.paged_decode_attention_fp8_plan(q, k, v, tab) == (1, 0)
