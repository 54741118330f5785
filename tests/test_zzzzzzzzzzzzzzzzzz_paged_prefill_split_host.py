"""CPU tests of the C boundary and wrappers of split-KV prefill attention over a paged KV cache (include/nnop_hip_paged_prefill_split.h):
the sixteenth library exports exactly its header's three functions and links none of the other fifteen, takes the thirteenth library's
descriptor with `reserved` as the split count, validates in the header's order and returns before any launch, resolves the automatic
count and the workspace size from host values alone, and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments
from test_zzzzzzzzzzzzzzz_paged_prefill_host import NULL, OK, OnGpu, _kw, at

HEADER = os.path.join(ROOT, "include", "nnop_hip_paged_prefill_split.h")
NAMES = {"nnop_paged_prefill_split_abi_version", "nnop_paged_prefill_split_plan", "nnop_paged_prefill_split"}
SMALL = dict(tokens=64, batch=1)                                 # 8 (4 + 1) = 40 workgroups unsplit: ceil(512 / 40) = 13


def _call(lib, d, ptrs, nbytes=0):
    return lib.nnop_paged_prefill_split(C.byref(d), *ptrs, nbytes, None)


def _plan(lib, d):
    s, n = C.c_int32(-1), C.c_size_t(1)
    return lib.nnop_paged_prefill_split_plan(C.byref(d), C.byref(s), C.byref(n)), s.value, n.value


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_paged_prefill_split
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_paged_prefill_split.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_paged_prefill_split_abi_version() == M.PAGED_PREFILL_SPLIT_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert M.PagedPrefillDesc is pkg._lib_paged_prefill.PagedPrefillDesc and C.sizeof(M.PagedPrefillDesc) == 136
    assert (M.MAX_SPLITS, M.MIN_CHUNK_TILES) == tuple(int(re.search(rf"#define NNOP_PAGED_PREFILL_SPLIT_{n}\s+(\d+)", header).group(1))
                                                     for n in ("MAX_SPLITS", "MIN_CHUNK_TILES"))
    for name in ("paged_prefill_attention_split", "paged_prefill_attention_split_into", "paged_prefill_attention_split_plan",
                 "paged_prefill_split", "_lib_paged_prefill_split"):
        assert name in pkg.__all__ and hasattr(pkg, name)


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(reserved=65), "NNOP_ERR_OPTS"),                            # the split count: 0 ... 64
    (dict(reserved=-1), "NNOP_ERR_OPTS"),
    (dict(window_left=-2), "NNOP_ERR_OPTS"),
    (dict(emb=32), "NNOP_ERR_SHAPE"),
    (dict(tokens=0), "NNOP_ERR_SHAPE"),
    (dict(qh=60), "NNOP_ERR_SHAPE"),
    (dict(page_size=8), "NNOP_ERR_SHAPE"),
    (dict(max_pages=2 ** 27), "NNOP_ERR_SHAPE"),
    (dict(v_stride_p=8 * 16 * 64 + 4), "NNOP_ERR_SHAPE"),
    (dict(o_stride_h=68), "NNOP_ERR_SHAPE"),
    (dict(table_stride=255), "NNOP_ERR_SHAPE"),
    (dict(batch=2 ** 26, reserved=8), "NNOP_ERR_SHAPE"),             # 2^29 workgroups unsplit (the automatic count is 1), 2^32 in 8 chunks
    (dict(tokens=2 ** 26), "NNOP_ERR_SHAPE"),                        # 2^32 rows of lse
    # the order: dtype before options before shape, all before the pointers and the workspace
    (dict(dtype=0, reserved=65, page_size=8), "NNOP_ERR_DTYPE"),
    (dict(reserved=65, page_size=8), "NNOP_ERR_OPTS"),
    (dict(page_size=8, reserved=7), "NNOP_ERR_SHAPE"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    M, want = pkg._lib_paged_prefill_split, getattr(pkg._lib, status)
    lib, d = M.load(), M.PagedPrefillDesc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 10) == want
    assert _plan(lib, d) == (want, -1, 1)
    assert lib.nnop_paged_prefill_split(None, *[OK] * 10, 0, None) == pkg._lib.NNOP_ERR_NULL
    assert lib.nnop_paged_prefill_split_plan(C.byref(d), None, C.byref(C.c_size_t())) == pkg._lib.NNOP_ERR_NULL
    assert lib.nnop_paged_prefill_split_plan(C.byref(d), C.byref(C.c_int32()), None) == pkg._lib.NNOP_ERR_NULL
    assert _plan(lib, M.PagedPrefillDesc(**_kw(batch=2 ** 26)))[:2] == (pkg._lib.NNOP_OK, 1)


def test_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_paged_prefill_split, pkg._lib
    lib, d = M.load(), M.PagedPrefillDesc(**_kw(reserved=3))
    need = _plan(lib, d)[2]
    assert need == 4 * 1000 * 64 * 3 * 66
    # o lse q k v block_table cu_seqlens_q seqlens sinks workspace; lse and sinks are optional, the workspace is not at three chunks
    for pos, a in enumerate((16, 4, 16, 16, 16, 4, 4, 4, 4, 16)):
        b, c = [OK] * 10, [at(1)] * 10                               # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c, need) == (L.NNOP_ERR_ALIGN if pos in (1, 8) else L.NNOP_ERR_NULL), pos
        if pos not in (1, 8):
            assert _call(lib, d, b, need) == L.NNOP_ERR_NULL, pos
        c = [OK] * 10
        c[pos] = at(a // 2)                                          # aligned to half of what is needed
        assert _call(lib, d, c, need) == L.NNOP_ERR_ALIGN, pos
    assert _call(lib, d, [OK] * 10, need - 1) == L.NNOP_ERR_WORKSPACE == _call(lib, d, [OK] * 10, 0)
    one = M.PagedPrefillDesc(**_kw(reserved=1))                      # at one chunk no workspace is asked for: the next check answers
    assert _call(lib, one, [OK, OK, at(8)] + [OK] * 6 + [NULL]) == L.NNOP_ERR_ALIGN


@pytest.mark.parametrize("kw,splits", [
    (dict(), 1),                                                     # 8 (62 + 4) = 528 workgroups: the unsplit call fills the chip
    (dict(tokens=8192, batch=8), 1),
    (dict(SMALL), 13),                                               # 128 tiles: chunks of 8 would allow 16
    (dict(SMALL, emb=128, **{f"{t}_stride_{a}": 64 * 128 if a == "t" else 128 for t in "qo" for a in "th"},
          **{f"{t}_stride_{a}": 128 for t in "kv" for a in "phl"}), 13),
    (dict(SMALL, max_pages=32), 2),                                  # 16 tiles: two chunks of 8
    (dict(SMALL, max_pages=15), 1),                                  # 8 tiles: one chunk
    (dict(SMALL, window_left=100), 1),                               # (16 + 100) / 32 + 2 = 5 live tiles
    (dict(SMALL, window_left=1000), 4),                              # 33 live tiles
    (dict(SMALL, window_left=4096), 13),                             # a window past the table's end removes nothing
    (dict(tokens=16, batch=1, qh=8, kh=1, max_pages=2 ** 20, table_stride=2 ** 20), 64),   # 2 workgroups: 256, clamped
    (dict(reserved=7), 7),
    (dict(SMALL, reserved=64), 64),
    (dict(SMALL, reserved=1), 1),
])
def test_the_plan_resolves_the_split_count_and_the_workspace_from_host_values(pkg, kw, splits):
    M = pkg._lib_paged_prefill_split
    d = M.PagedPrefillDesc(**_kw(**kw))
    assert _plan(M.load(), d) == (pkg._lib.NNOP_OK, splits, 4 * d.tokens * d.qh * splits * (d.emb + 2) if splits > 1 else 0)


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    q, k, v, tab = mk(7, 16, 64), mk(9, 2, 16, 64), mk(9, 2, 16, 64), mk(2, 3, dt=torch.int32)
    cu, lens = mk(3, dt=torch.int32), mk(2, dt=torch.int32)
    A, E = pkg.paged_prefill_attention_split, pkg.NNopError
    for bad, status in ((lambda: A(q, mk(9, 2, 16, 64, dt=torch.float16), v, tab, cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, mk(9, 2, 16, 64, dt=torch.float8_e4m3fn), v, tab, cu, lens), "NNOP_ERR_DTYPE"),   # 16-bit pages only
                        (lambda: A(q, mk(9, 2, 8, 64), mk(9, 2, 8, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(mk(7, 34, 64), k, v, tab, cu, lens), "NNOP_ERR_SHAPE"),                # G = 17
                        (lambda: A(q, k, v, tab, mk(2, dt=torch.int32), lens, num_splits=3), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, tab, cu, lens, num_splits=3, workspace=mk(16)[::2]), "NNOP_ERR_WORKSPACE"),   # not contiguous
                        (lambda: pkg.paged_prefill_attention_split_into(mk(7, 16, 64, dt=torch.float16), None, q, k, v, tab, cu, lens), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    for bad, err in ((dict(num_splits=0), ValueError), (dict(num_splits=65), ValueError), (dict(num_splits=2.0), TypeError),
                     (dict(num_splits=True), TypeError), (dict(window_left=-1), ValueError)):
        with pytest.raises(err):
            A(q, k, v, tab, cu, lens, **bad)
    P = pkg.paged_prefill_attention_split_plan
    assert P(q, k, v, tab) == (1, 0) == P(q[:0], k, v, tab, num_splits=5)          # 3 pages of 16: a single tile and a half; no token
    assert P(q, k, v, tab, num_splits=5) == (5, 4 * 7 * 16 * 5 * 66)
    assert pkg.paged_prefill_split._desc(q, k, v, tab, 128, 9).reserved == 9
