"""CPU tests of the weight-streaming MXFP4 expert layer (include/nnop_hip_moe_mx_decode.h), the checks tests/test_zzzzzzzzz_moe_mx_host.py
makes of the seventh library made of the eighth: it loads and exports exactly its header's two functions, none of the other seven
libraries exports them, it links none of them, its header is plain C99 and its descriptor matches the ctypes one, the binding passes what
tests/test_zzzzzz_bindings_host.py asks of the others, the entry point validates in the header's order and returns before any launch,
and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_moe_mx_decode.h")
NAMES = {"nnop_moe_mx_decode_abi_version", "nnop_moe_mx_decode_linear"}
PY_NAMES = ("moe_decode_linear_mxfp4", "_moe_decode_linear_mxfp4", "moe_decode_linear_mxfp4_into")
FIELDS = ["dtype", "rows", "experts", "in_dim", "out_dim", "ld_x", "ld_y", "ld_b", "ld_q", "ld_s", "flags", "reserved"]
REBUILD = "rebuild with `make -C nnop.jl_amd/csrc -j8`"
ALIGNS, OPTIONAL = ("t", "t", 16, 1, "t", 4), (4,)   # ys xs blocks scales bias offsets: the alignment of each pointer ("t" = dtype)
OK = C.c_void_p(0x7f0000001000)                      # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
at = lambda off: C.c_void_p(0x7f0000001000 + off)


# ---- the library, its header, its binding ---------------------------------------------------------------------------------------------
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_exactly_the_headers_functions(pkg):
    M = pkg._lib_moe_mx_decode
    lib = M.load()
    assert set(M.EXPORTED_SYMBOLS) == NAMES
    assert _defined(M.LIB_PATH) == NAMES
    header = strip_c_comments(open(HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert lib.nnop_moe_mx_decode_abi_version() == M.MOE_MX_DECODE_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_MX_DECODE_ABI_VERSION (\d+)", header).group(1)) == 1
    needed = subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip" not in needed                               # none of the other seven libraries
    for name in PY_NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name)) and name in pkg.moe_mx_decode.__all__
    assert "moe_mx_decode" in pkg.__all__ and "_lib_moe_mx_decode" in pkg.__all__
    others = (pkg._lib, pkg._lib_ext, pkg._lib_moe, pkg._lib_moe_data, pkg._lib_moe_gemm, pkg._lib_moe_linear, pkg._lib_moe_mx)
    assert len({o.LIB_PATH for o in others} | {M.LIB_PATH}) == 8
    for other in others:
        assert not NAMES & set(other.EXPORTED_SYMBOLS) and not NAMES & _defined(other.LIB_PATH)


def test_descriptor_matches_the_header_and_the_seventh_librarys(pkg):
    M = pkg._lib_moe_mx_decode
    body = re.search(r"typedef struct nnop_moe_mx_decode_desc \{(.*?)\} nnop_moe_mx_decode_desc;", strip_c_comments(open(HEADER).read()), re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), int(m.group(2) or 1), {"int32_t": C.c_int32, "uint32_t": C.c_uint32}[ctype]))
    D = M.MoeMxDecodeDesc
    assert C.sizeof(D) == 64
    assert [f[0] for f in fields] == FIELDS == [n for n, _ in D._fields_]
    assert [f[1] for f in fields] == [getattr(t, "_length_", 1) for _, t in D._fields_]
    assert [f[2] for f in fields] == [(t._type_ if hasattr(t, "_length_") else t) for _, t in D._fields_]
    assert D.flags.offset == 40 and D.reserved.offset == 44
    assert (M.MAX_EXPERTS, M.MAX_DIM, M.BLOCK) == (1024, 65536, 32)
    S = pkg._lib_moe_mx.MoeMxDesc                                    # the fields of nnop_moe_mx_desc, one for one
    assert [(n, getattr(D, n).offset, getattr(D, n).size) for n in FIELDS] == [(n, getattr(S, n).offset, getattr(S, n).size) for n in FIELDS]


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe_mx_decode.h"\n'
                 "int main(void){ nnop_moe_mx_decode_desc a; a.flags = 0u;\n"
                 "  return (sizeof(a) == 64 && NNOP_HIP_MOE_MX_DECODE_ABI_VERSION == 1 && a.flags == 0u) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_the_bindings_glue_holds_for_the_eighth_library(pkg, monkeypatch):
    """the three checks tests/test_zzzzzz_bindings_host.py makes of the other bindings, and its check of an operator module"""
    M, common, module = pkg._lib_moe_mx_decode, pkg._common, pkg.moe_mx_decode
    lib = M.load()
    assert M.load() is lib is M._lib and M.EXPORTED_SYMBOLS == tuple(M.PROTOTYPES)
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
    assert module.NNopError is common.NNopError and module._DTYPES is common._DTYPES
    for name in ("_ptr", "_stream", "_on_device", "_raise", "_launch", "_dtype_name"):
        assert vars(module).get(name, getattr(common, name)) is getattr(common, name), name
    assert "_ptr" in vars(module)
    # the checks and the pullbacks are the seventh and sixth library's own, not copies
    assert module._check is pkg.moe_mx._check and module.grad_moe_grouped_linear_mxfp4_x_into is pkg.moe_mx.grad_moe_grouped_linear_mxfp4_x_into
    assert module.grad_moe_grouped_linear_b_into is pkg.moe_linear.grad_moe_grouped_linear_b_into
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "MOE_MX_DECODE_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} has moe-mx-decode-ABI version 1, this binding needs 2: {REBUILD}"
    monkeypatch.setattr(M, "MOE_MX_DECODE_ABI_VERSION", 1)
    monkeypatch.setattr(M, "EXPORTED_SYMBOLS", M.EXPORTED_SYMBOLS + ("nnop_not_there",))
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} does not export nnop_not_there: {REBUILD}"
    monkeypatch.setattr(M, "LIB_PATH", "/nonexistent/libnnop.so")
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == ("/nonexistent/libnnop.so not found: build it with `make -C nnop.jl_amd/csrc -j8` "
                            "(or __graft_entry__.build()).  There is no CPU or PyTorch fallback.")
    assert M._lib is None                        # a refused load leaves nothing behind


# ---- validation: order and codes, before any launch -----------------------------------------------------------------------------------
def _desc(pkg, reserved=(0, 0, 0, 0, 0), **kw):
    base = dict(dtype=2, rows=256, experts=8, in_dim=128, out_dim=64, ld_x=128, ld_y=64, ld_b=64, ld_q=64, ld_s=4, flags=0)
    base.update(kw)
    d = pkg._lib_moe_mx_decode.MoeMxDecodeDesc(**base)
    for i, r in enumerate(reserved):
        d.reserved[i] = r
    return d


def _call(lib, d, ptrs):
    return lib.nnop_moe_mx_decode_linear(C.byref(d) if d is not None else None, *ptrs, None)


def _all(lib, d, ptr=OK):
    return _call(lib, d, [ptr] * len(ALIGNS))


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # fp32 rows beside packed weights
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(flags=0x80000000), "NNOP_ERR_OPTS"),
    (dict(reserved=(1, 0, 0, 0, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, 0, -1, 0, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, 0, 0, 0, 7)), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-3), "NNOP_ERR_SHAPE"),
    (dict(experts=0), "NNOP_ERR_SHAPE"),
    (dict(experts=1025), "NNOP_ERR_SHAPE"),
    (dict(in_dim=0), "NNOP_ERR_SHAPE"),
    (dict(out_dim=0), "NNOP_ERR_SHAPE"),
    (dict(in_dim=65568, ld_x=65568, ld_q=32784, ld_s=2049), "NNOP_ERR_SHAPE"),
    (dict(out_dim=65537, ld_y=65537, ld_b=65537), "NNOP_ERR_SHAPE"),
    (dict(in_dim=120, ld_x=120), "NNOP_ERR_SHAPE"),                  # K no multiple of 32
    (dict(in_dim=16, ld_x=16), "NNOP_ERR_SHAPE"),
    (dict(ld_x=127), "NNOP_ERR_SHAPE"),                              # ld = dim - 1, each stride
    (dict(ld_y=63), "NNOP_ERR_SHAPE"),
    (dict(ld_b=63), "NNOP_ERR_SHAPE"),
    (dict(ld_q=48), "NNOP_ERR_SHAPE"),                               # below K / 2
    (dict(ld_q=72), "NNOP_ERR_SHAPE"),                               # no multiple of 16
    (dict(ld_s=3), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, flags=8, rows=0), "NNOP_ERR_DTYPE"),
    (dict(dtype=7, reserved=(5, 0, 0, 0, 0), in_dim=120), "NNOP_ERR_DTYPE"),
    (dict(reserved=(0, 3, 0, 0, 0), rows=0), "NNOP_ERR_OPTS"),
    (dict(flags=16, ld_q=72), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_mx_decode.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert _all(lib, d) == want
    assert _all(lib, d, NULL) == want                                # the descriptor is judged before the pointers
    assert _all(lib, d, at(1)) == want


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    """the largest shapes included: E ceil(N / 256) workgroups stay below 2^31 for every E and N the bounds admit, whatever S is"""
    lib, L = pkg._lib_moe_mx_decode.load(), pkg._lib
    for ok in (dict(), dict(dtype=1), dict(rows=1, experts=1, in_dim=32, out_dim=1, ld_x=32, ld_y=1, ld_b=1, ld_q=16, ld_s=1),
               dict(experts=1024), dict(ld_q=80, ld_s=9, ld_x=131, ld_y=67, ld_b=70), dict(out_dim=5, ld_y=5, ld_b=5),
               dict(in_dim=65536, ld_x=65536, ld_q=32768, ld_s=2048), dict(out_dim=65536, ld_y=65536, ld_b=65536),
               dict(rows=2 ** 31 - 1, in_dim=32, out_dim=8, ld_x=32, ld_y=8, ld_b=8, ld_q=16, ld_s=1),
               dict(rows=2 ** 31 - 1, experts=1024, in_dim=65536, out_dim=65536, ld_x=65536, ld_y=65536, ld_b=65536, ld_q=32768, ld_s=2048)):
        assert _all(lib, _desc(pkg, **ok), NULL) == L.NNOP_ERR_NULL, ok
    assert _all(lib, None) == L.NNOP_ERR_NULL                        # the descriptor itself: first of all
    assert _all(lib, None, at(1)) == L.NNOP_ERR_NULL


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe_mx_decode.load(), pkg._lib
    n = len(ALIGNS)
    for dtype in (1, 2):
        d = _desc(pkg, dtype=dtype)
        for pos, a in enumerate(ALIGNS):
            b, c = [OK] * n, [at(1)] * n                             # NULL is judged before alignment
            b[pos] = c[pos] = NULL
            if pos in OPTIONAL:                                      # bias: NULL means none, so the call goes on to the next check
                assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos
            else:
                assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
                assert _call(lib, d, c) == L.NNOP_ERR_NULL, pos
            size = 2 if a == "t" else a
            if size > 1:                                             # scales: bytes, any address
                c = [OK] * n
                c[pos] = at(size // 2)                               # aligned to half of what is needed
                assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, (pos, a)


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    S, E, N, K = 10, 3, 6, 64
    f = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt)
    u = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    xs, ys, q, sc, b, off = f(S, K), f(S, N), u(E, N, 2, 16), u(E, N, 2), f(E, N), torch.zeros(E + 1, dtype=torch.int32)
    for call in (lambda: pkg.moe_decode_linear_mxfp4(xs, q, sc, off), lambda: pkg._moe_decode_linear_mxfp4(xs, q, sc, off, b),
                 lambda: pkg.moe_decode_linear_mxfp4_into(ys, xs, q, sc, off, b),
                 lambda: pkg.moe_decode_linear_mxfp4(xs.clone().requires_grad_(True), q, sc, off, b),
                 lambda: pkg.moe_decode_linear_mxfp4(xs, q, sc, off, b.clone().requires_grad_(True))):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    mu = lambda *s: torch.zeros(*s, dtype=torch.uint8).as_subclass(OnGpu)
    mi = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnGpu)
    xs, ys, q, sc, b, off = mk(S, K), mk(S, N), mu(E, N, 2, 16), mu(E, N, 2), mk(E, N), mi(E + 1)
    for call in (lambda: pkg.moe_decode_linear_mxfp4(mk(S, K, dt=torch.float64), q, sc, off), lambda: pkg.moe_decode_linear_mxfp4(xs, [1], sc, off),
                 lambda: pkg.moe_decode_linear_mxfp4(xs, q, sc, off, mi(E, N)), lambda: pkg.moe_decode_linear_mxfp4(xs, q, sc, off.long())):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(pkg.NNopError, match="must be float16 or bfloat16") as e:     # fp32 rows beside packed weights
        pkg.moe_decode_linear_mxfp4(mk(S, K, dt=torch.float32), q, sc, off)
    assert e.value.status == pkg._lib.NNOP_ERR_DTYPE
    # packed weights of another type, not contiguous (never copied), of a shape that does not fit; rows, bias, outputs that do not fit
    for bad in (lambda: pkg.moe_decode_linear_mxfp4(xs, q.to(torch.int8).as_subclass(OnGpu), sc, off),
                lambda: pkg.moe_decode_linear_mxfp4(xs, q, mk(E, N, 2), off),
                lambda: pkg.moe_decode_linear_mxfp4(xs, mu(E, N, 16, 2).transpose(2, 3), sc, off),
                lambda: pkg.moe_decode_linear_mxfp4(xs, q, mu(E, 2, N).transpose(1, 2), off),
                lambda: pkg.moe_decode_linear_mxfp4(xs, mu(E, N, 2, 8), sc, off), lambda: pkg.moe_decode_linear_mxfp4(xs, mu(E, N, 33), sc, off),
                lambda: pkg.moe_decode_linear_mxfp4(xs, mu(E, N + 1, 2, 16), sc, off), lambda: pkg.moe_decode_linear_mxfp4(xs, mu(N, 2, 16), mu(N, 2), off),
                lambda: pkg.moe_decode_linear_mxfp4(mk(S, K + 32), q, sc, off), lambda: pkg.moe_decode_linear_mxfp4(mk(S, K, dt=torch.float16), q, sc, off, b),
                lambda: pkg.moe_decode_linear_mxfp4(xs, q, sc, off, mk(E, N + 1)), lambda: pkg.moe_decode_linear_mxfp4(xs, q, sc, mi(E)),
                lambda: pkg.moe_decode_linear_mxfp4_into(mk(S, N + 1), xs, q, sc, off), lambda: pkg.moe_decode_linear_mxfp4_into(mk(N, S).t(), xs, q, sc, off)):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    for call in (lambda: pkg.moe_decode_linear_mxfp4(mk(0, K), q, sc, off),
                 lambda: pkg.moe_decode_linear_mxfp4(mk(S, K), mu(1025, N, 2, 16), mu(1025, N, 2), mi(1026))):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    # the descriptor a call builds: the packed strides are the dense ones, unused row strides too
    d = pkg.moe_mx_decode._desc(torch.zeros(3, 96, dtype=torch.float16), 3, 4, 96, 24, ld_x=99, ld_y=32)
    assert [getattr(d, n) for n, _ in d._fields_[:-1]] == [1, 3, 4, 96, 24, 99, 32, 24, 48, 3, 0] and tuple(d.reserved) == (0,) * 5
