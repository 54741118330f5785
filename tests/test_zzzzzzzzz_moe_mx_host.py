"""CPU tests of the MXFP4 expert weights (include/nnop_hip_moe_mx.h): the seventh library loads and exports exactly its header's functions,
links none of the other six, its header is plain C99 and its descriptors match the ctypes ones, the binding passes what
tests/test_zzzzzz_bindings_host.py asks of the others, every entry point validates in the header's order and returns before any launch,
the Python wrappers raise before any device work, and the reference the GPU tests are judged against (tests/mx_ref.py) holds against
statements of the format that do not share its code.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mx_ref
from abi_util import ROOT, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_moe_mx.h")
NAMES = {"nnop_moe_mx_abi_version", "nnop_moe_mx_linear", "nnop_moe_mx_linear_bwd_x", "nnop_mxfp4_dequant", "nnop_mxfp4_quant"}
PY_NAMES = ("mxfp4_quantize", "mxfp4_dequantize", "moe_grouped_linear_mxfp4", "_moe_grouped_linear_mxfp4",
            "moe_grouped_linear_mxfp4_into", "grad_moe_grouped_linear_mxfp4_x_into")
REBUILD = "rebuild with `make -C nnop.jl_amd/csrc -j8`"
# entry point -> the alignment of each pointer ("t" = dtype, 16, 1, 4) and the optional positions
LINEAR = {"nnop_moe_mx_linear": (("t", "t", 16, 1, "t", 4), (4,)), "nnop_moe_mx_linear_bwd_x": (("t", "t", 16, 1, 4), ())}
ROWS = {"nnop_mxfp4_dequant": ("t", 16, 1), "nnop_mxfp4_quant": (16, 1, "t")}
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
at = lambda off: C.c_void_p(0x7f0000001000 + off)


# ---- the library, its header, its binding ---------------------------------------------------------------------------------------------
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_exactly_the_headers_functions(pkg):
    M = pkg._lib_moe_mx
    lib = M.load()
    assert set(M.EXPORTED_SYMBOLS) == NAMES
    assert _defined(M.LIB_PATH) == NAMES
    header = strip_c_comments(open(HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert lib.nnop_moe_mx_abi_version() == M.MOE_MX_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_MX_ABI_VERSION (\d+)", header).group(1)) == 1
    needed = subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip" not in needed                               # none of the other six libraries
    for name in PY_NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name)) and name in pkg.moe_mx.__all__
    assert "moe_mx" in pkg.__all__ and "_lib_moe_mx" in pkg.__all__
    for other in (pkg._lib, pkg._lib_ext, pkg._lib_moe, pkg._lib_moe_data, pkg._lib_moe_gemm, pkg._lib_moe_linear):
        assert not NAMES & set(other.EXPORTED_SYMBOLS) and not NAMES & _defined(other.LIB_PATH)


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), strip_c_comments(open(HEADER).read()), re.S).group(1)
    out = []
    for ctype, names in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            out.append((m.group(1), int(m.group(2) or 1), {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64}[ctype]))
    return out


def test_descriptors_match_the_header(pkg):
    M = pkg._lib_moe_mx
    for struct, D, size, names in (("nnop_moe_mx_desc", M.MoeMxDesc, 64, ["dtype", "rows", "experts", "in_dim", "out_dim", "ld_x", "ld_y",
                                                                         "ld_b", "ld_q", "ld_s", "flags", "reserved"]),
                                   ("nnop_mxfp4_desc", M.Mxfp4Desc, 32, ["dtype", "reserved", "rows", "cols", "ld", "ld_q", "ld_s"])):
        fields = _fields(struct)
        assert C.sizeof(D) == size
        assert [f[0] for f in fields] == names == [n for n, _ in D._fields_]
        assert [f[1] for f in fields] == [getattr(t, "_length_", 1) for _, t in D._fields_]
        assert [f[2] for f in fields] == [(t._type_ if hasattr(t, "_length_") else t) for _, t in D._fields_]
    assert M.MoeMxDesc.flags.offset == 40 and M.MoeMxDesc.reserved.offset == 44 and M.Mxfp4Desc.rows.offset == 8
    assert (M.MAX_EXPERTS, M.MAX_DIM, M.BLOCK, M.MAX_COLS, M.MAX_PIECES) == (1024, 65536, 32, 2 ** 30, 2 ** 39)


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe_mx.h"\n'
                 "int main(void){ nnop_moe_mx_desc a; nnop_mxfp4_desc b; a.flags = 0u; b.rows = 1;\n"
                 "  return (sizeof(a) == 64 && sizeof(b) == 32 && NNOP_HIP_MOE_MX_ABI_VERSION == 1 && a.flags == 0u && b.rows == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_the_bindings_glue_holds_for_the_seventh_library(pkg, monkeypatch):
    """the three checks tests/test_zzzzzz_bindings_host.py makes of the other bindings, and its check of an operator module"""
    M, common, module = pkg._lib_moe_mx, pkg._common, pkg.moe_mx
    lib = M.load()
    assert M.load() is lib is M._lib and M.EXPORTED_SYMBOLS == tuple(M.PROTOTYPES)
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
    assert module.NNopError is common.NNopError and module._DTYPES is common._DTYPES
    for name in ("_ptr", "_stream", "_on_device", "_raise", "_launch", "_dtype_name"):
        assert vars(module).get(name, getattr(common, name)) is getattr(common, name), name
    assert "_ptr" in vars(module)
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "MOE_MX_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} has moe-mx-ABI version 1, this binding needs 2: {REBUILD}"
    monkeypatch.setattr(M, "MOE_MX_ABI_VERSION", 1)
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


# ---- validation of the two products: order and codes, before any launch ---------------------------------------------------------------
def _desc(pkg, reserved=(0, 0, 0, 0, 0), **kw):
    base = dict(dtype=2, rows=256, experts=8, in_dim=128, out_dim=64, ld_x=128, ld_y=64, ld_b=64, ld_q=64, ld_s=4, flags=0)
    base.update(kw)
    d = pkg._lib_moe_mx.MoeMxDesc(**base)
    for i, r in enumerate(reserved):
        d.reserved[i] = r
    return d


def _call(lib, name, d, ptrs):
    return getattr(lib, name)(C.byref(d) if d is not None else None, *ptrs, None)


def _both(lib, d, ptr=OK):
    return [_call(lib, name, d, [ptr] * len(LINEAR[name][0])) for name in LINEAR]


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
    (dict(rows=2 ** 31 - 1, in_dim=65536, out_dim=65536, ld_x=65536, ld_y=65536, ld_b=65536, ld_q=32768, ld_s=2048), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, flags=8, rows=0), "NNOP_ERR_DTYPE"),
    (dict(dtype=7, reserved=(5, 0, 0, 0, 0), in_dim=120), "NNOP_ERR_DTYPE"),
    (dict(reserved=(0, 3, 0, 0, 0), rows=0), "NNOP_ERR_OPTS"),
    (dict(flags=16, ld_q=72), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_mx.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert _both(lib, d) == [want] * 2
    assert _both(lib, d, NULL) == [want] * 2                         # the descriptor is judged before the pointers
    assert _both(lib, d, at(1)) == [want] * 2


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    lib, L = pkg._lib_moe_mx.load(), pkg._lib
    for ok in (dict(), dict(dtype=1), dict(rows=1, experts=1, in_dim=32, out_dim=1, ld_x=32, ld_y=1, ld_b=1, ld_q=16, ld_s=1),
               dict(experts=1024), dict(ld_q=80, ld_s=9, ld_x=131, ld_y=67, ld_b=70), dict(out_dim=5, ld_y=5, ld_b=5),
               dict(in_dim=65536, ld_x=65536, ld_q=32768, ld_s=2048), dict(out_dim=65536, ld_y=65536, ld_b=65536),
               dict(rows=2 ** 31 - 1, in_dim=32, out_dim=8, ld_x=32, ld_y=8, ld_b=8, ld_q=16, ld_s=1)):
        assert _both(lib, _desc(pkg, **ok), NULL) == [L.NNOP_ERR_NULL] * 2, ok
    assert _both(lib, None) == [L.NNOP_ERR_NULL] * 2                 # the descriptor itself: first of all
    assert _both(lib, None, at(1)) == [L.NNOP_ERR_NULL] * 2


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe_mx.load(), pkg._lib
    for dtype in (1, 2):
        d = _desc(pkg, dtype=dtype)
        for name, (aligns, optional) in LINEAR.items():
            n = len(aligns)
            for pos, a in enumerate(aligns):
                b, c = [OK] * n, [at(1)] * n                         # NULL is judged before alignment
                b[pos] = c[pos] = NULL
                if pos in optional:                                  # bias: NULL means none, so the call goes on to the next check
                    assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos)
                else:
                    assert _call(lib, name, d, b) == L.NNOP_ERR_NULL, (name, pos)
                    assert _call(lib, name, d, c) == L.NNOP_ERR_NULL, (name, pos)
                size = 2 if a == "t" else a
                if size > 1:                                         # scales: bytes, any address
                    c = [OK] * n
                    c[pos] = at(size // 2)                           # aligned to half of what is needed
                    assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos, a)


# ---- validation of the two conversions ------------------------------------------------------------------------------------------------
def _rows_desc(pkg, **kw):
    base = dict(dtype=2, reserved=0, rows=37, cols=96, ld=96, ld_q=48, ld_s=3)
    base.update(kw)
    return pkg._lib_moe_mx.Mxfp4Desc(**base)


def _convs(lib, d, ptr=OK):
    return [_call(lib, name, d, [ptr] * 3) for name in ROWS]


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=3), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(reserved=1), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-1), "NNOP_ERR_SHAPE"),
    (dict(cols=0), "NNOP_ERR_SHAPE"),
    (dict(cols=16, ld_q=16), "NNOP_ERR_SHAPE"),
    (dict(cols=100, ld=100, ld_q=64, ld_s=4), "NNOP_ERR_SHAPE"),
    (dict(cols=2 ** 30 + 32, ld=2 ** 30 + 32, ld_q=2 ** 29 + 16, ld_s=2 ** 25 + 1), "NNOP_ERR_SHAPE"),
    (dict(ld=95), "NNOP_ERR_SHAPE"),
    (dict(ld_q=32), "NNOP_ERR_SHAPE"),
    (dict(ld_q=56), "NNOP_ERR_SHAPE"),
    (dict(ld_s=2), "NNOP_ERR_SHAPE"),
    (dict(rows=2 ** 39 // 12 + 1), "NNOP_ERR_SHAPE"),                # rows K / 8 above 2^39
    (dict(dtype=5, reserved=2, rows=0), "NNOP_ERR_DTYPE"),
    (dict(reserved=2, rows=0), "NNOP_ERR_OPTS"),
])
def test_conversion_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_mx.load(), getattr(pkg._lib, status)
    d = _rows_desc(pkg, **kw)
    assert _convs(lib, d) == _convs(lib, d, NULL) == _convs(lib, d, at(1)) == [want] * 2


def test_conversion_pointer_checks(pkg):
    lib, L = pkg._lib_moe_mx.load(), pkg._lib
    for ok in (dict(), dict(dtype=0), dict(dtype=1), dict(rows=1, cols=32, ld=32, ld_q=16, ld_s=1), dict(ld=104, ld_q=64, ld_s=7),
               dict(rows=2 ** 39 // 12), dict(rows=2 ** 9, cols=2 ** 30, ld=2 ** 30, ld_q=2 ** 29, ld_s=2 ** 25)):
        assert _convs(lib, _rows_desc(pkg, **ok), NULL) == [L.NNOP_ERR_NULL] * 2, ok
    assert _convs(lib, None) == _convs(lib, None, at(1)) == [L.NNOP_ERR_NULL] * 2
    for dtype, esize in ((0, 4), (1, 2), (2, 2)):
        d = _rows_desc(pkg, dtype=dtype)
        for name, aligns in ROWS.items():
            for pos, a in enumerate(aligns):
                b, c = [OK] * 3, [at(1)] * 3
                b[pos] = c[pos] = NULL
                assert _call(lib, name, d, b) == _call(lib, name, d, c) == L.NNOP_ERR_NULL, (name, pos)
                size = esize if a == "t" else a
                if size > 1:
                    c = [OK] * 3
                    c[pos] = at(size // 2)
                    assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos, a)


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    S, E, N, K = 10, 3, 6, 64
    f = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt)
    u = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    xs, ys, q, sc, b, off = f(S, K), f(S, N), u(E, N, 2, 16), u(E, N, 2), f(E, N), torch.zeros(E + 1, dtype=torch.int32)
    for call in (lambda: pkg.moe_grouped_linear_mxfp4(xs, q, sc, off), lambda: pkg._moe_grouped_linear_mxfp4(xs, q, sc, off, b),
                 lambda: pkg.moe_grouped_linear_mxfp4_into(ys, xs, q, sc, off, b),
                 lambda: pkg.grad_moe_grouped_linear_mxfp4_x_into(xs, ys, q, sc, off),
                 lambda: pkg.moe_grouped_linear_mxfp4(xs.clone().requires_grad_(True), q, sc, off, b),
                 lambda: pkg.moe_grouped_linear_mxfp4(xs, q, sc, off, b.clone().requires_grad_(True)),
                 lambda: pkg.mxfp4_quantize(f(4, K)), lambda: pkg.mxfp4_dequantize(q, sc)):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    mu = lambda *s: torch.zeros(*s, dtype=torch.uint8).as_subclass(OnGpu)
    mi = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnGpu)
    xs, ys, q, qf, sc, b, off = mk(S, K), mk(S, N), mu(E, N, 2, 16), mu(E, N, 32), mu(E, N, 2), mk(E, N), mi(E + 1)
    for call in (lambda: pkg.moe_grouped_linear_mxfp4(mk(S, K, dt=torch.float64), q, sc, off), lambda: pkg.moe_grouped_linear_mxfp4(xs, [1], sc, off),
                 lambda: pkg.moe_grouped_linear_mxfp4(xs, q, sc, off, mi(E, N)), lambda: pkg.moe_grouped_linear_mxfp4(xs, q, sc, off.long()),
                 lambda: pkg.mxfp4_quantize(mi(4, K)), lambda: pkg.mxfp4_dequantize(q, sc, dtype=torch.float64)):
        with pytest.raises(TypeError):
            call()
    # fp32 rows beside packed weights
    for call in (lambda: pkg.moe_grouped_linear_mxfp4(mk(S, K, dt=torch.float32), q, sc, off),
                 lambda: pkg.grad_moe_grouped_linear_mxfp4_x_into(mk(S, K, dt=torch.float32), mk(S, N, dt=torch.float32), q, sc, off)):
        with pytest.raises(pkg.NNopError, match="must be float16 or bfloat16") as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_DTYPE
    # packed weights of another type, not contiguous (never copied), of a shape that does not fit; rows, bias, outputs that do not fit
    for bad in (lambda: pkg.moe_grouped_linear_mxfp4(xs, q.to(torch.int8).as_subclass(OnGpu), sc, off),
                lambda: pkg.moe_grouped_linear_mxfp4(xs, q, mk(E, N, 2), off),
                lambda: pkg.moe_grouped_linear_mxfp4(xs, mu(E, N, 16, 2).transpose(2, 3), sc, off),
                lambda: pkg.moe_grouped_linear_mxfp4(xs, q, mu(E, 2, N).transpose(1, 2), off),
                lambda: pkg.mxfp4_dequantize(mu(4, 4, 16)[:, ::2], mu(4, 2)),
                lambda: pkg.moe_grouped_linear_mxfp4(xs, mu(E, N, 2, 8), sc, off), lambda: pkg.moe_grouped_linear_mxfp4(xs, mu(E, N, 33), sc, off),
                lambda: pkg.moe_grouped_linear_mxfp4(xs, mu(E, N + 1, 2, 16), sc, off), lambda: pkg.moe_grouped_linear_mxfp4(xs, mu(N, 2, 16), mu(N, 2), off),
                lambda: pkg.mxfp4_dequantize(mu(4, 3, 16), mu(4, 2)), lambda: pkg.mxfp4_dequantize(mu(4, 0, 16), mu(4, 0)),
                lambda: pkg.moe_grouped_linear_mxfp4(mk(S, K + 32), q, sc, off), lambda: pkg.moe_grouped_linear_mxfp4(mk(S, K, dt=torch.float16), q, sc, off, b),
                lambda: pkg.moe_grouped_linear_mxfp4(xs, q, sc, off, mk(E, N + 1)), lambda: pkg.moe_grouped_linear_mxfp4(xs, q, sc, mi(E)),
                lambda: pkg.moe_grouped_linear_mxfp4_into(mk(S, N + 1), xs, q, sc, off), lambda: pkg.moe_grouped_linear_mxfp4_into(mk(N, S).t(), xs, q, sc, off),
                lambda: pkg.grad_moe_grouped_linear_mxfp4_x_into(mk(S, K + 1), ys, q, sc, off),
                lambda: pkg.grad_moe_grouped_linear_mxfp4_x_into(xs, mk(S, N + 1), q, sc, off),
                lambda: pkg.grad_moe_grouped_linear_mxfp4_x_into(mk(S, K, dt=torch.float16), ys, qf, sc, off)):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    for call in (lambda: pkg.moe_grouped_linear_mxfp4(mk(0, K), q, sc, off), lambda: pkg.mxfp4_quantize(mk(4, 48)), lambda: pkg.mxfp4_quantize(mk(4, 16)),
                 lambda: pkg.mxfp4_quantize(mk(0, 32)), lambda: pkg.moe_grouped_linear_mxfp4(mk(S, K), mu(1025, N, 2, 16), mu(1025, N, 2), mi(1026))):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    # the descriptor a call builds: the packed strides are the dense ones, unused row strides too
    d = pkg.moe_mx._desc(torch.zeros(3, 96, dtype=torch.float16), 3, 4, 96, 24, ld_x=99, ld_y=32)
    assert [getattr(d, n) for n, _ in d._fields_[:-1]] == [1, 3, 4, 96, 24, 99, 32, 24, 48, 3, 0] and tuple(d.reserved) == (0,) * 5


# ---- the reference against statements that do not share its code ------------------------------------------------------------------------
E2M1 = {0: 0.0, 1: 0.5, 2: 1.0, 3: 1.5, 4: 2.0, 5: 3.0, 6: 4.0, 7: 6.0}


def test_reference_table_covers_the_16_codes():
    for c in range(16):
        sign, ex, man = c >> 3, (c >> 1) & 3, c & 1
        want = (-1.0) ** sign * (man * 0.5 if ex == 0 else 2.0 ** (ex - 1) * (1 + man / 2))      # E2M1, bias 1
        assert mx_ref.VALUES[c] == want == (-1.0) ** sign * E2M1[c & 7] and np.signbit(mx_ref.VALUES[c]) == bool(sign), c
    blocks = np.arange(16, dtype=np.uint8).reshape(1, 16) * 17                                   # byte j: code j in both nibbles
    for e in (0, 1, 126, 127, 128, 254):
        got = mx_ref.dequant64(blocks, np.array([e], np.uint8))
        np.testing.assert_array_equal(got, np.repeat(mx_ref.VALUES, 2) * 2.0 ** (e - 127))
    assert np.isnan(mx_ref.dequant64(blocks, np.array([255], np.uint8))).all()
    flat = mx_ref.dequant64(np.arange(32, dtype=np.uint8).reshape(1, 32), np.array([[127, 128]], np.uint8))  # [..., K/2] beside [..., K/32]
    assert flat.shape == (1, 64) and flat[0, 2] == 0.5 and flat[0, 3] == 0.0 and flat[0, 32] == 0.0 and flat[0, 33] == 1.0  # byte 16 = 0x10
    # rounding to a type: exact in fp32 and bf16 below the overflow, Inf above it, subnormals kept, f16 rounds to nearest even
    one = lambda c, e, dt: mx_ref.dequant(np.full((1, 16), c, np.uint8), np.array([e], np.uint8), dt)[0]
    assert one(7, 252, "f32") == 6 * 2.0 ** 125 and one(6, 253, "f32") == np.inf and one(5, 253, "bf16") == 3 * 2.0 ** 126
    assert one(4, 254, "bf16") == np.inf and one(12, 254, "f32") == -np.inf and one(3, 254, "f32") == 1.5 * 2.0 ** 127
    assert one(1, 0, "f32") == 2.0 ** -128 and one(3, 0, "bf16") == 1.5 * 2.0 ** -127 and one(1, 0, "f16") == 0
    assert one(7, 140, "f16") == 49152 and one(7, 141, "f16") == np.inf and one(2, 142, "f16") == 32768 and one(2, 143, "f16") == np.inf
    assert one(3, 103, "f16") == 2.0 ** -23 and one(5, 102, "f16") == 2.0 ** -23 and one(1, 104, "f16") == 2.0 ** -24 and one(1, 103, "f16") == 0
    assert np.signbit(one(9, 100, "f16"))


def _blocks_with(seed, top, n=64):
    """n random blocks whose largest magnitude code is `top`"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, top + 1, size=(n, 32)).astype(np.uint8) | (rng.integers(0, 2, size=(n, 32)).astype(np.uint8) << 3)
    codes[np.arange(n), rng.integers(0, 32, size=n)] = top
    return mx_ref.pack(codes), rng.integers(1, 253, size=n).astype(np.uint8)


@pytest.mark.parametrize("top", [6, 7])
def test_quant_inverts_dequant(top):
    """a block whose largest magnitude is 4 or 6 has floor(log2(amax)) - 2 = its own scale, and every value is a grid point"""
    blocks, scales = _blocks_with(top, top)
    got = mx_ref.quant(mx_ref.dequant64(blocks, scales))
    np.testing.assert_array_equal(got[0], blocks), np.testing.assert_array_equal(got[1], scales)
    for dt in ("f32", "bf16"):                                               # the rounded values are the same numbers
        again = mx_ref.quant(mx_ref.dequant(blocks, scales, dt))
        np.testing.assert_array_equal(again[0], blocks), np.testing.assert_array_equal(again[1], scales)


def test_quant_of_zero_blocks_ties_saturation_and_non_finite_blocks():
    zeros = mx_ref.pack(np.tile(np.array([0, 8], np.uint8), (3, 16)))
    got = mx_ref.quant(mx_ref.dequant64(zeros, np.zeros(3, np.uint8)))
    np.testing.assert_array_equal(got[0], zeros), np.testing.assert_array_equal(got[1], np.zeros(3, np.uint8))
    # the seven tie points beside a 6 that fixes the scale at 2^0: each lands on the even code
    x = np.zeros((2, 32))
    x[0, :8] = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0]
    x[1] = -x[0]
    blocks, scales = mx_ref.quant(x * 2.0 ** 10)
    codes = mx_ref.unpack(blocks)[:, 0]
    assert list(codes[0, :8]) == [0, 2, 2, 4, 4, 6, 6, 7] and list(codes[1, :8]) == [8, 10, 10, 12, 12, 14, 14, 15] and scales.tolist() == [[137], [137]]
    x[0, 8:15], x[0, 16:23] = np.nextafter(x[0, :7], 8.0), np.nextafter(x[0, :7], 0.0)      # the neighbours of a tie are no ties
    codes = mx_ref.unpack(mx_ref.quant(x[:1])[0])[0, 0]
    assert list(codes[8:15]) == [1, 2, 3, 4, 5, 6, 7] and list(codes[16:23]) == [0, 1, 2, 3, 4, 5, 6]
    # saturation: amax = 7.5 has floor(log2) = 2, so 7.5 / 2^0 is above 6 and stays 6; the largest finite fp32 inputs have the scale byte 252
    sat = np.zeros((2, 32))
    sat[0, :3], sat[1, :2] = [7.5, -7.9, 6.5], [2.0 ** 127 * 1.9, -2.0 ** 126]
    blocks, scales = mx_ref.quant(sat)
    assert list(mx_ref.unpack(blocks)[0, 0, :3]) == [7, 15, 7] and scales[0, 0] == 127
    assert list(mx_ref.unpack(blocks)[1, 0, :2]) == [7, 12] and scales[1, 0] == 252
    tiny = np.zeros((1, 32))
    tiny[0, :2] = [2.0 ** -149, 2.0 ** -140]                                 # the scale clamps at byte 0
    blocks, scales = mx_ref.quant(tiny)
    assert scales[0, 0] == 0 and list(mx_ref.unpack(blocks)[0, 0, :2]) == [0, 0]
    # a block with an Inf or a NaN: scale byte 255, all codes 0; its neighbour is untouched
    bad = np.ones((3, 64))
    bad[0, 5], bad[1, 40], bad[2, 63] = np.inf, np.nan, -np.inf
    blocks, scales = mx_ref.quant(bad)
    assert scales.tolist() == [[255, 125], [125, 255], [125, 255]]
    assert not blocks[0, 0].any() and not blocks[1, 1].any() and (blocks[0, 1] == 0x66).all() and (blocks[2, 0] == 0x66).all()
