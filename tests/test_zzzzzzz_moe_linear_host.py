"""CPU tests of the expert linear layers (include/nnop_hip_moe_linear.h): the sixth library loads and exports exactly its header's
functions, links none of the other five, its header is plain C99 and its descriptor matches the ctypes one, the frozen boundaries of the
other five libraries still hold, every entry point validates in the header's order and returns before any launch, the Python wrappers
raise before any device work, the reference the GPU tests are judged against (tests/moe_linear_ref.py) agrees with a per-expert torch
fp64 loop and its autograd in both layouts, and each derived gate passes fp32 evaluations and fails wrong ones.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import moe_linear_ref as ref
from abi_util import ROOT, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_moe_linear.h")
NAMES = {"nnop_moe_linear_abi_version", "nnop_moe_linear", "nnop_moe_linear_bwd_x", "nnop_moe_linear_bwd_w", "nnop_moe_linear_bwd_b"}
PY_NAMES = ("moe_grouped_linear", "_moe_grouped_linear", "grad_moe_grouped_linear", "moe_grouped_linear_into",
            "grad_moe_grouped_linear_x_into", "grad_moe_grouped_linear_w_into", "grad_moe_grouped_linear_b_into")
# entry point -> (number of pointers, alignment of each as ("t" = dtype, "g" = grad_dtype, 4), the optional positions)
ENTRY = {"nnop_moe_linear": (5, ("t", "t", "t", "t", 4), (3,)), "nnop_moe_linear_bwd_x": (4, ("t", "t", "t", 4), ()),
         "nnop_moe_linear_bwd_w": (4, ("g", "t", "t", 4), ()), "nnop_moe_linear_bwd_b": (3, ("g", "t", 4), ())}
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
at = lambda off: C.c_void_p(0x7f0000001000 + off)
FIELDS = ["dtype", "grad_dtype", "rows", "experts", "in_dim", "out_dim", "ld_x", "ld_y", "ld_w", "ld_dw", "ld_b", "ld_db", "flags", "reserved"]


# ---- the library and its header -----------------------------------------------------------------------------------------------------
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_exactly_the_headers_functions(pkg):
    M = pkg._lib_moe_linear
    lib = M.load()
    assert set(M.EXPORTED_SYMBOLS) == NAMES
    assert _defined(M.LIB_PATH) == NAMES
    header = strip_c_comments(open(HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header)) == NAMES
    assert lib.nnop_moe_linear_abi_version() == M.MOE_LINEAR_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_LINEAR_ABI_VERSION (\d+)", header).group(1)) == 1
    assert (int(re.search(r"#define NNOP_MOE_LINEAR_KN (\d+)u", header).group(1)), M.KN) == (1, 1)
    assert (int(re.search(r"#define NNOP_MOE_LINEAR_ACCUMULATE (\d+)u", header).group(1)), M.ACCUMULATE) == (2, 2)
    needed = subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip" not in needed                               # none of the other five libraries
    for name in PY_NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name)) and name in pkg.moe_linear.__all__
    assert "moe_linear" in pkg.__all__ and "_lib_moe_linear" in pkg.__all__


def test_the_other_five_boundaries_are_unchanged(pkg):
    assert pkg._lib.ABI_VERSION == 7 and len(pkg._lib.EXPORTED_SYMBOLS) == 30
    assert pkg._lib_ext.EXT_ABI_VERSION == 1 and len(pkg._lib_ext.EXPORTED_SYMBOLS) == 4
    assert pkg._lib_moe.MOE_ABI_VERSION == 1 and len(pkg._lib_moe.EXPORTED_SYMBOLS) == 5
    assert pkg._lib_moe_data.MOE_DATA_ABI_VERSION == 1 and len(pkg._lib_moe_data.EXPORTED_SYMBOLS) == 5
    assert pkg._lib_moe_gemm.MOE_GEMM_ABI_VERSION == 1 and len(pkg._lib_moe_gemm.EXPORTED_SYMBOLS) == 4
    others = (pkg._lib, pkg._lib_ext, pkg._lib_moe, pkg._lib_moe_data, pkg._lib_moe_gemm)
    for M in others:
        lib = M.load()
        for name in NAMES:
            assert name not in M.EXPORTED_SYMBOLS and not hasattr(lib, name)
    for M in others[1:]:
        assert _defined(M.LIB_PATH) == set(M.EXPORTED_SYMBOLS)
    assert not NAMES & _defined(pkg._lib.LIB_PATH)
    assert C.sizeof(pkg._lib_moe_gemm.MoeGemmDesc) == 40               # the fifth descriptor, its reserved words still reserved
    for h in ("nnop_hip.h", "nnop_hip_ext.h", "nnop_hip_moe.h", "nnop_hip_moe_data.h", "nnop_hip_moe_gemm.h"):
        text = strip_c_comments(open(os.path.join(ROOT, "include", h)).read())
        assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES) and "nnop_moe_linear_desc" not in text


def test_descriptor_matches_the_header(pkg):
    D = pkg._lib_moe_linear.MoeLinearDesc
    body = re.search(r"typedef struct nnop_moe_linear_desc \{(.*?)\} nnop_moe_linear_desc;", strip_c_comments(open(HEADER).read()), re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(u?int32_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), int(m.group(2) or 1), C.c_uint32 if ctype[0] == "u" else C.c_int32))
    assert C.sizeof(D) == 64
    assert [f[:2] for f in fields] == [(n, getattr(t, "_length_", 1)) for n, t in D._fields_]
    assert [f[0] for f in fields] == FIELDS
    assert [f[2] for f in fields] == [(t._type_ if hasattr(t, "_length_") else t) for _, t in D._fields_]
    assert D.reserved.offset == 52 and D.flags.offset == 48
    assert (pkg._lib_moe_linear.MAX_EXPERTS, pkg._lib_moe_linear.MAX_DIM) == (1024, 65536)


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe_linear.h"\n'
                 "int main(void){ nnop_moe_linear_desc r; r.flags = NNOP_MOE_LINEAR_KN | NNOP_MOE_LINEAR_ACCUMULATE;\n"
                 "  return (sizeof(r) == 64 && r.flags == 3u && NNOP_HIP_MOE_LINEAR_ABI_VERSION == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_missing_or_mismatched_library_fails_loudly(pkg, monkeypatch):
    M = pkg._lib_moe_linear
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "MOE_LINEAR_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="moe-linear-ABI version 1"):
        M.load()
    monkeypatch.setattr(M, "MOE_LINEAR_ABI_VERSION", 1)
    monkeypatch.setattr(M, "EXPORTED_SYMBOLS", M.EXPORTED_SYMBOLS + ("nnop_moe_linear_not_there",))
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="does not export nnop_moe_linear_not_there"):
        M.load()
    monkeypatch.setattr(M, "LIB_PATH", "/nonexistent/libnnop_hip_moe_linear.so")
    with pytest.raises(ImportError, match="no CPU or PyTorch fallback"):
        M.load()


def test_the_bindings_glue_holds_for_the_sixth_library(pkg):
    """what tests/test_zzzzzz_bindings_host.py asks of the other five bindings and operator modules"""
    M, common, module = pkg._lib_moe_linear, pkg._common, pkg.moe_linear
    lib = M.load()
    assert M.load() is lib is M._lib and M.EXPORTED_SYMBOLS == tuple(M.PROTOTYPES)
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
    assert module.NNopError is common.NNopError and module._DTYPES is common._DTYPES
    for name in ("_ptr", "_stream", "_on_device", "_raise", "_launch", "_dtype_name"):
        assert vars(module).get(name, getattr(common, name)) is getattr(common, name), name
    assert "_ptr" in vars(module)


# ---- validation: order and codes, before any launch -------------------------------------------------------------------------------------
def _desc(pkg, reserved=(0, 0, 0), **kw):
    base = dict(dtype=2, grad_dtype=2, rows=256, experts=8, in_dim=128, out_dim=64, ld_x=128, ld_y=64, ld_w=128, ld_dw=128, ld_b=64, ld_db=64,
                flags=0)
    base.update(kw)
    d = pkg._lib_moe_linear.MoeLinearDesc(**base)
    d.reserved[0], d.reserved[1], d.reserved[2] = reserved
    return d


def _call(lib, name, d, ptrs=None):
    return getattr(lib, name)(C.byref(d) if d is not None else None, *(ptrs or [OK] * ENTRY[name][0]), None)


def _all(lib, d, ptr=None):
    return [_call(lib, name, d, None if ptr is None else [ptr] * ENTRY[name][0]) for name in ENTRY]


KN_OK = dict(flags=1, ld_w=64, ld_dw=64)                               # [E][K][N]: a weight row has N = 64 elements


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(grad_dtype=1), "NNOP_ERR_DTYPE"),                          # f16 gradients beside bf16 operands
    (dict(dtype=0, grad_dtype=2), "NNOP_ERR_DTYPE"),                 # 16-bit gradients beside fp32 operands
    (dict(grad_dtype=7), "NNOP_ERR_DTYPE"),
    (dict(flags=4), "NNOP_ERR_OPTS"),
    (dict(flags=0x80000001), "NNOP_ERR_OPTS"),
    (dict(reserved=(1, 0, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, -1, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, 0, 7)), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-3), "NNOP_ERR_SHAPE"),
    (dict(experts=0), "NNOP_ERR_SHAPE"),
    (dict(experts=1025), "NNOP_ERR_SHAPE"),
    (dict(in_dim=0), "NNOP_ERR_SHAPE"),
    (dict(out_dim=0), "NNOP_ERR_SHAPE"),
    (dict(in_dim=65537, ld_x=65537, ld_w=65537, ld_dw=65537), "NNOP_ERR_SHAPE"),
    (dict(out_dim=65537, ld_y=65537, ld_b=65537, ld_db=65537), "NNOP_ERR_SHAPE"),
    (dict(ld_x=127), "NNOP_ERR_SHAPE"),                              # ld = dim - 1, each stride
    (dict(ld_y=63), "NNOP_ERR_SHAPE"),
    (dict(ld_w=127), "NNOP_ERR_SHAPE"),
    (dict(ld_dw=127), "NNOP_ERR_SHAPE"),
    (dict(ld_b=63), "NNOP_ERR_SHAPE"),
    (dict(ld_db=63), "NNOP_ERR_SHAPE"),
    (dict(KN_OK, ld_w=63), "NNOP_ERR_SHAPE"),                        # with KN a weight row has N elements ...
    (dict(KN_OK, ld_dw=63), "NNOP_ERR_SHAPE"),
    (dict(in_dim=64, out_dim=128, ld_x=64, ld_y=128, ld_b=128, ld_db=128, ld_w=64, ld_dw=64, flags=1), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, flags=8, rows=0), "NNOP_ERR_DTYPE"),
    (dict(grad_dtype=1, reserved=(5, 0, 0), rows=0), "NNOP_ERR_DTYPE"),
    (dict(reserved=(0, 3, 0), rows=0), "NNOP_ERR_OPTS"),
    (dict(flags=16, in_dim=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_linear.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert _all(lib, d) == [want] * 4
    assert _all(lib, d, NULL) == [want] * 4                          # the descriptor is judged before the pointers
    assert _all(lib, d, at(1)) == [want] * 4


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    lib, L = pkg._lib_moe_linear.load(), pkg._lib
    one = dict(rows=1, experts=1, in_dim=1, out_dim=1, ld_x=1, ld_y=1, ld_w=1, ld_dw=1, ld_b=1, ld_db=1)
    for ok in (dict(), dict(dtype=0, grad_dtype=0), dict(dtype=1, grad_dtype=1), dict(grad_dtype=0), dict(dtype=1, grad_dtype=0), one,
               dict(one, flags=3), dict(experts=1024), dict(flags=1, ld_w=64, ld_dw=64), dict(flags=2), dict(flags=3, ld_w=64, ld_dw=70),
               dict(in_dim=65536, ld_x=65536, ld_w=65536, ld_dw=65536), dict(out_dim=65536, ld_y=65536, ld_b=65536, ld_db=65536),
               dict(in_dim=7, out_dim=5, ld_x=10, ld_y=5, ld_w=7, ld_dw=9, ld_b=5, ld_db=6),
               dict(rows=2 ** 31 - 1, in_dim=8, out_dim=8, ld_x=8, ld_y=8, ld_w=8, ld_dw=8, ld_b=8, ld_db=8)):
        d = _desc(pkg, **ok)
        assert _all(lib, d, NULL) == [L.NNOP_ERR_NULL] * 4, ok
    assert _all(lib, None) == [L.NNOP_ERR_NULL] * 4                  # the descriptor itself: first of all
    assert _all(lib, None, at(1)) == [L.NNOP_ERR_NULL] * 4


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe_linear.load(), pkg._lib
    for dtype, grad in ((0, 0), (1, 1), (2, 2), (1, 0), (2, 0)):
        size = {"t": 4 if dtype == 0 else 2, "g": 4 if grad == 0 else 2, 4: 4}
        d = _desc(pkg, dtype=dtype, grad_dtype=grad)
        for name, (n, aligns, optional) in ENTRY.items():
            for pos, a in enumerate(aligns):
                b = [OK] * n
                b[pos] = NULL
                c = [at(1)] * n                                      # NULL is judged before alignment
                c[pos] = NULL
                if pos in optional:                                  # bias: NULL means none, so the call goes on to the next check
                    assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos)
                else:
                    assert _call(lib, name, d, b) == L.NNOP_ERR_NULL, (name, pos)
                    assert _call(lib, name, d, c) == L.NNOP_ERR_NULL, (name, pos)
                c = [OK] * n
                c[pos] = at(size[a] // 2)                            # aligned to half of what is needed
                assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos, a)
                if size[a] == 4 and a == "g" and dtype != 0:         # an fp32 gradient is judged by its own element size
                    c[pos] = at(2)
                    assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos)


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    S, E, N, K = 10, 3, 6, 8
    f = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt)
    xs, ys, w, wk, b, off = f(S, K), f(S, N), f(E, N, K), f(E, K, N), f(E, N), torch.zeros(E + 1, dtype=torch.int32)
    for call in (lambda: pkg.moe_grouped_linear(xs, w, off), lambda: pkg._moe_grouped_linear(xs, wk, off, b, layout="kn"),
                 lambda: pkg.moe_grouped_linear_into(ys, xs, w, off, b), lambda: pkg.grad_moe_grouped_linear(ys, xs, w, off),
                 lambda: pkg.grad_moe_grouped_linear_x_into(xs, ys, wk, off, layout="kn"),
                 lambda: pkg.grad_moe_grouped_linear_w_into(w, ys, xs, off), lambda: pkg.grad_moe_grouped_linear_b_into(b, ys, off),
                 lambda: pkg.moe_grouped_linear(xs.clone().requires_grad_(True), w, off, b),
                 lambda: pkg.moe_grouped_linear(xs, w, off, b.clone().requires_grad_(True))):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    mi = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnGpu)
    xs, ys, w, wk, b, off = mk(S, K), mk(S, N), mk(E, N, K), mk(E, K, N), mk(E, N), mi(E + 1)
    h = lambda *s: mk(*s, dt=torch.bfloat16)
    # wrong types
    for call in (lambda: pkg.moe_grouped_linear(mk(S, K, dt=torch.float64), w, off), lambda: pkg.moe_grouped_linear(xs, w, off, [1.0]),
                 lambda: pkg.moe_grouped_linear(xs, w, off, mi(E, N)), lambda: pkg.moe_grouped_linear(xs, w, off.long()),
                 lambda: pkg.grad_moe_grouped_linear_b_into(mi(E, N), ys, off), lambda: pkg.grad_moe_grouped_linear_b_into(b, ys, mk(E + 1)),
                 lambda: pkg.grad_moe_grouped_linear_w_into(mi(E, N, K), ys, xs, off)):
        with pytest.raises(TypeError):
            call()
    # a layout that is none; types that differ; shapes that do not fit the layout; outputs of the wrong type, shape or stride
    for bad in (lambda: pkg.moe_grouped_linear(xs, w, off, layout="NK"), lambda: pkg.grad_moe_grouped_linear(ys, xs, w, off, layout="tn"),
                lambda: pkg.grad_moe_grouped_linear_w_into(w, ys, xs, off, layout=None),
                lambda: pkg.moe_grouped_linear(xs, h(E, N, K), off), lambda: pkg.moe_grouped_linear(xs, w, off, h(E, N)),
                lambda: pkg.moe_grouped_linear(xs, wk, off), lambda: pkg.moe_grouped_linear(xs, w, off, layout="kn"),
                lambda: pkg.moe_grouped_linear(xs, w, off, mk(E, N + 1)), lambda: pkg.moe_grouped_linear(xs, w, off, mk(E + 1, N)),
                lambda: pkg.moe_grouped_linear(xs, w, off, mk(N)), lambda: pkg.moe_grouped_linear(xs, w, mi(E)),
                lambda: pkg.moe_grouped_linear_into(mk(S, N + 1), xs, w, off), lambda: pkg.moe_grouped_linear_into(mk(N, S).t(), xs, w, off),
                lambda: pkg.grad_moe_grouped_linear_x_into(mk(S, K + 1), ys, w, off),
                lambda: pkg.grad_moe_grouped_linear_x_into(xs, ys, w, off, layout="kn"),
                lambda: pkg.grad_moe_grouped_linear_w_into(wk, ys, xs, off), lambda: pkg.grad_moe_grouped_linear_w_into(w, ys, xs, off, layout="kn"),
                lambda: pkg.grad_moe_grouped_linear_w_into(mk(E, K, N).transpose(1, 2), ys, xs, off),
                lambda: pkg.grad_moe_grouped_linear_w_into(h(E, N, K), ys, xs, off),                     # 16-bit dw beside fp32 operands
                lambda: pkg.grad_moe_grouped_linear_w_into(mk(E, N, K, dt=torch.float16), h(S, N), h(S, K), off),
                lambda: pkg.grad_moe_grouped_linear_b_into(h(E, N), ys, off), lambda: pkg.grad_moe_grouped_linear_b_into(mk(E, N + 1), ys, off),
                lambda: pkg.grad_moe_grouped_linear_b_into(mk(N, E).t(), ys, off), lambda: pkg.grad_moe_grouped_linear_b_into(mk(E + 1, N), ys, off),
                lambda: pkg.grad_moe_grouped_linear(ys, xs, w, off, out=(None, None, mk(E, N + 1))),
                lambda: pkg.grad_moe_grouped_linear(ys, xs, wk, off, layout="kn", out=(None, mk(E, N, K), None)),
                lambda: pkg.grad_moe_grouped_linear(ys, xs, w, off, accumulate=True),
                lambda: pkg.grad_moe_grouped_linear(ys, xs, w, off, out=(None, w, None), accumulate=True)):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    for call in (lambda: pkg.moe_grouped_linear(mk(0, K), w, off, b), lambda: pkg.grad_moe_grouped_linear_b_into(mk(1025, N), ys, mi(1026)),
                 lambda: pkg.grad_moe_grouped_linear_b_into(mk(E, 0), mk(S, 0), off)):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    # the descriptor a call builds: unused strides are the dense ones, the flags follow layout and accumulate
    G = pkg.moe_linear
    d = G._desc(torch.zeros(3, 60, dtype=torch.bfloat16), 3, 4, 60, 24, True, ld_x=63, ld_y=32, ld_dw=40, grad=torch.zeros(1), accumulate=True)
    assert [getattr(d, n) for n in FIELDS[:-1]] == [2, 0, 3, 4, 60, 24, 63, 32, 24, 40, 24, 24, 3] and tuple(d.reserved) == (0, 0, 0)
    d = G._desc(torch.zeros(3, 60), 3, 4, 60, 24, False)
    assert [getattr(d, n) for n in FIELDS[:-1]] == [0, 0, 3, 4, 60, 24, 60, 24, 60, 60, 24, 24, 0]


# ---- the reference against an independent statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("counts,lead,tail,K,N", [([3, 0, 5, 1], 0, 0, 7, 5), ([0, 0, 4], 2, 3, 8, 3), ([6], 0, 1, 4, 9), ([0, 2, 0], 0, 0, 3, 3)])
def test_reference_matches_a_torch_loop_and_its_autograd(counts, lead, tail, K, N, layout):
    off = ref.offsets_of(counts, lead)
    S, E = int(off[-1]) + tail, len(counts)
    rng = np.random.default_rng(S + K)
    xs, dys, b = rng.standard_normal((S, K)), rng.standard_normal((S, N)), rng.standard_normal((E, N))
    w = rng.standard_normal((E, N, K) if layout == "nk" else (E, K, N))
    lx, lw, lb = (torch.tensor(a, requires_grad=True) for a in (xs, w, b))
    mm = (lambda e: lx[off[e]:off[e + 1]] @ lw[e].T + lb[e]) if layout == "nk" else (lambda e: lx[off[e]:off[e + 1]] @ lw[e] + lb[e])
    ys_t = torch.cat([torch.zeros(lead, N, dtype=torch.float64)] + [mm(e) for e in range(E)] + [torch.zeros(tail, N, dtype=torch.float64)])
    ys, A, B = ref.linear_ref(xs, w, off, b, layout)
    np.testing.assert_allclose(ys, ys_t.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert (A + B >= np.abs(ys) - 1e-12).all() and (B[:lead] == 0).all() and (B[S - tail:] == 0).all() and (ys[S - tail:] == 0).all()
    e_of = ref.rows_of(off, S)
    np.testing.assert_allclose(ref.linear_ref(xs, w, off, None, layout)[0] + np.where(e_of[:, None] >= 0, b[e_of], 0), ys, rtol=1e-13, atol=1e-15)
    ys_t.backward(torch.tensor(dys))
    dxs, Ax = ref.bwd_x_ref(dys, w, off, layout)
    np.testing.assert_allclose(dxs, lx.grad.numpy(), rtol=1e-13, atol=1e-15)
    dw, Aw, R = ref.bwd_w_ref(dys, xs, off, layout)
    assert dw.shape == w.shape == Aw.shape
    np.testing.assert_allclose(dw, lw.grad.numpy(), rtol=1e-13, atol=1e-15)
    db, Ab, Rb = ref.bwd_b_ref(dys, off)
    np.testing.assert_allclose(db, lb.grad.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(R.reshape(-1), counts), np.testing.assert_array_equal(Rb.reshape(-1), counts)
    assert (Ab >= np.abs(db) - 1e-12).all() and all((db[e] == 0).all() and (dw[e] == 0).all() for e in range(E) if counts[e] == 0)


# ---- the gates -------------------------------------------------------------------------------------------------------------------
def _share(r):
    return float((r > 1.0).mean())


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(37, 24, 8), (129, 72, 520), (33, 5, 7), (65, 40, 40)])
def test_the_forward_gate(dt, M, N, K, layout):
    off = ref.offsets_of([M // 3, M - 2 * (M // 3), M // 3])
    xs, b = ref.make(1, (M, K), dt), ref.make(3, (3, N), dt)
    w = ref.make(2, (3, N, K) if layout == "nk" else (3, K, N), dt)
    want, A, B = ref.linear_ref(xs, w, off, b, layout)
    ratios = lambda got: ref.fwd_ratios(got, want, A, B, K, dt)
    for order in ("blas", "sequential"):
        assert ratios(ref.linear_f32(xs, w, off, dt, b, layout, order)).max() <= 1.0, order
    assert _share(ratios(ref.linear_f32(xs, w, off, dt, b, layout, bias_mode="omit"))) > 0.5           # bias omitted
    assert _share(ratios(ref.linear_f32(xs, w, off, dt, b, layout, bias_mode="next"))) > 0.5           # bias of expert e + 1
    assert _share(ratios(ref.linear_f32(xs, w, off, dt, b, layout, short=min(8, K - 1)))) > 0.5        # the last terms dropped
    if K == N:                                                                                         # the weights read in the other layout
        assert _share(ratios(ref.linear_f32(xs, w, off, dt, b, "kn" if layout == "nk" else "nk"))) > 0.5
    # without a bias the gate is moe_gemm_ref's with one unit more
    want0, A0, B0 = ref.linear_ref(xs, w, off, None, layout)
    assert not B0.any() and ref.fwd_ratios(ref.linear_f32(xs, w, off, dt, None, layout), want0, A0, B0, K, dt).max() <= 1.0


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("dt,gdt", [("f32", "f32"), ("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("bf16", "f32")])
def test_the_gradient_gates(dt, gdt, layout):
    counts, N, K = [40, 0, 129, 23], 40, 40
    off = ref.offsets_of(counts)
    S, own = int(off[-1]), [0, 2, 3]
    xs, dys = ref.make(1, (S, K), dt), ref.make(3, (S, N), dt)
    old_w = ref.round_to(4 * ref.make(4, (4, N, K), "f32"), gdt)
    old_b = ref.round_to(8 * ref.make(5, (4, N), "f32"), gdt)
    dw, Aw, R = ref.bwd_w_ref(dys, xs, off, layout)
    db, Ab, Rb = ref.bwd_b_ref(dys, off)
    for order in ("blas", "sequential"):
        assert ref.grad_ratios(ref.bwd_w_f32(dys, xs, off, gdt, layout, order), dw, Aw, R, gdt).max() <= 1.0
        assert ref.grad_ratios(ref.bwd_b_f32(dys, off, gdt, order), db, Ab, Rb, gdt).max() <= 1.0
        assert ref.grad_ratios(ref.bwd_w_f32(dys, xs, off, gdt, layout, order, old=old_w), old_w + dw, Aw, R, gdt, old_w).max() <= 1.0
        assert ref.grad_ratios(ref.bwd_b_f32(dys, off, gdt, order, old=old_b), old_b + db, Ab, Rb, gdt, old_b).max() <= 1.0
    wrong_w = lambda **kw: ref.grad_ratios(ref.bwd_w_f32(dys, xs, off, gdt, layout, **kw), old_w + dw, Aw, R, gdt, old_w)[own]
    wrong_b = lambda **kw: ref.grad_ratios(ref.bwd_b_f32(dys, off, gdt, **kw), old_b + db, Ab, Rb, gdt, old_b)[own]
    for mode in ("omit", "twice"):                                                                     # old not added, old added twice
        assert _share(wrong_w(old=old_w, old_mode=mode)) > 0.5 and _share(wrong_b(old=old_b, old_mode=mode)) > 0.5
    assert _share(wrong_w(old=old_w, short=8)) > 0.5 and _share(wrong_b(old=old_b, short=8)) > 0.5      # the last 8 rows dropped
    assert _share(ref.grad_ratios(ref.bwd_w_f32(dys, xs, off, gdt, layout, short=8), dw, Aw, R, gdt)[own]) > 0.5
    assert _share(ref.grad_ratios(ref.bwd_b_f32(dys, off, gdt, short=8), db, Ab, Rb, gdt)[own]) > 0.5
    other = "kn" if layout == "nk" else "nk"                                                           # dw stored in the other layout (K = N)
    assert _share(ref.grad_ratios(ref.bwd_w_f32(dys, xs, off, gdt, other), dw, Aw, R, gdt)[own]) > 0.5
    # an expert without rows: +0 when stored, untouched when accumulated
    assert (ref.bwd_w_f32(dys, xs, off, gdt, layout)[1] == 0).all() and (ref.bwd_b_f32(dys, off, gdt)[1] == 0).all()
    np.testing.assert_array_equal(ref.bwd_w_f32(dys, xs, off, gdt, layout, old=old_w)[1], old_w[1])
    bad = ref.bwd_b_f32(dys, off, gdt)
    bad[0, 0] = float("nan")
    assert ref.grad_ratios(bad, db, Ab, Rb, gdt).max() == float("inf")
