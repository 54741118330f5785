"""CPU tests of the grouped expert GEMM (include/nnop_hip_moe_gemm.h): the fifth library loads and exports exactly its header's functions,
links none of the other four, its header is plain C99 and its descriptor matches the ctypes one, the frozen boundaries of the other four
libraries still hold, every entry point validates in the header's order and returns before any launch, the Python wrappers raise before
any device work, the reference the GPU tests are judged against (tests/moe_gemm_ref.py) agrees with a per-expert torch fp64 loop and its
autograd, and the derived gate passes an fp32 evaluation and fails a wrong one.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import moe_gemm_ref as ref
from abi_util import ROOT, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_moe_gemm.h")
NAMES = {"nnop_moe_gemm_abi_version", "nnop_moe_gemm", "nnop_moe_gemm_bwd_x", "nnop_moe_gemm_bwd_w"}
PY_NAMES = ("moe_grouped_gemm", "_moe_grouped_gemm", "grad_moe_grouped_gemm", "moe_grouped_gemm_into", "grad_moe_grouped_gemm_x_into",
            "grad_moe_grouped_gemm_w_into")
ENTRY = ("nnop_moe_gemm", "nnop_moe_gemm_bwd_x", "nnop_moe_gemm_bwd_w")     # each: three arrays of `dtype`, then offsets
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
at = lambda off: C.c_void_p(0x7f0000001000 + off)


# ---- the library and its header -----------------------------------------------------------------------------------------------------
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_exactly_the_headers_functions(pkg):
    M = pkg._lib_moe_gemm
    lib = M.load()
    assert set(M.EXPORTED_SYMBOLS) == NAMES
    assert _defined(M.LIB_PATH) == NAMES
    header = strip_c_comments(open(HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header)) == NAMES
    assert lib.nnop_moe_gemm_abi_version() == M.MOE_GEMM_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_GEMM_ABI_VERSION (\d+)", header).group(1)) == 1
    needed = subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip" not in needed                               # none of the other four libraries
    for name in PY_NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert "moe_gemm" in pkg.__all__ and "_lib_moe_gemm" in pkg.__all__


def test_the_other_four_boundaries_are_unchanged(pkg):
    assert pkg._lib.ABI_VERSION == 7 and len(pkg._lib.EXPORTED_SYMBOLS) == 30
    assert pkg._lib_ext.EXT_ABI_VERSION == 1 and len(pkg._lib_ext.EXPORTED_SYMBOLS) == 4
    assert pkg._lib_moe.MOE_ABI_VERSION == 1 and len(pkg._lib_moe.EXPORTED_SYMBOLS) == 5
    assert pkg._lib_moe_data.MOE_DATA_ABI_VERSION == 1 and len(pkg._lib_moe_data.EXPORTED_SYMBOLS) == 5
    others = (pkg._lib, pkg._lib_ext, pkg._lib_moe, pkg._lib_moe_data)
    for M in others:
        lib = M.load()
        for name in NAMES:
            assert name not in M.EXPORTED_SYMBOLS and not hasattr(lib, name)
    for M in others[1:]:
        assert _defined(M.LIB_PATH) == set(M.EXPORTED_SYMBOLS)
    assert not NAMES & _defined(pkg._lib.LIB_PATH)
    for h in ("nnop_hip.h", "nnop_hip_ext.h", "nnop_hip_moe.h", "nnop_hip_moe_data.h"):
        text = strip_c_comments(open(os.path.join(ROOT, "include", h)).read())
        assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES) and "nnop_moe_gemm_desc" not in text


def test_descriptor_matches_the_header(pkg):
    D = pkg._lib_moe_gemm.MoeGemmDesc
    body = re.search(r"typedef struct nnop_moe_gemm_desc \{(.*?)\} nnop_moe_gemm_desc;", strip_c_comments(open(HEADER).read()), re.S).group(1)
    fields = []
    for names in re.findall(r"int32_t\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert C.sizeof(D) == 40
    assert fields == [(n, getattr(t, "_length_", 1)) for n, t in D._fields_]
    assert [n for n, _ in fields] == ["dtype", "rows", "experts", "in_dim", "out_dim", "ld_x", "ld_y", "ld_w", "reserved"]
    assert all((t._type_ if hasattr(t, "_length_") else t) is C.c_int32 for _, t in D._fields_)
    assert (pkg._lib_moe_gemm.MAX_EXPERTS, pkg._lib_moe_gemm.MAX_DIM) == (1024, 65536)


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe_gemm.h"\n'
                 "int main(void){ nnop_moe_gemm_desc r; (void)r;\n"
                 "  return (sizeof(r) == 40 && NNOP_HIP_MOE_GEMM_ABI_VERSION == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_missing_or_mismatched_library_fails_loudly(pkg, monkeypatch):
    M = pkg._lib_moe_gemm
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "MOE_GEMM_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="moe-gemm-ABI version 1"):
        M.load()
    monkeypatch.setattr(M, "MOE_GEMM_ABI_VERSION", 1)
    monkeypatch.setattr(M, "EXPORTED_SYMBOLS", M.EXPORTED_SYMBOLS + ("nnop_moe_gemm_not_there",))
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="does not export nnop_moe_gemm_not_there"):
        M.load()
    monkeypatch.setattr(M, "LIB_PATH", "/nonexistent/libnnop_hip_moe_gemm.so")
    with pytest.raises(ImportError, match="no CPU or PyTorch fallback"):
        M.load()


# ---- validation: order and codes, before any launch -------------------------------------------------------------------------------------
def _desc(pkg, reserved=(0, 0), **kw):
    base = dict(dtype=2, rows=256, experts=8, in_dim=128, out_dim=64, ld_x=128, ld_y=64, ld_w=128)
    base.update(kw)
    d = pkg._lib_moe_gemm.MoeGemmDesc(**base)
    d.reserved[0], d.reserved[1] = reserved
    return d


def _call(lib, name, d, ptrs=None):
    return getattr(lib, name)(C.byref(d) if d is not None else None, *(ptrs or [OK] * 4), None)


def _all(lib, d, ptr=None):
    return [_call(lib, name, d, None if ptr is None else [ptr] * 4) for name in ENTRY]


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(reserved=(1, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, -1)), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-3), "NNOP_ERR_SHAPE"),
    (dict(experts=0), "NNOP_ERR_SHAPE"),
    (dict(experts=1025), "NNOP_ERR_SHAPE"),
    (dict(in_dim=0), "NNOP_ERR_SHAPE"),
    (dict(out_dim=0), "NNOP_ERR_SHAPE"),
    (dict(in_dim=65537, ld_x=65537, ld_w=65537), "NNOP_ERR_SHAPE"),
    (dict(out_dim=65537, ld_y=65537), "NNOP_ERR_SHAPE"),
    (dict(ld_x=127), "NNOP_ERR_SHAPE"),                          # ld = dim - 1, each stride
    (dict(ld_y=63), "NNOP_ERR_SHAPE"),
    (dict(ld_w=127), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, reserved=(5, 0), rows=0), "NNOP_ERR_DTYPE"),
    (dict(reserved=(0, 3), rows=0), "NNOP_ERR_OPTS"),
    (dict(reserved=(2, 0), in_dim=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_gemm.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert _all(lib, d) == [want] * 3
    assert _all(lib, d, NULL) == [want] * 3                          # the descriptor is judged before the pointers
    assert _all(lib, d, at(1)) == [want] * 3


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    lib, L = pkg._lib_moe_gemm.load(), pkg._lib
    for ok in (dict(), dict(dtype=0), dict(dtype=1), dict(rows=1, experts=1, in_dim=1, out_dim=1, ld_x=1, ld_y=1, ld_w=1),
               dict(experts=1024), dict(in_dim=65536, ld_x=65536, ld_w=65536), dict(out_dim=65536, ld_y=65536),
               dict(in_dim=7, out_dim=5, ld_x=10, ld_y=5, ld_w=7), dict(in_dim=7, out_dim=5, ld_x=7, ld_y=13, ld_w=15),
               dict(rows=2 ** 31 - 1, in_dim=8, out_dim=8, ld_x=8, ld_y=8, ld_w=8)):
        d = _desc(pkg, **ok)
        assert _all(lib, d, NULL) == [L.NNOP_ERR_NULL] * 3, ok
    assert _all(lib, None) == [L.NNOP_ERR_NULL] * 3                  # the descriptor itself: first of all
    assert _all(lib, None, at(1)) == [L.NNOP_ERR_NULL] * 3


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe_gemm.load(), pkg._lib
    for dtype in (0, 1, 2):
        es = 4 if dtype == 0 else 2
        d = _desc(pkg, dtype=dtype)
        aligns = [es, es, es, 4]
        for name in ENTRY:
            for pos, a in enumerate(aligns):
                b = [OK] * 4
                b[pos] = NULL                                        # none is optional
                assert _call(lib, name, d, b) == L.NNOP_ERR_NULL, (name, pos)
                c = [at(1)] * 4                                      # NULL is judged before alignment
                c[pos] = NULL
                assert _call(lib, name, d, c) == L.NNOP_ERR_NULL, (name, pos)
                c = [OK] * 4
                c[pos] = at(a // 2)                                  # aligned to half of what is needed
                assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos, a)


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    S, E, N, K = 10, 3, 6, 8
    f = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt)
    xs, ys, w, off = f(S, K), f(S, N), f(E, N, K), torch.zeros(E + 1, dtype=torch.int32)
    for call in (lambda: pkg.moe_grouped_gemm(xs, w, off), lambda: pkg._moe_grouped_gemm(xs, w, off),
                 lambda: pkg.moe_grouped_gemm_into(ys, xs, w, off), lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, off),
                 lambda: pkg.grad_moe_grouped_gemm_x_into(xs, ys, w, off), lambda: pkg.grad_moe_grouped_gemm_w_into(w, ys, xs, off),
                 lambda: pkg.moe_grouped_gemm(xs.clone().requires_grad_(True), w, off),
                 lambda: pkg.moe_grouped_gemm(xs, w.clone().requires_grad_(True), off)):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    mi = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnGpu)
    xs, ys, w, off = mk(S, K), mk(S, N), mk(E, N, K), mi(E + 1)
    h = lambda *s: mk(*s, dt=torch.bfloat16)
    # wrong types: arrays that are no float32 / float16 / bfloat16, offsets that is not int32
    for call in (lambda: pkg.moe_grouped_gemm(mk(S, K, dt=torch.float64), w, off), lambda: pkg.moe_grouped_gemm([1.0], w, off),
                 lambda: pkg.moe_grouped_gemm(xs, mk(E, N, K, dt=torch.float64), off), lambda: pkg.moe_grouped_gemm(xs, w, off.long()),
                 lambda: pkg.moe_grouped_gemm(xs, w, mk(E + 1)), lambda: pkg.moe_grouped_gemm_into(mi(S, N), xs, w, off),
                 lambda: pkg.grad_moe_grouped_gemm(mi(S, N), xs, w, off), lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, mk(E + 1)),
                 lambda: pkg.grad_moe_grouped_gemm_x_into(xs, ys, w, off.long()),
                 lambda: pkg.grad_moe_grouped_gemm_w_into(mi(E, N, K), ys, xs, off)):
        with pytest.raises(TypeError):
            call()
    # element types that differ between the arrays of one call; offsets of the wrong length; w and the rows of shapes that do not fit
    for bad in (lambda: pkg.moe_grouped_gemm(xs, h(E, N, K), off), lambda: pkg.moe_grouped_gemm(h(S, K), w, off),
                lambda: pkg.moe_grouped_gemm_into(h(S, N), xs, w, off), lambda: pkg.grad_moe_grouped_gemm(h(S, N), xs, w, off),
                lambda: pkg.grad_moe_grouped_gemm(ys, h(S, K), w, off),
                lambda: pkg.moe_grouped_gemm(xs, w, mi(E)), lambda: pkg.moe_grouped_gemm(xs, w, mi(E + 2)),
                lambda: pkg.moe_grouped_gemm(xs, w, mi(1, E + 1)), lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, mi(E)),
                lambda: pkg.grad_moe_grouped_gemm_x_into(xs, ys, w, mi(E + 2)), lambda: pkg.grad_moe_grouped_gemm_w_into(w, ys, xs, mi(E)),
                lambda: pkg.moe_grouped_gemm(xs, mk(E, N, K + 1), off), lambda: pkg.moe_grouped_gemm(xs, mk(N, K), off),
                lambda: pkg.moe_grouped_gemm(xs, mk(1, E, N, K), off), lambda: pkg.moe_grouped_gemm(mk(2, S, K), w, off),
                lambda: pkg.moe_grouped_gemm(mk(S, K - 1), w, off), lambda: pkg.grad_moe_grouped_gemm(mk(S, N + 1), xs, w, off),
                lambda: pkg.grad_moe_grouped_gemm(ys, mk(S + 1, K), w, off), lambda: pkg.grad_moe_grouped_gemm(ys, mk(S, K + 1), w, off),
                lambda: pkg.grad_moe_grouped_gemm_w_into(mk(E, N + 1, K), ys, xs, off),
                lambda: pkg.grad_moe_grouped_gemm_w_into(mk(E, N, K), ys, mk(S - 1, K), off)):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    # `out` buffers of the wrong shape or stride
    for bad in (lambda: pkg.moe_grouped_gemm_into(mk(S, N + 1), xs, w, off), lambda: pkg.moe_grouped_gemm_into(mk(S + 1, N), xs, w, off),
                lambda: pkg.moe_grouped_gemm_into(mk(N, S).t(), xs, w, off), lambda: pkg.moe_grouped_gemm_into(mk(S, N, 2)[:, :, 0], xs, w, off),
                lambda: pkg.grad_moe_grouped_gemm_x_into(mk(K, S).t(), ys, w, off),
                lambda: pkg.grad_moe_grouped_gemm_x_into(mk(S, K + 1), ys, w, off),
                lambda: pkg.grad_moe_grouped_gemm_w_into(mk(E, K, N).transpose(1, 2), ys, xs, off),
                lambda: pkg.grad_moe_grouped_gemm_w_into(mk(E, N + 1, K)[:, :N], ys, xs, off),
                lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, off, out=(mk(S, K + 1), None)),
                lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, off, out=(None, mk(E, N, K + 1))),
                lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, off, out=(mk(S, K), mk(E + 1, N, K))),
                lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, off, out=(mk(K, S).t(), None), needs=(True, False)),
                lambda: pkg.grad_moe_grouped_gemm(ys, xs, w, off, out=(None, mk(E, K, N).transpose(1, 2)), needs=(False, True))):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    # the limits of the descriptor
    for call in (lambda: pkg.moe_grouped_gemm(mk(0, K), w, off), lambda: pkg.moe_grouped_gemm(mk(S, 0), mk(E, N, 0), off),
                 lambda: pkg.moe_grouped_gemm(mk(S, 2), mk(1025, 1, 2), mi(1026)), lambda: pkg.moe_grouped_gemm(mk(2, 65537), mk(1, 1, 65537), mi(2)),
                 lambda: pkg.moe_grouped_gemm(xs, mk(E, 0, K), off), lambda: pkg.grad_moe_grouped_gemm(mk(0, N), mk(0, K), w, off)):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    G = pkg.moe_gemm
    d = G._desc(torch.zeros(3, 60, dtype=torch.bfloat16), 3, 4, 60, 24, 63, 32, 64)
    assert (d.dtype, d.rows, d.experts, d.in_dim, d.out_dim, d.ld_x, d.ld_y, d.ld_w, tuple(d.reserved)) == (2, 3, 4, 60, 24, 63, 32, 64, (0, 0))
    # the weight layouts that are taken as they are: dense, padded rows with the expert stride N ld_w; anything else is copied (inputs)
    assert G._w_layout("w", torch.zeros(E, N, K))[1] == K
    wp = torch.zeros(E, N, K + 3)[:, :, :K]
    assert G._w_layout("w", wp)[0] is wp and G._w_layout("w", wp)[1] == K + 3
    wt = torch.zeros(E, K, N).transpose(1, 2)
    assert G._w_layout("w", wt)[0] is not wt and G._w_layout("w", wt)[1] == K
    assert G._w_layout("w", torch.zeros(E, N + 1, K)[:, :N])[1] == K and G._w_layout("w", torch.zeros(E, N + 1, K)[:, :N])[0].is_contiguous()


# ---- the reference against an independent statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("counts,lead,tail,K,N", [([3, 0, 5, 1], 0, 0, 7, 5), ([0, 0, 4], 2, 3, 8, 3), ([6], 0, 1, 4, 9), ([0, 2, 0], 0, 0, 3, 3)])
def test_reference_matches_a_torch_loop_and_its_autograd(counts, lead, tail, K, N):
    off = ref.offsets_of(counts, lead)
    S, E = int(off[-1]) + tail, len(counts)
    rng = np.random.default_rng(S + K)
    xs, w, dys = rng.standard_normal((S, K)), rng.standard_normal((E, N, K)), rng.standard_normal((S, N))
    lx, lw = torch.tensor(xs, requires_grad=True), torch.tensor(w, requires_grad=True)
    # INTEGRATION.md's earlier recipe: a loop over the experts' slices, zeros in front of and behind them
    parts = [torch.zeros(lead, N, dtype=torch.float64)] + [lx[off[e]:off[e + 1]] @ lw[e].T for e in range(E)]
    ys_t = torch.cat(parts + [torch.zeros(tail, N, dtype=torch.float64)])
    ys, A = ref.gemm_ref(xs, w, off)
    np.testing.assert_allclose(ys, ys_t.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert (A >= np.abs(ys) - 1e-12).all()
    ys_t.backward(torch.tensor(dys))
    dxs, A = ref.bwd_x_ref(dys, w, off)
    np.testing.assert_allclose(dxs, lx.grad.numpy(), rtol=1e-13, atol=1e-15)
    assert (A >= np.abs(dxs) - 1e-12).all() and (dxs[:lead] == 0).all() and (dxs[S - tail:] == 0).all()
    dw, A, R = ref.bwd_w_ref(dys, xs, off)
    np.testing.assert_allclose(dw, lw.grad.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(R.reshape(-1), counts)
    assert all((dw[e] == 0).all() for e in range(E) if counts[e] == 0)
    # offsets outside [0, S] are clamped
    wild = off.astype(np.int64).copy()
    wild[0], wild[-1] = -5, S + 9
    np.testing.assert_array_equal(ref.clamp_offsets(wild, S), np.concatenate([[0], off[1:-1], [S]]))
    np.testing.assert_array_equal(ref.gemm_ref(xs, w, wild)[0][lead:S - tail], ys[lead:S - tail])


# ---- the gate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(37, 24, 8), (129, 72, 520), (65, 264, 1030), (33, 5, 7), (257, 8, 2880)])
def test_an_fp32_evaluation_is_inside_the_gate_and_a_wrong_one_is_not(dt, M, N, K):
    """the forward with R = K; the two pullbacks are the same sums with other operands (below, at one shape)"""
    off = ref.offsets_of([M // 3, M - 2 * (M // 3), M // 3])
    xs, w = ref.make(1, (M, K), dt), ref.make(2, (3, N, K), dt)
    want, A = ref.gemm_ref(xs, w, off)
    for order in ("blas", "sequential"):
        r = ref.ratios(ref.gemm_f32(xs, w, off, dt, order), want, A, K, dt)
        assert r.max() <= 1.0, (order, r.max())
    short = ref.ratios(ref.gemm_f32(xs, w, off, dt, short=8), want, A, K, dt)
    assert (short > 1.0).mean() > 0.5, (short > 1.0).mean()
    other = ref.ratios(ref.gemm_f32(xs, w, off, dt, shift=1), want, A, K, dt)
    assert (other > 1.0).mean() > 0.5, (other > 1.0).mean()


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_the_gate_on_the_two_pullbacks(dt):
    counts, N, K = [40, 0, 129, 23], 72, 40
    off = ref.offsets_of(counts)
    S = int(off[-1])
    xs, w, dys = ref.make(1, (S, K), dt), ref.make(2, (4, N, K), dt), ref.make(3, (S, N), dt)
    want, A = ref.bwd_x_ref(dys, w, off)
    for order in ("blas", "sequential"):
        assert ref.ratio(ref.bwd_x_f32(dys, w, off, dt, order), want, A, N, dt) <= 1.0
    assert (ref.ratios(ref.bwd_x_f32(dys, w, off, dt, short=8), want, A, N, dt) > 1.0).mean() > 0.5
    assert (ref.ratios(ref.bwd_x_f32(dys, w, off, dt, shift=1), want, A, N, dt) > 1.0).mean() > 0.5
    want, A, R = ref.bwd_w_ref(dys, xs, off)
    for order in ("blas", "sequential"):
        assert ref.ratio(ref.bwd_w_f32(dys, xs, off, dt, order), want, A, R, dt) <= 1.0
    own = [e for e, c in enumerate(counts) if c]
    assert (ref.ratios(ref.bwd_w_f32(dys, xs, off, dt, short=8), want, A, R, dt)[own] > 1.0).mean() > 0.5
    assert (ref.ratios(ref.bwd_w_f32(dys, xs, off, dt, shift=1), want, A, R, dt)[own] > 1.0).mean() > 0.5
    bad = ref.bwd_w_f32(dys, xs, off, dt)
    bad[0, 0, 0] = float("nan")
    assert ref.ratio(bad, want, A, R, dt) == float("inf")
    assert (ref.bwd_w_f32(dys, xs, off, dt)[1] == 0).all() and (want[1] == 0).all()
