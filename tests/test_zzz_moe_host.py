"""CPU tests of the mixture-of-experts routing (include/nnop_hip_moe.h): the third library loads and exports exactly its five functions,
links neither of the other two, its header is plain C99 and its descriptors match the ctypes ones, the frozen boundaries of the other
two libraries still hold, every entry point validates in the header's order and returns before any launch, the Python wrappers raise
before any device work, and the reference the GPU tests are judged against (tests/moe_ref.py) agrees with independent statements:
torch softmax / topk / gather and its autograd in fp64, finite differences, NORM_TOPK = renormalised NORM_ALL, hand-written rows for
the tie and NaN rules and hand-written plans.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import moe_ref as ref
from abi_util import ROOT, strip_c_comments

MOE_HEADER = os.path.join(ROOT, "include", "nnop_hip_moe.h")
FIVE = {"nnop_moe_abi_version", "nnop_moe_router", "nnop_moe_router_bwd", "nnop_moe_plan_workspace_bytes", "nnop_moe_plan"}
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
INF, NAN = float("inf"), float("nan")
at = lambda off: C.c_void_p(0x7f0000001000 + off)


# ---- the library and its header -----------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_headers_functions(pkg):
    lib = pkg._lib_moe.load()
    assert set(pkg._lib_moe.EXPORTED_SYMBOLS) == FIVE
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib_moe.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == FIVE, out
    header = strip_c_comments(open(MOE_HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header)) == FIVE
    assert lib.nnop_moe_abi_version() == pkg._lib_moe.MOE_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_ABI_VERSION (\d+)", header).group(1)) == 1
    needed = subprocess.run(["readelf", "-d", pkg._lib_moe.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip.so" not in needed and "libnnop_hip_ext.so" not in needed
    for name in ("moe_router", "_moe_router", "grad_moe_router", "moe_router_into", "grad_moe_router_into", "moe_dispatch_plan",
                 "moe_dispatch_plan_into"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_the_other_two_boundaries_are_unchanged(pkg):
    assert pkg._lib.ABI_VERSION == 7 and len(pkg._lib.EXPORTED_SYMBOLS) == 30
    assert pkg._lib_ext.EXT_ABI_VERSION == 1 and len(pkg._lib_ext.EXPORTED_SYMBOLS) == 4
    main, ext = pkg._lib.load(), pkg._lib_ext.load()
    for name in FIVE:
        assert name not in pkg._lib.EXPORTED_SYMBOLS and name not in pkg._lib_ext.EXPORTED_SYMBOLS
        assert not hasattr(main, name) and not hasattr(ext, name)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib_ext.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == set(pkg._lib_ext.EXPORTED_SYMBOLS)


def _c_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), strip_c_comments(open(MOE_HEADER).read()), re.S).group(1)
    fields = []
    for names in re.findall(r"int32_t\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), int(m.group(2) or 1)))
    return fields


def test_descriptors_match_the_header(pkg):
    for struct, D, size in (("nnop_moe_router_desc", pkg._lib_moe.MoeRouterDesc, 32), ("nnop_moe_plan_desc", pkg._lib_moe.MoePlanDesc, 16)):
        assert C.sizeof(D) == size
        assert _c_fields(struct) == [(n, getattr(t, "_length_", 1)) for n, t in D._fields_]
        assert all((t._type_ if hasattr(t, "_length_") else t) is C.c_int32 for _, t in D._fields_)
    header = strip_c_comments(open(MOE_HEADER).read())
    for name, value in (("NNOP_MOE_NORM_TOPK", pkg._lib_moe.NNOP_MOE_NORM_TOPK), ("NNOP_MOE_NORM_ALL", pkg._lib_moe.NNOP_MOE_NORM_ALL)):
        assert int(re.search(name + r"\s*=\s*(\d+)", header).group(1)) == value
    assert pkg._lib_moe.NORMS == {"topk": 0, "all": 1}


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe.h"\n'
                 "int main(void){ nnop_moe_router_desc r; nnop_moe_plan_desc p; (void)r; (void)p;\n"
                 "  return (sizeof(r) == 32 && sizeof(p) == 16 && NNOP_HIP_MOE_ABI_VERSION == 1 && NNOP_MOE_NORM_ALL == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_missing_or_mismatched_library_fails_loudly(pkg, monkeypatch):
    monkeypatch.setattr(pkg._lib_moe, "_lib", None)
    monkeypatch.setattr(pkg._lib_moe, "MOE_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="moe-ABI version 1"):
        pkg._lib_moe.load()
    monkeypatch.setattr(pkg._lib_moe, "LIB_PATH", "/nonexistent/libnnop_hip_moe.so")
    with pytest.raises(ImportError, match="no CPU or PyTorch fallback"):
        pkg._lib_moe.load()


# ---- validation: order and codes, before any launch -------------------------------------------------------------------------------------
def _rdesc(pkg, reserved=(0, 0), **kw):
    base = dict(dtype=2, tokens=64, experts=128, topk=4, ld=128, norm=0)
    base.update(kw)
    d = pkg._lib_moe.MoeRouterDesc(**base)
    d.reserved[0], d.reserved[1] = reserved
    return d


def _pdesc(pkg, reserved=0, **kw):
    base = dict(tokens=64, topk=4, experts=128)
    base.update(kw)
    d = pkg._lib_moe.MoePlanDesc(**base)
    d.reserved[0] = reserved
    return d


def _fwd(lib, d, ptrs=None):
    return lib.nnop_moe_router(C.byref(d) if d is not None else None, *(ptrs or [OK] * 4), None)


def _bwd(lib, d, ptrs=None):
    return lib.nnop_moe_router_bwd(C.byref(d) if d is not None else None, *(ptrs or [OK] * 7), None)


def _plan(lib, d, ptrs=None, ws=OK, nbytes=1 << 40):
    return lib.nnop_moe_plan(C.byref(d) if d is not None else None, *(ptrs or [OK] * 5), ws, C.c_size_t(nbytes), None)


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(norm=2), "NNOP_ERR_OPTS"),
    (dict(norm=-1), "NNOP_ERR_OPTS"),
    (dict(reserved=(1, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, -1)), "NNOP_ERR_OPTS"),
    (dict(experts=0), "NNOP_ERR_SHAPE"),
    (dict(experts=1025, ld=1025), "NNOP_ERR_SHAPE"),
    (dict(topk=0), "NNOP_ERR_SHAPE"),
    (dict(topk=17), "NNOP_ERR_SHAPE"),
    (dict(experts=7, ld=7, topk=8), "NNOP_ERR_SHAPE"),
    (dict(tokens=0), "NNOP_ERR_SHAPE"),
    (dict(tokens=-3), "NNOP_ERR_SHAPE"),
    (dict(ld=127), "NNOP_ERR_SHAPE"),
    (dict(tokens=2 ** 29, topk=4), "NNOP_ERR_SHAPE"),            # T k = 2^31
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, norm=5, experts=0), "NNOP_ERR_DTYPE"),
    (dict(norm=5, experts=0), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, 3), tokens=0), "NNOP_ERR_OPTS"),
])
def test_router_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe.load(), getattr(pkg._lib, status)
    d = _rdesc(pkg, **kw)
    assert [_fwd(lib, d), _bwd(lib, d)] == [want] * 2
    assert [_fwd(lib, d, [NULL] * 4), _bwd(lib, d, [NULL] * 7)] == [want] * 2        # the descriptor is judged before the pointers


def test_valid_router_descriptors_reach_the_pointer_checks(pkg):
    lib, L = pkg._lib_moe.load(), pkg._lib
    for ok in (dict(), dict(norm=1), dict(dtype=0), dict(dtype=1), dict(experts=1, ld=1, topk=1), dict(experts=1024, ld=1024, topk=16),
               dict(experts=7, ld=10, topk=7), dict(experts=60, ld=60, topk=8), dict(experts=160, ld=163), dict(tokens=2 ** 29 - 1, topk=4),
               dict(tokens=2 ** 31 - 1, topk=1)):
        d = _rdesc(pkg, **ok)
        assert [_fwd(lib, d, [NULL] * 4), _bwd(lib, d, [NULL] * 7)] == [L.NNOP_ERR_NULL] * 2, ok
    assert _fwd(lib, None) == L.NNOP_ERR_NULL and _bwd(lib, None) == L.NNOP_ERR_NULL


def test_router_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe.load(), pkg._lib
    for dtype in (0, 1, 2):
        es = 4 if dtype == 0 else 2
        d = _rdesc(pkg, dtype=dtype)
        # forward: idx, w, lse, logits;  pullback: dlogits, dw, dlse (optional), w, idx, lse, logits
        for fn, aligns, optional in ((_fwd, [4, 4, 4, es], ()), (_bwd, [es, 4, 4, 4, 4, 4, es], (2,))):
            for pos, a in enumerate(aligns):
                if pos not in optional:
                    b = [OK] * len(aligns)
                    b[pos] = NULL
                    assert fn(lib, d, b) == L.NNOP_ERR_NULL, (fn.__name__, pos)
                    c = [at(1)] * len(aligns)                    # NULL is judged before alignment
                    c[pos] = NULL
                    assert fn(lib, d, c) == L.NNOP_ERR_NULL, (fn.__name__, pos)
                c = [OK] * len(aligns)
                c[pos] = at(a // 2)                              # aligned to half of what is needed
                assert fn(lib, d, c) == L.NNOP_ERR_ALIGN, (fn.__name__, pos, a)
        # a NULL dlse is no error: with every other pointer misaligned the call gets as far as the alignment check
        c = [at(1)] * 7
        c[2] = NULL
        assert _bwd(lib, d, c) == L.NNOP_ERR_ALIGN


@pytest.mark.parametrize("kw,status", [
    (dict(reserved=1), "NNOP_ERR_OPTS"),
    (dict(reserved=-1, tokens=0), "NNOP_ERR_OPTS"),              # options before shape
    (dict(tokens=0), "NNOP_ERR_SHAPE"),
    (dict(topk=0), "NNOP_ERR_SHAPE"),
    (dict(experts=0), "NNOP_ERR_SHAPE"),
    (dict(experts=1025), "NNOP_ERR_SHAPE"),
    (dict(tokens=2 ** 29, topk=4), "NNOP_ERR_SHAPE"),
    (dict(tokens=2 ** 20, topk=2 ** 20), "NNOP_ERR_SHAPE"),
])
def test_plan_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe.load(), getattr(pkg._lib, status)
    d = _pdesc(pkg, **kw)
    assert _plan(lib, d) == want and _plan(lib, d, [NULL] * 5, NULL, 0) == want
    assert lib.nnop_moe_plan_workspace_bytes(C.byref(d)) == 0


def test_plan_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe.load(), pkg._lib
    assert _plan(lib, None) == L.NNOP_ERR_NULL and lib.nnop_moe_plan_workspace_bytes(None) == 0
    for ok in (dict(), dict(tokens=1, topk=1, experts=1), dict(tokens=2 ** 31 - 1, topk=1, experts=1024), dict(topk=40, experts=3)):
        d = _pdesc(pkg, **ok)
        need = lib.nnop_moe_plan_workspace_bytes(C.byref(d))
        assert need > 0 and need % 16 == 0
        assert _plan(lib, d, [NULL] * 5, NULL, 0) == L.NNOP_ERR_NULL
        for pos in range(5):                                     # counts, offsets, perm, slot, idx
            b = [OK] * 5
            b[pos] = NULL
            assert _plan(lib, d, b) == L.NNOP_ERR_NULL
            c = [at(2)] * 5
            c[pos] = NULL
            assert _plan(lib, d, c) == L.NNOP_ERR_NULL
            c = [OK] * 5
            c[pos] = at(2)
            assert _plan(lib, d, c) == L.NNOP_ERR_ALIGN
        assert _plan(lib, d, ws=NULL) == L.NNOP_ERR_NULL
        assert _plan(lib, d, ws=at(8)) == L.NNOP_ERR_ALIGN
        assert _plan(lib, d, ws=at(8), nbytes=0) == L.NNOP_ERR_ALIGN             # alignment before size
        assert _plan(lib, d, [at(2)] * 5, nbytes=0) == L.NNOP_ERR_ALIGN          # ... and the pointers before the workspace
        assert _plan(lib, d, nbytes=need - 1) == L.NNOP_ERR_WORKSPACE            # the workspace size is judged last
        assert _plan(lib, d, nbytes=0) == L.NNOP_ERR_WORKSPACE


def test_plan_workspace_bytes_is_a_function_of_the_descriptor(pkg):
    lib = pkg._lib_moe.load()
    wb = lambda **kw: lib.nnop_moe_plan_workspace_bytes(C.byref(_pdesc(pkg, **kw)))
    assert wb(tokens=1, topk=1, experts=1) == 16                                # one histogram of one word, rounded up to 16 bytes
    assert wb(tokens=16, topk=4, experts=128) == 128 * 4                         # 64 flat ids: one chunk
    assert wb(tokens=17, topk=4, experts=128) == 2 * 128 * 4
    assert wb(tokens=8192, topk=8, experts=256) == 1024 * 256 * 4
    assert wb(tokens=2 ** 31 - 1, topk=1, experts=1024) <= 4096 * 1024 * 4       # longer chunks, never above 4096 of them


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    T, E, k = 5, 8, 2
    x, w, idx, lse = torch.ones(T, E), torch.ones(T, k), torch.zeros(T, k, dtype=torch.int32), torch.ones(T)
    for call in (lambda: pkg.moe_router(x, k), lambda: pkg._moe_router(x, k), lambda: pkg.moe_router_into(w, idx, lse, x, k),
                 lambda: pkg.grad_moe_router(w, w, idx, lse, x), lambda: pkg.grad_moe_router_into(x, w, w, idx, lse, x),
                 lambda: pkg.moe_router(x.clone().requires_grad_(True), k), lambda: pkg.moe_dispatch_plan(idx, E),
                 lambda: pkg.moe_dispatch_plan_into(idx, idx, idx, idx, idx, E)):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    x, w, idx, lse = mk(T, E), mk(T, k), mk(T, k, dt=torch.int32), mk(T)
    fwd = lambda x, k, **kw: (lambda: pkg.moe_router(x, k, **kw), lambda: pkg._moe_router(x, k, **kw),
                              lambda: pkg.moe_router_into(w, idx, lse, x, k, **kw))
    for args in (([1.0], k), (mk(T, E, dt=torch.float64), k), (mk(T, E, dt=torch.int32), k), (x, 2.0), (x, True), (x, "2")):
        for call in fwd(*args):
            with pytest.raises(TypeError):
                call()
    for args, kw, status in (((x, 0), {}, "NNOP_ERR_SHAPE"), ((x, E + 1), {}, "NNOP_ERR_SHAPE"), ((mk(T, 64), 17), {}, "NNOP_ERR_SHAPE"),
                             ((mk(2, 1025), 2), {}, "NNOP_ERR_SHAPE"), ((mk(0, E), 2), {}, "NNOP_ERR_SHAPE"), ((mk(T, 0), 1), {}, "NNOP_ERR_SHAPE"),
                             ((x, k), dict(norm="softmax"), "NNOP_ERR_OPTS"), ((x, k), dict(norm=0), "NNOP_ERR_OPTS")):
        for call in fwd(*args, **kw):
            with pytest.raises(pkg.NNopError) as e:
                call()
            assert e.value.status == getattr(pkg._lib, status)
    # the buffers of the _into forms and of the pullback
    for bad in (lambda: pkg.moe_router_into(mk(T, k + 1), idx, lse, x, k), lambda: pkg.moe_router_into(w, mk(T, k), lse, x, k),
                lambda: pkg.moe_router_into(w, idx, mk(T, 1), x, k), lambda: pkg.moe_router_into(mk(k, T).t(), idx, lse, x, k),
                lambda: pkg.grad_moe_router(mk(T, k, dt=torch.bfloat16), w, idx, lse, x), lambda: pkg.grad_moe_router(w, w, idx, mk(T + 1), x),
                lambda: pkg.grad_moe_router(w, w, idx, lse, x, dlse=mk(T, 1)), lambda: pkg.grad_moe_router(w, w, idx, lse, x, out=mk(T, E + 1)),
                lambda: pkg.grad_moe_router(w, w, idx, lse, x, out=mk(T, E, dt=torch.bfloat16)),
                lambda: pkg.grad_moe_router_into(mk(E, T).t(), w, w, idx, lse, x),
                lambda: pkg.grad_moe_router_into(mk(T, E + 3)[:, :E], w, w, idx, lse, x)):       # another row stride than that of logits
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    # the plan
    for args in ((mk(T, k), E), (idx, 8.0), ([0, 1], E)):
        with pytest.raises(TypeError):
            pkg.moe_dispatch_plan(*args)
    for args in ((idx, 0), (idx, 1025), (mk(0, k, dt=torch.int32), E), (mk(T, 0, dt=torch.int32), E)):
        with pytest.raises(pkg.NNopError) as e:
            pkg.moe_dispatch_plan(*args)
        assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    i32 = lambda *s: mk(*s, dt=torch.int32)
    for bufs in ((i32(E + 1), i32(E + 1), i32(T * k), i32(T, k)), (i32(E), i32(E), i32(T * k), i32(T, k)), (i32(E), i32(E + 1), i32(T, k), i32(T, k)),
                 (i32(E), i32(E + 1), i32(T * k), i32(T * k)), (mk(E), i32(E + 1), i32(T * k), i32(T, k))):
        with pytest.raises(pkg.NNopError, match="must"):
            pkg.moe_dispatch_plan_into(*bufs, idx, E)
    with pytest.raises(pkg.NNopError, match="workspace") as e:
        pkg.moe_dispatch_plan_into(i32(E), i32(E + 1), i32(T * k), i32(T, k), idx, E, workspace=mk(8, dt=torch.uint8))
    assert e.value.status == pkg._lib.NNOP_ERR_WORKSPACE
    d = pkg.moe._desc(torch.zeros(3, 60, dtype=torch.bfloat16), 3, 60, 4, 63, "all")
    assert (d.dtype, d.tokens, d.experts, d.topk, d.ld, d.norm, tuple(d.reserved)) == (2, 3, 60, 4, 63, 1, (0, 0))
    assert pkg.moe._rows(torch.zeros(5, 11)[:, :8], 8)[1] == 11 and pkg.moe._rows(torch.zeros(2, 5, 8), 8)[1] == 8


# ---- the reference against independent statements -------------------------------------------------------------------------------------
def _rows_without_boundary_ties(x, k):
    s = -np.sort(-x, axis=-1)
    return x[(np.diff(s[:, :k + 1], axis=-1) != 0).all(axis=-1)] if k < x.shape[1] else x[(np.diff(s, axis=-1) != 0).all(axis=-1)]


def _torch_router(x, k, norm):
    p = torch.softmax(x, dim=-1)
    pv, pi = torch.topk(x, k, dim=-1)
    w = torch.gather(p, -1, pi)
    if norm == "topk":
        w = w / w.sum(-1, keepdim=True)
    return w, pi, torch.logsumexp(x, dim=-1)


@pytest.mark.parametrize("norm", ref.NORMS)
@pytest.mark.parametrize("T,E,k", [(33, 7, 3), (17, 60, 8), (9, 160, 16), (5, 4, 4), (4, 1, 1)])
def test_reference_matches_torch_softmax_topk_gather_and_its_autograd(T, E, k, norm):
    x = _rows_without_boundary_ties(ref.make_logits(E + k, T, E).astype(np.float64), k)
    assert x.shape[0] >= 4
    rng = np.random.default_rng(1)
    dw, dlse = rng.standard_normal((x.shape[0], k)), rng.standard_normal(x.shape[0])
    w, idx, lse = ref.router_ref(x, k, norm)
    leaf = torch.tensor(x, requires_grad=True)
    tw, ti, tlse = _torch_router(leaf, k, norm)
    np.testing.assert_array_equal(idx, ti.numpy())
    np.testing.assert_allclose(w, tw.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(lse, tlse.detach().numpy(), rtol=1e-13)
    for use_dlse in (False, True):
        leaf.grad = None
        loss = (tw * torch.tensor(dw)).sum() + ((tlse * torch.tensor(dlse)).sum() if use_dlse else 0.0)
        loss.backward(retain_graph=True)
        got = ref.router_grad_ref(dw, x, k, norm, dlse if use_dlse else None)
        np.testing.assert_allclose(got, leaf.grad.numpy(), rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("norm", ref.NORMS)
@pytest.mark.parametrize("use_dlse", [False, True])
def test_reference_gradient_matches_finite_differences(norm, use_dlse):
    T, E, k = 6, 12, 3
    x = ref.make_logits(3, T, E).astype(np.float64)
    rng = np.random.default_rng(2)
    dw, dlse = rng.standard_normal((T, k)), rng.standard_normal(T)

    def loss(x):
        w, _, lse = ref.router_ref(x, k, norm)
        return float((w * dw).sum() + ((lse * dlse).sum() if use_dlse else 0.0))
    g = ref.router_grad_ref(dw, x, k, norm, dlse if use_dlse else None)
    h = 1e-6                                                         # far below the gaps between N(0, 9) logits: the selection stays
    for t in range(T):
        for e in range(E):
            d = np.zeros_like(x)
            d[t, e] = h
            fd = (loss(x + d) - loss(x - d)) / (2 * h)
            assert abs(fd - g[t, e]) < 1e-7 * max(1.0, abs(g[t, e])), (t, e, fd, g[t, e])
    if norm == "topk" and not use_dlse:
        mask = np.ones_like(g, bool)
        np.put_along_axis(mask, ref.select(x, k).astype(np.int64), False, axis=-1)
        assert (g[mask] == 0).all()


def test_norm_topk_is_the_renormalised_norm_all():
    x = ref.make_logits(5, 40, 60).astype(np.float64)
    wt, it, lt = ref.router_ref(x, 8, "topk")
    wa, ia, la = ref.router_ref(x, 8, "all")
    np.testing.assert_array_equal(it, ia)
    np.testing.assert_array_equal(lt, la)
    np.testing.assert_allclose(wt, wa / wa.sum(-1, keepdims=True), rtol=1e-13)
    np.testing.assert_allclose(wt.sum(-1), 1.0, rtol=1e-14)
    assert (np.diff(wt, axis=-1) <= 0).all()                         # best first


def test_tie_and_nan_rules_on_hand_written_rows():
    x = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],                         # equal values: the lower index first
                  [0.0, -0.0, -1.0, -0.0, 0.0],                      # -0 == +0
                  [1.0, NAN, INF, NAN, 5.0],                         # NaN above +inf, NaN against NaN by index
                  [-INF, -INF, 2.0, -INF, -INF],                     # fewer than k finite
                  [-INF, -INF, -INF, -INF, -INF],
                  [7.0, 7.0, 7.0, 7.0, 7.0]])                        # all equal
    np.testing.assert_array_equal(ref.select(x, 3), [[1, 2, 4], [0, 1, 3], [1, 3, 2], [2, 0, 1], [0, 1, 2], [0, 1, 2]])
    np.testing.assert_array_equal(ref.select(x, 5)[2], [1, 3, 2, 4, 0])
    for norm in ref.NORMS:
        w, idx, lse = ref.router_ref(x, 3, norm)
        assert np.isnan(w[2]).all() and np.isnan(w[4]).all() and np.isnan(lse[[2, 4]]).all()
        assert np.isfinite(w[[0, 1, 3, 5]]).all() and np.isfinite(lse[[0, 1, 3, 5]]).all()
        np.testing.assert_allclose(w[3], [1.0, 0.0, 0.0])
        np.testing.assert_allclose(w[5], [1 / 3] * 3 if norm == "topk" else [1 / 5] * 3)
        assert lse[3] == 2.0
    for row in x:                                                    # always k distinct indices in [0, E)
        for k in range(1, 6):
            s = ref.select(row[None], k)[0]
            assert len(set(s.tolist())) == k and s.min() >= 0 and s.max() < 5


def test_bf16_grid_inputs_have_ties_at_the_kth_place():
    """the GPU grid's inputs, N(0, 3^2) rounded to bf16: the k-th and (k+1)-th largest are equal in several per cent of the rows"""
    for E, k in ((128, 8), (60, 4), (1024, 16)):
        x = torch.tensor(ref.make_logits(E, 1030, E)).to(torch.bfloat16).double().numpy()
        s = -np.sort(-x, axis=-1)
        assert 0.02 < (s[:, k - 1] == s[:, k]).mean() < 0.5, (E, k)


def test_plan_reference_on_hand_written_cases():
    idx = np.array([[2, 0], [0, 2], [3, 0], [2, 2]], np.int32)      # expert 1 is empty; a token may name an expert twice
    counts, offsets, perm, slot = ref.plan_ref(idx, 4)
    np.testing.assert_array_equal(counts, [3, 0, 4, 1])
    np.testing.assert_array_equal(offsets, [0, 3, 3, 7, 8])
    np.testing.assert_array_equal(perm, [1, 2, 5, 0, 3, 6, 7, 4])
    np.testing.assert_array_equal(slot, [[3, 0], [1, 4], [7, 2], [5, 6]])
    counts, offsets, perm, slot = ref.plan_ref(np.zeros((5, 2), np.int32), 3)         # one expert takes everything
    np.testing.assert_array_equal(counts, [10, 0, 0])
    np.testing.assert_array_equal(offsets, [0, 10, 10, 10])
    np.testing.assert_array_equal(perm, np.arange(10))
    np.testing.assert_array_equal(slot.reshape(-1), np.arange(10))
    idx = np.array([[1, -1], [-1, 0], [7, 1], [0, -1]], np.int32)   # -1 and an id past E are skipped
    counts, offsets, perm, slot = ref.plan_ref(idx, 2)
    np.testing.assert_array_equal(counts, [2, 2])
    np.testing.assert_array_equal(offsets, [0, 2, 4])
    np.testing.assert_array_equal(perm, [3, 6, 0, 5, -1, -1, -1, -1])
    np.testing.assert_array_equal(slot, [[2, -1], [-1, 0], [-1, 3], [1, -1]])
    valid = slot >= 0
    np.testing.assert_array_equal(perm[slot[valid]], np.arange(8).reshape(4, 2)[valid])


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_an_fp32_evaluation_is_inside_the_gates_and_a_wrong_one_is_not(dt):
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    x = torch.tensor(ref.make_logits(11, 257, 128)).to(tdt).double().numpy()
    rng = np.random.default_rng(3)
    dw = rng.standard_normal((257, 8)).astype(np.float32)
    for norm in ref.NORMS:
        w, idx, lse = ref.router_ref(x, 8, norm)
        x32 = x.astype(np.float32)
        m = x32.max(-1, keepdims=True)
        lse32 = (m + np.log(np.exp(x32 - m).sum(-1, keepdims=True, dtype=np.float32)))[:, 0]
        xs = np.take_along_axis(x32, idx.astype(np.int64), -1)
        e = np.exp(xs - xs[:, :1])
        w32 = e / e.sum(-1, keepdims=True, dtype=np.float32) if norm == "topk" else np.exp(xs - lse32[:, None])
        assert w32.dtype == np.float32 and ref.w_ratio(w32, w) <= 0.5 and ref.lse_ratio(lse32, lse) <= 0.5
        assert ref.w_ratio(w32 * np.float32(1 + 1e-5), w) > 1.0 and ref.lse_ratio(lse32 + 1e-4, lse) > 1.0
        g = ref.router_grad_ref(dw, x, 8, norm)
        once = torch.tensor(g).to(tdt).double().numpy()
        assert ref.dl_ratio(once, g, dt) <= 0.5
        bad = once.copy()
        bad[3, 5] = NAN
        assert ref.dl_ratio(bad, g, dt) == INF
    w, _, _ = ref.router_ref(np.array([[1.0, NAN, 2.0]]), 2, "topk")
    assert ref.w_ratio(w, w) == 0.0 and ref.w_ratio(np.zeros_like(w), w) == INF      # the NaN pattern has to match
