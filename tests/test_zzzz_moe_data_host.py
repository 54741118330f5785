"""CPU tests of the mixture-of-experts permute and weighted combine (include/nnop_hip_moe_data.h): the fourth library loads and exports
exactly its header's functions, links none of the other three, its header is plain C99 and its descriptor matches the ctypes one, the
frozen boundaries of the other three libraries still hold, every entry point validates in the header's order and returns before any
launch, the Python wrappers raise before any device work, the reference the GPU tests are judged against (tests/moe_data_ref.py) agrees
with torch fp64 indexing and its autograd and with a hand-written plan, and the derived gates pass an fp32 evaluation and fail a wrong one.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import moe_data_ref as ref
from abi_util import ROOT, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_moe_data.h")
NAMES = {"nnop_moe_data_abi_version", "nnop_moe_permute", "nnop_moe_permute_bwd", "nnop_moe_combine", "nnop_moe_combine_bwd"}
PY_NAMES = ("moe_permute", "_moe_permute", "grad_moe_permute", "moe_permute_into", "grad_moe_permute_into", "moe_combine", "_moe_combine",
            "grad_moe_combine", "moe_combine_into", "grad_moe_combine_into")
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
INF, NAN = float("inf"), float("nan")
at = lambda off: C.c_void_p(0x7f0000001000 + off)
# entry point -> the alignment of each pointer argument ("e": the element size of the row arrays)
ENTRY = {"nnop_moe_permute": ["e", "e", 4], "nnop_moe_permute_bwd": ["e", "e", 4], "nnop_moe_combine": ["e", "e", 4, 4],
         "nnop_moe_combine_bwd": ["e", 4, "e", "e", 4, 4, 4]}


# ---- the library and its header -----------------------------------------------------------------------------------------------------
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_exactly_the_headers_functions(pkg):
    M = pkg._lib_moe_data
    lib = M.load()
    assert set(M.EXPORTED_SYMBOLS) == NAMES
    assert _defined(M.LIB_PATH) == NAMES
    header = strip_c_comments(open(HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header)) == NAMES
    assert lib.nnop_moe_data_abi_version() == M.MOE_DATA_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_DATA_ABI_VERSION (\d+)", header).group(1)) == 1
    needed = subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip" not in needed                               # none of libnnop_hip.so, libnnop_hip_ext.so, libnnop_hip_moe.so
    for name in PY_NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert "moe_data" in pkg.__all__ and "_lib_moe_data" in pkg.__all__


def test_the_other_three_boundaries_are_unchanged(pkg):
    assert pkg._lib.ABI_VERSION == 7 and len(pkg._lib.EXPORTED_SYMBOLS) == 30
    assert pkg._lib_ext.EXT_ABI_VERSION == 1 and len(pkg._lib_ext.EXPORTED_SYMBOLS) == 4
    assert pkg._lib_moe.MOE_ABI_VERSION == 1 and len(pkg._lib_moe.EXPORTED_SYMBOLS) == 5
    for M in (pkg._lib, pkg._lib_ext, pkg._lib_moe):
        lib = M.load()
        for name in NAMES:
            assert name not in M.EXPORTED_SYMBOLS and not hasattr(lib, name)
    for M in (pkg._lib_ext, pkg._lib_moe):
        assert _defined(M.LIB_PATH) == set(M.EXPORTED_SYMBOLS)
    assert not NAMES & _defined(pkg._lib.LIB_PATH)
    for h in ("nnop_hip.h", "nnop_hip_ext.h", "nnop_hip_moe.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES) and "nnop_moe_rows_desc" not in text


def test_descriptor_matches_the_header(pkg):
    D = pkg._lib_moe_data.MoeRowsDesc
    body = re.search(r"typedef struct nnop_moe_rows_desc \{(.*?)\} nnop_moe_rows_desc;", strip_c_comments(open(HEADER).read()), re.S).group(1)
    fields = []
    for names in re.findall(r"int32_t\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert C.sizeof(D) == 32
    assert fields == [(n, getattr(t, "_length_", 1)) for n, t in D._fields_]
    assert [n for n, _ in fields] == ["dtype", "tokens", "topk", "dim", "ld_tok", "ld_slot", "reserved"]
    assert all((t._type_ if hasattr(t, "_length_") else t) is C.c_int32 for _, t in D._fields_)
    assert (pkg._lib_moe_data.MAX_TOPK, pkg._lib_moe_data.MAX_DIM) == (64, 65536)


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe_data.h"\n'
                 "int main(void){ nnop_moe_rows_desc r; (void)r;\n"
                 "  return (sizeof(r) == 32 && NNOP_HIP_MOE_DATA_ABI_VERSION == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_missing_or_mismatched_library_fails_loudly(pkg, monkeypatch):
    M = pkg._lib_moe_data
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "MOE_DATA_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="moe-data-ABI version 1"):
        M.load()
    monkeypatch.setattr(M, "MOE_DATA_ABI_VERSION", 1)
    monkeypatch.setattr(M, "EXPORTED_SYMBOLS", M.EXPORTED_SYMBOLS + ("nnop_moe_not_there",))
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="does not export nnop_moe_not_there"):
        M.load()
    monkeypatch.setattr(M, "LIB_PATH", "/nonexistent/libnnop_hip_moe_data.so")
    with pytest.raises(ImportError, match="no CPU or PyTorch fallback"):
        M.load()


# ---- validation: order and codes, before any launch -------------------------------------------------------------------------------------
def _desc(pkg, reserved=(0, 0), **kw):
    base = dict(dtype=2, tokens=64, topk=4, dim=128, ld_tok=128, ld_slot=128)
    base.update(kw)
    d = pkg._lib_moe_data.MoeRowsDesc(**base)
    d.reserved[0], d.reserved[1] = reserved
    return d


def _call(lib, name, d, ptrs=None):
    return getattr(lib, name)(C.byref(d) if d is not None else None, *(ptrs or [OK] * len(ENTRY[name])), None)


def _all(lib, d, ptr=None):
    return [_call(lib, name, d, None if ptr is None else [ptr] * len(ENTRY[name])) for name in ENTRY]


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(reserved=(1, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, -1)), "NNOP_ERR_OPTS"),
    (dict(tokens=0), "NNOP_ERR_SHAPE"),
    (dict(tokens=-3), "NNOP_ERR_SHAPE"),
    (dict(topk=0), "NNOP_ERR_SHAPE"),
    (dict(topk=65), "NNOP_ERR_SHAPE"),
    (dict(dim=0, ld_tok=1, ld_slot=1), "NNOP_ERR_SHAPE"),
    (dict(dim=65537, ld_tok=65537, ld_slot=65537), "NNOP_ERR_SHAPE"),
    (dict(ld_tok=127), "NNOP_ERR_SHAPE"),                        # ld = D - 1, either stride
    (dict(ld_slot=127), "NNOP_ERR_SHAPE"),
    (dict(tokens=2 ** 29, topk=4), "NNOP_ERR_SHAPE"),            # T k = 2^31
    (dict(tokens=2 ** 25, topk=64), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, reserved=(5, 0), tokens=0), "NNOP_ERR_DTYPE"),
    (dict(reserved=(0, 3), tokens=0), "NNOP_ERR_OPTS"),
    (dict(reserved=(2, 0), dim=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_data.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert _all(lib, d) == [want] * 4
    assert _all(lib, d, NULL) == [want] * 4                          # the descriptor is judged before the pointers
    assert _all(lib, d, at(1)) == [want] * 4


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    lib, L = pkg._lib_moe_data.load(), pkg._lib
    for ok in (dict(), dict(dtype=0), dict(dtype=1), dict(tokens=1, topk=1, dim=1, ld_tok=1, ld_slot=1), dict(topk=64),
               dict(dim=65536, ld_tok=65536, ld_slot=65536), dict(dim=7, ld_tok=10, ld_slot=7), dict(dim=7, ld_tok=7, ld_slot=15),
               dict(tokens=2 ** 29 - 1, topk=4), dict(tokens=2 ** 31 - 1, topk=1)):
        d = _desc(pkg, **ok)
        assert _all(lib, d, NULL) == [L.NNOP_ERR_NULL] * 4, ok
    assert _all(lib, None) == [L.NNOP_ERR_NULL] * 4                  # the descriptor itself: first of all
    assert _all(lib, None, at(1)) == [L.NNOP_ERR_NULL] * 4


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe_data.load(), pkg._lib
    for dtype in (0, 1, 2):
        es = 4 if dtype == 0 else 2
        d = _desc(pkg, dtype=dtype)
        for name, aligns in ENTRY.items():
            aligns = [es if a == "e" else a for a in aligns]
            for pos, a in enumerate(aligns):
                b = [OK] * len(aligns)
                b[pos] = NULL                                        # none is optional
                assert _call(lib, name, d, b) == L.NNOP_ERR_NULL, (name, pos)
                c = [at(1)] * len(aligns)                            # NULL is judged before alignment
                c[pos] = NULL
                assert _call(lib, name, d, c) == L.NNOP_ERR_NULL, (name, pos)
                c = [OK] * len(aligns)
                c[pos] = at(a // 2)                                  # aligned to half of what is needed
                assert _call(lib, name, d, c) == L.NNOP_ERR_ALIGN, (name, pos, a)


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    T, k, D = 5, 2, 8
    S = T * k
    f = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    x, xs, w, perm, slot = f(T, D), f(S, D), f(T, k), i(S), i(T, k)
    for call in (lambda: pkg.moe_permute(x, perm, slot), lambda: pkg._moe_permute(x, perm, slot), lambda: pkg.moe_permute_into(xs, x, perm),
                 lambda: pkg.grad_moe_permute(xs, slot), lambda: pkg.grad_moe_permute_into(x, xs, slot),
                 lambda: pkg.moe_combine(xs, w, perm, slot), lambda: pkg._moe_combine(xs, w, perm, slot),
                 lambda: pkg.moe_combine_into(x, xs, w, slot), lambda: pkg.grad_moe_combine(x, xs, w, perm, slot),
                 lambda: pkg.grad_moe_combine_into(xs, w, x, xs, w, perm, slot),
                 lambda: pkg.moe_permute(x.clone().requires_grad_(True), perm, slot),
                 lambda: pkg.moe_combine(xs.clone().requires_grad_(True), w, perm, slot)):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    mi = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnGpu)
    x, xs, w, perm, slot = mk(T, D), mk(S, D), mk(T, k), mi(S), mi(T, k)
    h = lambda *s: mk(*s, dt=torch.bfloat16)
    # wrong types: row arrays that are no float32 / float16 / bfloat16, index arrays that are not int32, a 16-bit w
    for call in (lambda: pkg.moe_permute(mk(T, D, dt=torch.float64), perm, slot), lambda: pkg.moe_permute([1.0], perm, slot),
                 lambda: pkg.moe_permute(x, mk(S), slot), lambda: pkg.moe_permute(x, perm, mk(T, k)),
                 lambda: pkg.moe_permute(x, perm.long(), slot), lambda: pkg.moe_permute_into(xs, x, mk(S)),
                 lambda: pkg.moe_permute_into(mi(S, D), x, perm), lambda: pkg.grad_moe_permute(mi(S, D), slot),
                 lambda: pkg.grad_moe_permute(xs, mk(T, k)), lambda: pkg.moe_combine(mk(S, D, dt=torch.float64), w, perm, slot),
                 lambda: pkg.moe_combine(h(S, D), h(T, k), perm, slot), lambda: pkg.moe_combine(xs, mk(T, k, dt=torch.float16), perm, slot),
                 lambda: pkg._moe_combine(xs, w, mk(S), slot), lambda: pkg.moe_combine_into(h(T, D), h(S, D), h(T, k), slot),
                 lambda: pkg.grad_moe_combine(h(T, D), h(S, D), h(T, k), perm, slot),
                 lambda: pkg.grad_moe_combine_into(xs, h(T, k), x, xs, w, perm, slot),
                 lambda: pkg.grad_moe_combine(x, xs, w, perm.long(), slot)):
        with pytest.raises(TypeError):
            call()
    # shapes of perm / slot / the row arrays that do not fit
    for bad in (lambda: pkg.moe_permute(x, mi(S + 1), slot), lambda: pkg.moe_permute(x, mi(T, k), slot), lambda: pkg.moe_permute(x, perm, mi(T + 1, k)),
                lambda: pkg.moe_permute(mk(1, T, D), perm, slot), lambda: pkg.moe_permute_into(mk(S, D + 1), x, perm),
                lambda: pkg.moe_permute_into(mk(S + 1, D), x, perm), lambda: pkg.moe_permute_into(h(S, D), x, perm),
                lambda: pkg.moe_permute_into(xs, x, mi(S + 1)), lambda: pkg.grad_moe_permute(mk(S + 1, D), slot),
                lambda: pkg.grad_moe_permute(xs, slot, out=mk(T, D + 1)), lambda: pkg.grad_moe_permute(xs, slot, out=h(T, D)),
                lambda: pkg.grad_moe_permute(mk(2, T, D), slot),
                lambda: pkg.moe_combine(mk(S - 1, D), w, perm, slot), lambda: pkg.moe_combine(xs, mk(T, k + 1), perm, slot),
                lambda: pkg.moe_combine(xs, w, mi(S - 1), slot), lambda: pkg.moe_combine_into(mk(T + 1, D), xs, w, slot),
                lambda: pkg.moe_combine_into(mk(T, D), xs, mk(T), slot), lambda: pkg.grad_moe_combine(mk(T, D + 1), xs, w, perm, slot),
                lambda: pkg.grad_moe_combine(x, xs, w, perm, slot, out=(mk(S, D + 1), mk(T, k))),
                lambda: pkg.grad_moe_combine(x, xs, w, perm, slot, out=(xs, mk(T, k + 1))),
                lambda: pkg.grad_moe_combine(x, xs, w, mi(S + 2), slot)):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    # strided outputs of the _into forms: a transposed buffer, a dw that is not dense, a dys with another row stride than ys
    for bad in (lambda: pkg.moe_permute_into(mk(D, S).t(), x, perm), lambda: pkg.grad_moe_permute_into(mk(D, T).t(), xs, slot),
                lambda: pkg.moe_combine_into(mk(D, T).t(), xs, w, slot), lambda: pkg.moe_combine_into(mk(T, D, 2)[:, :, 0], xs, w, slot),
                lambda: pkg.grad_moe_combine_into(mk(D, S).t(), mk(T, k), x, xs, w, perm, slot),
                lambda: pkg.grad_moe_combine_into(xs, mk(k, T).t(), x, xs, w, perm, slot),
                lambda: pkg.grad_moe_combine_into(mk(S, D + 3)[:, :D], mk(T, k), x, xs, w, perm, slot)):
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    # the limits of the descriptor
    for call, status in ((lambda: pkg.moe_permute(mk(T, 65537), perm, slot), "NNOP_ERR_SHAPE"),
                         (lambda: pkg.moe_permute(mk(1, D), mi(65), mi(1, 65)), "NNOP_ERR_SHAPE"),
                         (lambda: pkg.moe_permute(mk(0, D), mi(0), mi(0, k)), "NNOP_ERR_SHAPE"),
                         (lambda: pkg.moe_permute(mk(T, 0), perm, slot), "NNOP_ERR_SHAPE"),
                         (lambda: pkg.moe_combine(mk(0, D), mk(T, 0), mi(0), mi(T, 0)), "NNOP_ERR_SHAPE"),
                         (lambda: pkg.grad_moe_permute(mk(65, D), mi(1, 65)), "NNOP_ERR_SHAPE")):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == getattr(pkg._lib, status)
    d = pkg.moe_data._desc(torch.zeros(3, 60, dtype=torch.bfloat16), 3, 4, 60, 63, 64)
    assert (d.dtype, d.tokens, d.topk, d.dim, d.ld_tok, d.ld_slot, tuple(d.reserved)) == (2, 3, 4, 60, 63, 64, (0, 0))
    assert pkg.moe_data._out_rows("xs", torch.zeros(5, 11)[:, :8], 8)[1] == 11 and pkg.moe_data._out_rows("y", torch.zeros(2, 5, 8), 8)[1] == 8


# ---- the reference against independent statements -------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k,D,E,skip", [(37, 1, 7, 8, 0.3), (33, 4, 24, 8, 0.0), (17, 8, 10, 60, 0.3), (9, 16, 5, 1, 0.5)])
def test_reference_matches_torch_indexing_and_its_autograd(T, k, D, E, skip):
    _, perm, slot = ref.make_plan(T + k, T, k, E, skip)
    S = T * k
    rng = np.random.default_rng(D)
    x, ys, w = rng.standard_normal((T, D)), rng.standard_normal((S, D)), ref.make_weights(3, T, k).astype(np.float64)
    dxs, dy = rng.standard_normal((S, D)), rng.standard_normal((T, D))
    tp, ts = torch.tensor(perm.astype(np.int64)), torch.tensor(slot.astype(np.int64))
    okp, oks = (tp >= 0)[:, None], (ts >= 0)[..., None]
    # the composition of INTEGRATION.md's earlier recipe, skipped entries masked
    lx = torch.tensor(x, requires_grad=True)
    xs_t = torch.where(okp, lx[tp.clamp(min=0) // k], 0.0)
    np.testing.assert_array_equal(ref.permute_ref(x, perm, k), xs_t.detach().numpy())
    xs_t.backward(torch.tensor(dxs))
    got, A = ref.permute_bwd_ref(dxs, slot)
    np.testing.assert_allclose(got, lx.grad.numpy(), rtol=1e-13, atol=1e-15)
    assert (A >= np.abs(got) - 1e-12).all()
    lys, lw = torch.tensor(ys, requires_grad=True), torch.tensor(w, requires_grad=True)
    y_t = torch.where(oks, lys[ts.clamp(min=0)] * lw[..., None], 0.0).sum(1)
    got, A = ref.combine_ref(ys, w, slot)
    np.testing.assert_allclose(got, y_t.detach().numpy(), rtol=1e-13, atol=1e-15)
    y_t.backward(torch.tensor(dy))
    dys, dw, B = ref.combine_bwd_ref(dy, ys, w, perm, slot)
    np.testing.assert_allclose(dys, lys.grad.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(dw, lw.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert (B >= np.abs(dw) - 1e-12).all() and (dw[slot < 0] == 0).all() and (dys[perm < 0] == 0).all()
    if not skip:                                                     # nothing masked: the recipe as it was written
        np.testing.assert_array_equal(ref.permute_ref(x, perm, k), x[perm // k])
        np.testing.assert_allclose(ref.combine_ref(ys, w, slot)[0], (ys[slot] * w[..., None]).sum(1), rtol=1e-13)


def test_reference_on_the_hand_written_plan():
    """the plans of test_plan_reference_on_hand_written_cases (tests/test_zzz_moe_host.py), a token naming expert 2 twice included"""
    idx, perm, slot = ref.make_plan(0, 4, 2, 4, idx=[[2, 0], [0, 2], [3, 0], [2, 2]])
    np.testing.assert_array_equal(perm, [1, 2, 5, 0, 3, 6, 7, 4])
    np.testing.assert_array_equal(slot, [[3, 0], [1, 4], [7, 2], [5, 6]])
    x = np.arange(4.0)[:, None] * np.ones((1, 3)) + 1.0              # token t: a row of t + 1
    np.testing.assert_array_equal(ref.permute_ref(x, perm, 2)[:, 0], [1, 2, 3, 1, 2, 4, 4, 3])
    ys = 10.0 * np.arange(8.0)[:, None] * np.ones((1, 3))            # slot s: a row of 10 s
    w = np.array([[1, 2], [3, 4], [5, 6], [0.5, 0.25]])
    y, A = ref.combine_ref(ys, w, slot)
    np.testing.assert_array_equal(y[:, 0], [30 * 1 + 0, 10 * 3 + 40 * 4, 70 * 5 + 20 * 6, 50 * 0.5 + 60 * 0.25])
    np.testing.assert_array_equal(ref.permute_bwd_ref(ys, slot)[0][:, 0], [30, 50, 90, 110])
    dy = np.arange(1.0, 5.0)[:, None] * np.ones((1, 3))
    dys, dw, _ = ref.combine_bwd_ref(dy, ys, w, perm, slot)
    np.testing.assert_array_equal(dys[:, 0], [2 * 1, 3 * 2, 6 * 3, 1 * 1, 4 * 2, 0.5 * 4, 0.25 * 4, 5 * 3])
    np.testing.assert_array_equal(dw, 3 * dy[:, :1] * 10.0 * slot)
    idx, perm, slot = ref.make_plan(0, 4, 2, 2, idx=[[1, -1], [-1, 0], [7, 1], [0, -1]])      # -1 and an id past E are skipped
    np.testing.assert_array_equal(perm, [3, 6, 0, 5, -1, -1, -1, -1])
    np.testing.assert_array_equal(slot, [[2, -1], [-1, 0], [-1, 3], [1, -1]])
    xs = ref.permute_ref(x, perm, 2)
    np.testing.assert_array_equal(xs[:, 0], [2, 4, 1, 3, 0, 0, 0, 0])
    y, _ = ref.combine_ref(ys, w, slot)
    np.testing.assert_array_equal(y[:, 0], [20 * 1, 0 * 4, 30 * 6, 10 * 0.5])
    wn = w.copy()
    wn[0, 1] = NAN                                                   # a NaN weight at a skipped slot stays out of the sum
    np.testing.assert_array_equal(ref.combine_ref(ys, wn, slot)[0], y)
    np.testing.assert_array_equal(ref.valid(np.array([-1, 0, 7, 8, -2 ** 31, 2 ** 31 - 1]), 8), [False, True, True, False, False, False])
    _, perm, slot = ref.make_plan(0, 3, 2, 4, idx=np.full((3, 2), -1))                          # nothing valid
    assert (ref.combine_ref(ys[:6], w[:3], slot)[0] == 0).all() and (ref.permute_ref(x[:3], perm, 2) == 0).all()


# ---- the gates --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("T,k,D", [(37, 1, 7), (257, 4, 520), (257, 8, 1030), (129, 16, 64)])
def test_an_fp32_evaluation_is_inside_the_gates_and_a_wrong_one_is_not(dt, T, k, D):
    _, perm, slot = ref.make_plan(T + D, T, k, 8, skip=0.3)
    S = T * k
    ys, dy, w = ref.make_rows(1, S, D, dt), ref.make_rows(2, T, D, dt), ref.make_weights(3, T, k)
    # y = combine, dx = permute_bwd (w = None): fp32 in ascending j, rounded once
    for wts in (w, None):
        want, A = ref.combine_ref(ys, wts, slot)
        r = ref.y_ratio(ref.combine_f32(ys, wts, slot, dt), want, A, k, dt)
        assert r <= (0.5 if dt == "f32" else 1.0), r
        if k > 1:                                                    # one term dropped: two orders of magnitude outside
            assert ref.y_ratio(ref.combine_f32(ys, wts, slot, dt, drop=k - 1), want, A, k, dt) > 100.0
    # dys: one product rounded once
    dys, dw, B = ref.combine_bwd_ref(dy, ys, w, perm, slot)
    ok = ref.valid(perm, S)
    p = np.where(ok, perm, 0)
    got = ref.round_to(np.where(ok[:, None], w.reshape(-1)[p][:, None] * dy[p // k], np.float32(0)), dt)
    assert ref.dys_ratio(got, dys, dt) <= 1.0
    assert ref.dys_ratio(ref.round_to(got * np.float32(1 + 4 * ref.U[dt]), dt), dys, dt) > 1.0
    bad = got.copy()
    bad[0, 0] = NAN
    assert ref.dys_ratio(bad, dys, dt) == INF
    # dw: any order of fp32 summation
    for order in ("sequential", "pairwise"):
        assert ref.dw_ratio(ref.dw_f32(dy, ys, slot, order), dw, B, D) <= 0.25
    if D >= 520:                                                     # one column dropped from every dot product
        assert ref.dw_ratio(ref.dw_f32(dy, ys, slot, "pairwise", drop=D // 2), dw, B, D) > 1.0
    assert ref.exact(ys, ys.copy()) == 0.0 and ref.exact(ys, -ys) == INF
