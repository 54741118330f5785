"""CPU tests of the fused QK-norm + RoPE (include/nnop_hip_ext.h): the extension library loads and exports exactly its four functions, the
header is plain C99 with a 48-byte descriptor, the main library's frozen boundary is untouched, both entry points validate in the
header's order and return before any launch, the Python wrappers raise before any device work, the Julia shim binds the second library
with the header's types, and the reference the GPU tests are judged against (tests/qknr_ref.py) agrees with the project's two oracles
chained, with autograd of a plain fp64 formula and with finite differences.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qknr_ref as ref
from abi_util import ROOT, SHIM, c_params, strip_c_comments

EXT_HEADER = os.path.join(ROOT, "include", "nnop_hip_ext.h")
FOUR = {"nnop_ext_abi_version", "nnop_qk_norm_rope", "nnop_qk_norm_rope_bwd_workspace_bytes", "nnop_qk_norm_rope_bwd"}
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
INF, NAN = float("inf"), float("nan")


# ---- the library and its header -----------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_four_functions(pkg):
    lib = pkg._lib_ext.load()
    assert set(pkg._lib_ext.EXPORTED_SYMBOLS) == FOUR
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib_ext.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == FOUR, out
    header = strip_c_comments(open(EXT_HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header)) == FOUR
    assert lib.nnop_ext_abi_version() == pkg._lib_ext.EXT_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_EXT_ABI_VERSION (\d+)", header).group(1)) == 1
    # it links nothing from the main library
    needed = subprocess.run(["readelf", "-d", pkg._lib_ext.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip.so" not in needed
    for name in ("qk_norm_rope", "_qk_norm_rope", "grad_qk_norm_rope", "qk_norm_rope_into"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_main_library_boundary_is_unchanged(pkg):
    assert pkg._lib.ABI_VERSION == 7 and len(pkg._lib.EXPORTED_SYMBOLS) == 30
    assert not FOUR & set(pkg._lib.EXPORTED_SYMBOLS)
    main = pkg._lib.load()
    for name in FOUR:
        assert not hasattr(main, name)


def test_descriptor_is_48_bytes_and_matches_the_header(pkg):
    D = pkg._lib_ext.QknrDesc
    assert C.sizeof(D) == 48
    body = re.search(r"typedef struct nnop_qknr_desc \{(.*?)\} nnop_qknr_desc;", strip_c_comments(open(EXT_HEADER).read()), re.S).group(1)
    c_fields = []
    for ctype, names in re.findall(r"(int32_t|float)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            c_fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    want = [(n, "float" if t is C.c_float else "int32_t", 1) if not hasattr(t, "_length_") else (n, "int32_t", t._length_) for n, t in D._fields_]
    assert c_fields == want


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_ext.h"\n'
                 "int main(void){ nnop_qknr_desc d; (void)d; return (sizeof(nnop_qknr_desc) == 48 && NNOP_HIP_EXT_ABI_VERSION == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_missing_or_mismatched_library_fails_loudly(pkg, monkeypatch):
    monkeypatch.setattr(pkg._lib_ext, "_lib", None)
    monkeypatch.setattr(pkg._lib_ext, "EXT_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing, match="ext-ABI version 1"):
        pkg._lib_ext.load()
    monkeypatch.setattr(pkg._lib_ext, "LIB_PATH", "/nonexistent/libnnop_hip_ext.so")
    with pytest.raises(ImportError, match="no CPU or PyTorch fallback"):
        pkg._lib_ext.load()


# ---- validation: order and codes, before any launch -------------------------------------------------------------------------------------
def _desc(pkg, reserved=(0, 0), **kw):
    base = dict(dtype=2, w_dtype=0, cs_dtype=0, dim=128, seq=64, qh=4, kh=2, batch=2, eps=1e-6, offset=0.0)
    base.update(kw)
    d = pkg._lib_ext.QknrDesc(**base)
    d.reserved[0], d.reserved[1] = reserved
    return d


def _fwd(lib, d, ptrs=None):
    return lib.nnop_qk_norm_rope(C.byref(d) if d is not None else None, *(ptrs or [OK] * 8), None)


def _bwd(lib, d, ptrs=None, ws=OK, nbytes=1 << 40):
    return lib.nnop_qk_norm_rope_bwd(C.byref(d) if d is not None else None, *(ptrs or [OK] * 12), ws, C.c_size_t(nbytes), None)


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(w_dtype=3), "NNOP_ERR_DTYPE"),
    (dict(cs_dtype=7), "NNOP_ERR_DTYPE"),
    (dict(w_dtype=1), "NNOP_ERR_DTYPE"),                        # f16 weights with bf16 q
    (dict(cs_dtype=1), "NNOP_ERR_DTYPE"),
    (dict(dtype=0, w_dtype=2), "NNOP_ERR_DTYPE"),
    (dict(reserved=(1, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, -1)), "NNOP_ERR_OPTS"),
    (dict(eps=-1e-6), "NNOP_ERR_OPTS"),
    (dict(eps=INF), "NNOP_ERR_OPTS"),
    (dict(eps=NAN), "NNOP_ERR_OPTS"),
    (dict(offset=INF), "NNOP_ERR_OPTS"),
    (dict(offset=-INF), "NNOP_ERR_OPTS"),
    (dict(offset=NAN), "NNOP_ERR_OPTS"),
    (dict(dim=127), "NNOP_ERR_SHAPE"),
    (dict(dim=514), "NNOP_ERR_SHAPE"),
    (dict(dim=1024), "NNOP_ERR_SHAPE"),
    (dict(dim=0), "NNOP_ERR_SHAPE"),
    (dict(dim=-2), "NNOP_ERR_SHAPE"),
    (dict(seq=0), "NNOP_ERR_SHAPE"),
    (dict(qh=0), "NNOP_ERR_SHAPE"),
    (dict(kh=-1), "NNOP_ERR_SHAPE"),
    (dict(batch=0), "NNOP_ERR_SHAPE"),
    (dict(batch=2 ** 20, seq=2 ** 20), "NNOP_ERR_SHAPE"),       # more head rows than one launch takes
    (dict(batch=2 ** 15, seq=2 ** 15, qh=1, kh=1), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, reserved=(1, 0), dim=3), "NNOP_ERR_DTYPE"),
    (dict(reserved=(1, 0), dim=3), "NNOP_ERR_OPTS"),
    (dict(eps=NAN, seq=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_ext.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert [_fwd(lib, d), _bwd(lib, d)] == [want] * 2
    assert [_fwd(lib, d, [NULL] * 8), _bwd(lib, d, [NULL] * 12, NULL, 0)] == [want] * 2      # the descriptor is judged before the pointers
    assert lib.nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(d)) == 0


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    lib, L = pkg._lib_ext.load(), pkg._lib
    for ok in (dict(), dict(dim=2), dict(dim=512), dict(dim=6), dict(dim=80), dict(eps=0.0), dict(offset=1.0), dict(offset=-3.5),
               dict(dtype=0), dict(dtype=1, w_dtype=1, cs_dtype=1), dict(w_dtype=2, cs_dtype=2),
               dict(batch=2 ** 14, seq=2 ** 15, qh=2, kh=1)):            # 3 * 2^29 head rows: still one launch
        d = _desc(pkg, **ok)
        assert [_fwd(lib, d, [NULL] * 8), _bwd(lib, d, [NULL] * 12, NULL, 0)] == [L.NNOP_ERR_NULL] * 2, ok
        assert lib.nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(d)) > 0
    assert _fwd(lib, None) == L.NNOP_ERR_NULL and _bwd(lib, None) == L.NNOP_ERR_NULL
    assert lib.nnop_qk_norm_rope_bwd_workspace_bytes(None) == 0


def test_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_ext.load(), pkg._lib
    at = lambda off: C.c_void_p(0x7f0000001000 + off)
    for dtype, w_dtype, cs_dtype in ((2, 0, 0), (2, 2, 2), (1, 0, 1), (0, 0, 0)):
        es, ws_, cs = (4 if t == 0 else 2 for t in (dtype, w_dtype, cs_dtype))
        d = _desc(pkg, dtype=dtype, w_dtype=w_dtype, cs_dtype=cs_dtype)
        need = lib.nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(d))
        # forward: q_out, k_out, q, k, wq, wk, cos, sin;  pullback: dq, dk, dwq, dwk, dq_out, dk_out, q, k, wq, wk, cos, sin
        for fn, aligns in ((_fwd, [es, es, es, es, ws_, ws_, cs, cs]), (_bwd, [es, es, 4, 4, es, es, es, es, ws_, ws_, cs, cs])):
            for pos, a in enumerate(aligns):
                b = [OK] * len(aligns)
                b[pos] = NULL
                assert fn(lib, d, b) == L.NNOP_ERR_NULL, (fn.__name__, pos)
                c = [at(1)] * len(aligns)                        # NULL is judged before alignment
                c[pos] = NULL
                assert fn(lib, d, c) == L.NNOP_ERR_NULL
                c = [OK] * len(aligns)
                c[pos] = at(a // 2)                              # aligned to half of what is needed
                assert fn(lib, d, c) == L.NNOP_ERR_ALIGN, (fn.__name__, pos, a)
        assert _bwd(lib, d, ws=NULL) == L.NNOP_ERR_NULL
        assert _bwd(lib, d, ws=at(8)) == L.NNOP_ERR_ALIGN
        assert _bwd(lib, d, ws=at(8), nbytes=0) == L.NNOP_ERR_ALIGN          # alignment before size
        assert _bwd(lib, d, nbytes=need - 1) == L.NNOP_ERR_WORKSPACE
        assert _bwd(lib, d, nbytes=0) == L.NNOP_ERR_WORKSPACE
        ptrs = [at(1)] * 12
        assert _bwd(lib, d, ptrs, nbytes=0) == L.NNOP_ERR_ALIGN              # ... and the pointers before the workspace


def test_workspace_bytes_is_a_function_of_the_descriptor(pkg):
    lib = pkg._lib_ext.load()
    wb = lambda **kw: lib.nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(_desc(pkg, **kw)))
    assert wb(batch=1, seq=1, qh=1, kh=1, dim=64) == 2 * 64 * 4              # one partial row per tensor
    assert wb(batch=4, seq=4096, qh=32, kh=8, dim=128) == 2 * 1024 * 128 * 4  # the cap: 1024 partial rows per tensor
    assert wb(dtype=0) == wb(dtype=2) == wb(dtype=2, w_dtype=2, cs_dtype=2)   # fp32 partials whatever the dtypes
    assert wb() % 16 == 0


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    B, QH, KH, L, D = 2, 3, 1, 5, 16
    q, k, w, cs = torch.ones(B, QH, L, D), torch.ones(B, KH, L, D), torch.ones(D), torch.ones(B, L, D)
    calls = lambda q, k, wq, wk, cos, sin, **kw: (
        lambda: pkg.qk_norm_rope(q, k, wq, wk, cos=cos, sin=sin, **kw), lambda: pkg._qk_norm_rope(q, k, wq, wk, cos, sin, **kw),
        lambda: pkg.grad_qk_norm_rope((q, k), q, k, wq, wk, cos, sin, **kw), lambda: pkg.qk_norm_rope_into(q, k, q, k, wq, wk, cos, sin, **kw),
        lambda: pkg.grad_qk_norm_rope_into(q, k, wq, wk, (q, k), q, k, wq, wk, cos, sin, **kw))
    for call in calls(q, k, w, w, cs, cs) + calls(q.clone().requires_grad_(True), k, w, w, cs, cs)[:1]:
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    q, k, w, cs = mk(B, QH, L, D), mk(B, KH, L, D), mk(D), mk(B, L, D)
    type_errors = [
        (mk(QH, L, D), k, w, w, cs, cs), ([1.0], k, w, w, cs, cs), (mk(B, QH, L, D, dt=torch.float64), k, w, w, cs, cs),
        (q, mk(B, KH, L, D, dt=torch.float16), w, w, cs, cs), (q, k, mk(D, 1), w, cs, cs), (q, k, w, mk(D, dt=torch.float16), cs, cs),
        (q, k, mk(D, dt=torch.bfloat16), mk(D, dt=torch.bfloat16), cs, cs), (q, k, w, w, mk(B, L, D, dt=torch.float16), mk(B, L, D, dt=torch.float16)),
        (q, k, w, w, cs, mk(B, L, D, dt=torch.float64))]
    for args in type_errors:
        for call in calls(*args):
            with pytest.raises(TypeError):
                call()
    nnop_errors = [
        ((q, mk(B, KH, L + 1, D), w, w, cs, cs), {}, "AssertionError"), ((q, mk(B + 1, KH, L, D), w, w, cs, cs), {}, "AssertionError"),
        ((q, k, mk(D + 2), w, cs, cs), {}, "length"), ((q, k, w, w, mk(B, L + 1, D), cs), {}, "shape"), ((q, k, w, w, cs, mk(B, L, D // 2)), {}, "shape"),
        ((mk(B, QH, L, 7), mk(B, KH, L, 7), mk(7), mk(7), mk(B, L, 7), mk(B, L, 7)), {}, "even"),
        ((mk(1, 1, 1, 514), mk(1, 1, 1, 514), mk(514), mk(514), mk(1, 1, 514), mk(1, 1, 514)), {}, "512"),
        ((mk(B, QH, 0, D), mk(B, KH, 0, D), w, w, mk(B, 0, D), mk(B, 0, D)), {}, "non-empty"),
        ((q, k, w, w, cs, cs), dict(eps=-1.0), "eps"), ((q, k, w, w, cs, cs), dict(eps=NAN), "eps"), ((q, k, w, w, cs, cs), dict(offset=INF), "offset")]
    for args, kw, match in nnop_errors:
        for call in calls(*args, **kw):
            with pytest.raises(pkg.NNopError, match=match) as e:
                call()
            if kw:
                assert e.value.status == pkg._lib.NNOP_ERR_OPTS
    with pytest.raises(TypeError, match="eps"):
        pkg.qk_norm_rope(q, k, w, w, cos=cs, sin=cs, eps="1e-6")
    with pytest.raises(TypeError, match="dq2"):
        pkg.grad_qk_norm_rope((mk(B, QH, L + 1, D), k), q, k, w, w, cs, cs)
    with pytest.raises(pkg.NNopError, match="q_out"):
        pkg.qk_norm_rope_into(mk(B, QH, L, D).transpose(1, 2), k, q, k, w, w, cs, cs)
    with pytest.raises(pkg.NNopError, match="dwq"):
        pkg.grad_qk_norm_rope_into(q, k, mk(D, dt=torch.bfloat16), w, (q, k), q, k, w, w, cs, cs)
    d = pkg.qknorm._desc(torch.zeros(2, 3, 5, 16, dtype=torch.bfloat16), torch.zeros(2, 1, 5, 16), torch.zeros(16), torch.zeros(1, dtype=torch.bfloat16), 1e-5, 1.0)
    assert (d.dtype, d.w_dtype, d.cs_dtype, d.dim, d.seq, d.qh, d.kh, d.batch) == (2, 0, 2, 16, 5, 3, 1, 2)
    assert abs(d.eps - 1e-5) < 1e-12 and d.offset == 1.0 and tuple(d.reserved) == (0, 0)


def test_workmodel_bytes(pkg):
    wb = pkg.workmodel.qknr_bytes
    qk = 2 * 4 * 4096 * 128 * (32 + 8)
    tables = 2 * 4 * 4 * 4096 * 64 + 2 * 4 * 128
    assert wb(128, 4096, 32, 8, 4, 2) == 2 * qk + tables
    assert wb(128, 4096, 32, 8, 4, 2, bwd=True, n_parts=1024) == 3 * qk + tables + 2 * 4 * 128 + 2 * 2 * 1024 * 4 * 128
    assert wb(2, 1, 1, 1, 1, 4, cs_itemsize=2, w_itemsize=2) == 2 * 4 * 2 * 2 + 2 * 2 * 1 + 2 * 2 * 2


# ---- the reference --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,offset", [(16, 0.0), (6, 1.0), (80, 0.5)])
def test_reference_is_the_two_oracles_chained(D, offset):
    from oracle.naive_norms import naive_rms_norm, naive_rms_norm_grads
    from oracle.naive_rope import pairwise_llama_rope
    x = ref.make_inputs(D, 2, 3, 2, 7, D)
    eps = 1e-5
    q2, k2 = ref.qknr_ref(x["q"], x["k"], x["wq"], x["wk"], x["cos"], x["sin"], eps, offset)
    nq, nk = naive_rms_norm(x["q"], x["wq"], offset=offset, eps=eps)[0], naive_rms_norm(x["k"], x["wk"], offset=offset, eps=eps)[0]
    oq, ok_ = pairwise_llama_rope(nq, nk, x["cos"], x["sin"])
    np.testing.assert_allclose(q2, oq, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(k2, ok_, rtol=1e-13, atol=1e-13)
    assert not np.array_equal(x["cos"][0], x["cos"][1])          # the positions differ per batch
    # the pullback: the rope oracle with sin_sign = -1, then the norm oracle's gradients
    dq, dk, dwq, dwk = ref.qknr_grad_ref(x["dq2"], x["dk2"], x["q"], x["k"], x["wq"], x["wk"], x["cos"], x["sin"], eps, offset)
    gq, gk = pairwise_llama_rope(x["dq2"].astype(np.float64), x["dk2"].astype(np.float64), x["cos"], x["sin"], sin_sign=-1.0)
    for got, gw, g, xx, w in ((dq, dwq, gq, x["q"], x["wq"]), (dk, dwk, gk, x["k"], x["wk"])):
        rdx, rdw = naive_rms_norm_grads(g.reshape(-1, D), xx.reshape(-1, D), w, offset=offset, eps=eps)
        np.testing.assert_allclose(got.reshape(-1, D), rdx, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(gw, rdw, rtol=1e-12, atol=1e-12)


def _torch_formula(q, k, wq, wk, cos, sin, eps, offset):
    outs = []
    h = q.shape[-1] // 2
    c, s = cos[:, None, :, :h], sin[:, None, :, :h]
    for x, w in ((q, wq), (k, wk)):
        n = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * (w + offset)
        outs.append(torch.cat([n[..., :h] * c - n[..., h:] * s, n[..., h:] * c + n[..., :h] * s], -1))
    return outs


@pytest.mark.parametrize("D,offset", [(16, 0.0), (6, 1.0)])
def test_reference_gradients_match_autograd_and_finite_differences(D, offset):
    x = ref.make_inputs(100 + D, 2, 2, 1, 3, D)
    eps = 1e-3
    t = {n: torch.tensor(np.asarray(v, np.float64)) for n, v in x.items()}
    leaves = [t[n].clone().requires_grad_(True) for n in ("q", "k", "wq", "wk")]
    q2, k2 = _torch_formula(*leaves, t["cos"], t["sin"], eps, offset)
    r2 = ref.qknr_ref(x["q"], x["k"], x["wq"], x["wk"], x["cos"], x["sin"], eps, offset)
    np.testing.assert_allclose(q2.detach().numpy(), r2[0], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(k2.detach().numpy(), r2[1], rtol=1e-13, atol=1e-13)
    ((q2 * t["dq2"]).sum() + (k2 * t["dk2"]).sum()).backward()
    grads = ref.qknr_grad_ref(x["dq2"], x["dk2"], x["q"], x["k"], x["wq"], x["wk"], x["cos"], x["sin"], eps, offset)
    for got, leaf in zip(grads, leaves):
        np.testing.assert_allclose(got, leaf.grad.numpy(), rtol=1e-11, atol=1e-12)
    # central differences of L = <q', dq'> + <k', dk'> in every input
    def loss(**repl):
        a = {n: np.asarray(repl.get(n, x[n]), np.float64) for n in ("q", "k", "wq", "wk")}
        o = ref.qknr_ref(a["q"], a["k"], a["wq"], a["wk"], x["cos"], x["sin"], eps, offset)
        return float((o[0] * x["dq2"]).sum() + (o[1] * x["dk2"]).sum())
    rng = np.random.default_rng(0)
    hstep = 1e-6
    for name, g in zip(("q", "k", "wq", "wk"), grads):
        base = np.asarray(x[name], np.float64)
        for _ in range(6):
            idx = tuple(rng.integers(0, n) for n in base.shape)
            e = np.zeros_like(base)
            e[idx] = hstep
            fd = (loss(**{name: base + e}) - loss(**{name: base - e})) / (2 * hstep)
            assert abs(fd - g[idx]) < 1e-7 * max(1.0, abs(g[idx])), (name, idx, fd, g[idx])


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_gates_pass_one_rounding_and_fail_four_ulp(dt):
    """an fp32 evaluation rounded once is inside the gates; the same result 4 units in the last place off (16-bit) is not"""
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    x = ref.make_inputs(7, 2, 3, 1, 37, 64)
    rnd = {n: torch.tensor(v).to(tdt) for n, v in x.items() if n in ("q", "k", "dq2", "dk2")}
    x64 = dict(x, **{n: v.double().numpy() for n, v in rnd.items()})
    r = ref.qknr_ref(x64["q"], x64["k"], x["wq"], x["wk"], x["cos"], x["sin"], 1e-6, 1.0)
    f32 = {n: torch.tensor(np.asarray(v, np.float32)) for n, v in x64.items()}
    once = _torch_formula(f32["q"], f32["k"], f32["wq"], f32["wk"], f32["cos"], f32["sin"], 1e-6, 1.0)[0].to(tdt)
    assert ref.out_ratio(once.double().numpy(), r[0], dt) <= 0.5
    if dt != "f32":
        off = (once.view(torch.int16).to(torch.int32) + 4).to(torch.int16).view(tdt)
        assert ref.out_ratio(off.double().numpy(), r[0], dt) > 1.0
    bad = once.double().numpy().copy()
    bad[0, 0, 0, 0] = np.nan
    assert ref.out_ratio(bad, r[0], dt) == INF
    g = ref.qknr_grad_ref(x64["dq2"], x64["dk2"], x64["q"], x64["k"], x["wq"], x["wk"], x["cos"], x["sin"], 1e-6, 1.0)
    rows = 2 * 3 * 37
    assert ref.dw_ratio(g[2].astype(np.float32), g[2], rows) <= 0.1
    assert ref.dw_ratio(g[2] * (1 + 3e-4) + 2e-5 * np.abs(g[2]).max() + 2e-6 * rows, g[2], rows) > 1.0


# ---- the Julia shim ---------------------------------------------------------------------------------------------------------------------
JL = {"const nnop_qknr_desc*": "Ptr{QknrDesc}", "size_t": "Csize_t", "nnop_stream_t": "Ptr{Cvoid}"}


def _jl_type(param):
    ctype = re.sub(r"\s*\w+$", "", param).strip()                # drop the parameter's name
    return JL.get(ctype) or ("Ptr{Cvoid}" if ctype.endswith("*") else None)


def test_julia_shim_binds_the_second_library_with_the_headers_types():
    header = strip_c_comments(open(EXT_HEADER).read())
    shim = re.sub(r"#[^\n]*", "", open(SHIM).read())
    assert re.search(r"\nfunction libnnop_ext\(\)", shim) and "NNOP_HIP_EXT_LIB" in open(SHIM).read()
    assert re.search(r"const EXT_ABI_VERSION = 1\b", shim) and re.search(r"dlsym\(h, :nnop_ext_abi_version\)", shim)
    m = re.search(r"struct QknrDesc\n(.*?)\nend", shim, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == (
        "dtype::Int32; w_dtype::Int32; cs_dtype::Int32 dim::Int32; seq::Int32; qh::Int32; kh::Int32; batch::Int32 "
        "eps::Float32; offset::Float32 reserved::NTuple{2, Int32}")
    for name, ret in (("nnop_qk_norm_rope", "Cint"), ("nnop_qk_norm_rope_bwd", "Cint"), ("nnop_qk_norm_rope_bwd_workspace_bytes", "Csize_t")):
        call = re.search(r"ccall\(Libdl\.dlsym\(libnnop_ext\(\), :" + name + r"\), " + ret + r",\s*\((.*?)\),\s*\n?\s*d[,)]", shim, re.S)
        assert call, f"the Julia shim does not call {name} through libnnop_ext()"
        types = [t.strip() for t in call.group(1).split(",") if t.strip()]
        assert types == [_jl_type(p) for p in c_params(header, name)], name
    # the calls into the second library never go through libnnop(), whose symbols are the main header's
    assert not re.search(r"ccall\(\(:nnop_(qk_norm_rope|ext_abi_version)", shim)
    assert re.search(r"rrule\(::typeof\(qk_norm_rope\)", shim) and re.search(r"export [^\n]*\bqk_norm_rope\b", shim)
