"""CPU tests of logit soft-capping: the reference (tests/attn_ref.py) against torch fp64 autograd, that the cap changes the results
of the GPU tests' inputs by far more than the parity tolerance, the exports and the unchanged ABI, the validation order of
nnop_fa_fwd_softcap / nnop_fa_bwd_softcap, the kernel-form rules, the Julia shim and the Python argument checks."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import softcap_cases
from abi_util import HEADER, SHIM, c_params, fa_desc, fa_opts, jl_ccall_types, strip_c_comments
from attn_ref import attention_fwd, attention_grads, window_keep


# ---- the reference against torch autograd ----------------------------------------------------------------------------------------
def _torch_capped(q, k, v, pair, c, causal, kpad_mask, window, sinks=None):
    B, QH, QL, E = q.shape
    KH, KL = k.shape[1], k.shape[2]
    ke, ve = k.repeat_interleave(QH // KH, dim=1), v.repeat_interleave(QH // KH, dim=1)
    s = q @ ke.transpose(-1, -2) / np.sqrt(E)
    x = c * torch.tanh(s / c)
    if pair is not None:
        x = x + pair.permute(0, 3, 2, 1)                       # after the cap: never capped
    vis = torch.from_numpy(window_keep(QL, KL, window, causal))[None, None]
    if kpad_mask is not None:
        vis = vis & torch.from_numpy(kpad_mask)[:, None, None, :]
    x = x.masked_fill(~vis, float("-inf"))
    if sinks is not None:
        col = sinks[None, :, None, None].expand(B, QH, QL, 1)
        return torch.softmax(torch.cat([x, col], dim=-1), dim=-1)[..., :KL] @ ve
    return torch.softmax(x, dim=-1) @ ve


@pytest.mark.parametrize("c", [0.5, 1.0, 30.0])
@pytest.mark.parametrize("sinks", [False, True])
def test_reference_matches_torch_autograd(c, sinks):
    """GQA 4:2, causal + pair + key padding (no dead row: a valid prefix of keys), with and without sinks and a window"""
    B, QH, KH, QL, KL, E = 2, 4, 2, 9, 11, 8
    rng = np.random.default_rng(int(c * 10) + sinks)
    q, k, v, do = (rng.standard_normal(s) for s in ((B, QH, QL, E), (B, KH, KL, E), (B, KH, KL, E), (B, QH, QL, E)))
    q = q * 3.0                                                # scores well into the tanh's curved part at c <= 1
    pair = rng.standard_normal((B, KL, QL, QH))
    mask = np.ones((B, KL), bool)
    mask[1, -3:] = False
    window = (5, 0) if sinks else None
    sk = np.array([0.3, -1.0, 2.0, 0.0]) if sinks else None
    kw = dict(softcap=c, causal=True, kpad_mask=mask, window=window, sinks=sk)
    o, ms, ls = attention_fwd(q, k, v, pair, **kw)
    grads = attention_grads(q, k, v, do, pair, **kw)

    t = lambda x: torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tq, tk, tv, tp = t(q), t(k), t(v), t(pair)
    ts = t(sk) if sinks else None
    to = _torch_capped(tq, tk, tv, tp, c, True, mask, window, ts)
    to.backward(torch.tensor(do))
    np.testing.assert_allclose(o, to.detach().numpy(), rtol=1e-10, atol=1e-12)
    for got, ref in zip(grads, (tq, tk, tv, tp) + ((ts,) if sinks else ())):
        np.testing.assert_allclose(got, ref.grad.numpy(), rtol=1e-9, atol=1e-11)
    # ms, ls: row max and sum-exp of the capped, biased, masked logits (and the sink)
    s = np.einsum("bhie,bhje->bhij", q, np.repeat(k, QH // KH, axis=1)) / np.sqrt(E)
    x = c * np.tanh(s / c) + pair.transpose(0, 3, 2, 1)
    vis = window_keep(QL, KL, window, True)[None, None] & mask[:, None, None, :]
    x = np.where(vis, x, -np.inf)
    if sinks:
        x = np.concatenate([x, np.broadcast_to(sk[None, :, None, None], (B, QH, QL, 1))], axis=-1)
    np.testing.assert_allclose(ms, x.max(-1))
    np.testing.assert_allclose(ls, np.exp(x - x.max(-1, keepdims=True)).sum(-1), rtol=1e-12)


def test_dpair_is_not_scaled_by_the_tanh_derivative():
    """dpair = dS while dq goes through 1 - tanh^2: at a saturated cap dq vanishes and dpair does not"""
    rng = np.random.default_rng(3)
    q, k, v, do = (rng.standard_normal((1, 2, 6, 4)) for _ in range(4))
    pair = rng.standard_normal((1, 6, 6, 2))
    dq, dk, dv, dp = attention_grads(q * 400.0, k, v, do, pair, softcap=0.5, causal=False)
    # (every |s| / c of these inputs is > 6: 1 - tanh^2 < 4 exp(-12) = 2.5e-5 of the O(1) terms dpair keeps)
    assert np.abs(dp).max() > 0.1 and np.abs(dq).max() < 1e-4 * np.abs(dp).max() and np.abs(dk).max() < 1e-2 * np.abs(dp).max()


def test_dead_rows_keep_their_convention():
    rng = np.random.default_rng(4)
    q, k, v, do = (rng.standard_normal((1, 2, 6, 4)) for _ in range(4))
    mask = np.ones((1, 6), bool)
    mask[0, :2] = False                                        # causal rows 0, 1 see no key
    o, ms, ls = attention_fwd(q, k, v, softcap=1.0, causal=True, kpad_mask=mask)
    dq = attention_grads(q, k, v, do, softcap=1.0, causal=True, kpad_mask=mask)[0]
    assert np.isnan(o[:, :, :2]).all() and np.isneginf(ms[:, :, :2]).all() and (dq[:, :, :2] == 0).all()
    assert np.isfinite(o[:, :, 2:]).all()
    # sinks: head 0 has none (sigma = -inf), so its rows 0, 1 stay dead; head 1's see their sink alone
    sinks = np.array([-np.inf, 0.5])
    o, ms, ls = attention_fwd(q, k, v, softcap=1.0, causal=True, kpad_mask=mask, sinks=sinks)
    grads = attention_grads(q, k, v, do, softcap=1.0, causal=True, kpad_mask=mask, sinks=sinks)
    assert np.isnan(o[:, 0, :2]).all() and np.isneginf(ms[:, 0, :2]).all() and (o[:, 1, :2] == 0).all() and (ms[:, 1, :2] == 0.5).all()
    assert all(np.isfinite(g).all() for g in grads if g is not None)
    assert (grads[0][:, :, :2] == 0).all() and grads[4][0] == 0 and grads[4][1] != 0


# ---- the cap must bite: a kernel that ignores it cannot pass the GPU tests ---------------------------------------------------------
def _bite(d, causal, cap):
    n = lambda t: t.double().numpy()
    o_c = attention_fwd(n(d["q"]), n(d["k"]), n(d["v"]), softcap=cap, causal=causal)[0]
    o_u = attention_fwd(n(d["q"]), n(d["k"]), n(d["v"]), causal=causal)[0]
    return np.abs(o_c - o_u).max() / np.abs(o_u).max()


@pytest.mark.parametrize("case", softcap_cases.parity_grid(), ids=lambda c: "{}-E{}-c{}-L{}x{}-cap{}".format(*c))
def test_the_cap_changes_the_grid_inputs_results(case):
    dt, E, causal, QL, KL, cap = case
    bite = _bite(softcap_cases.grid_inputs(case, "cpu"), causal, cap)
    if causal and QL == 1:
        # the one row sees the one key 0: P = 1 whatever its logit, so no cap can show (the case stays in the grid for the kernels'
        # single-row, single-key path; the same lengths meet causal = False at other E, checked below)
        assert bite == 0
    else:
        assert bite > 0.05


@pytest.mark.parametrize("case", softcap_cases.REALISTIC, ids=lambda c: "{}-E{}-L{}x{}-cap{}".format(*c))
def test_the_realistic_cap_changes_its_inputs_results(case):
    assert _bite(softcap_cases.realistic_inputs(case, "cpu"), False, case[4]) > 0.05


def test_grid_covers_what_it_should():
    g = softcap_cases.parity_grid()
    for E in softcap_cases.EMBS:
        sub = [c for c in g if c[1] == E]
        assert {c[0] for c in sub} == set(softcap_cases.DTYPES) and {c[2] for c in sub} == {False, True}
        assert {(c[0], c[2]) for c in sub} == {(dt, cz) for dt in softcap_cases.DTYPES for cz in (False, True)}
    assert {c[5] for c in g} == set(softcap_cases.CAPS)
    assert {(c[3], c[4]) for c in g if c[1] < 128} == set(softcap_cases.LENS)
    assert sum(1 for c in g if c[3] == 1 and not c[2]) >= 2


# ---- exports, ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(pkg):
    header = strip_c_comments(open(HEADER).read())
    lib = pkg._lib.load()
    for name in ("nnop_fa_fwd_softcap", "nnop_fa_bwd_softcap"):
        assert re.search(r"\bint " + name + r"\s*\(", header)
        assert name in pkg._lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    for name in ("nnop_debug_fwd_form_cap", "nnop_debug_bwd_form_cap"):
        assert name in pkg._lib.DEBUG_SYMBOLS and hasattr(lib, name) and name not in header
    # the prototypes: the sinks calls plus one float behind (sinks | dsinks)
    proto = lambda n: re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(proto("nnop_fa_fwd_softcap")) == norm(proto("nnop_fa_fwd_sinks").replace("const float* sinks,", "const float* sinks, float softcap,"))
    assert norm(proto("nnop_fa_bwd_softcap")) == norm(proto("nnop_fa_bwd_sinks").replace("float* dsinks,", "float* dsinks, float softcap,"))
    assert lib.nnop_fa_fwd_softcap.argtypes[3] is C.c_float and lib.nnop_fa_bwd_softcap.argtypes[4] is C.c_float


def test_abi_version_and_options_layout_are_unchanged(pkg):
    lib = pkg._lib.load()
    assert lib.nnop_abi_version() == 7 == pkg._lib.ABI_VERSION
    header = open(HEADER).read()
    assert re.search(r"#define\s+NNOP_HIP_ABI_VERSION\s+7\b", header)
    m = re.search(r"typedef struct nnop_fa_opts \{(.*?)\} nnop_fa_opts;", header, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int32_t window_left; int32_t window_right; int32_t reserved[6];"
    assert C.sizeof(pkg._lib.FaOpts) == 32
    assert [f[0] for f in pkg._lib.FaOpts._fields_] == ["window_left", "window_right", "reserved"]


# ---- validation (NULL / fake tensors: every call fails a check before any launch) ---------------------------------------------------
def _fwd(lib, d, opts, cap, sinks=None, tensors=None):
    t = C.c_void_p(tensors) if tensors else C.c_void_p(0)
    op = C.byref(opts) if opts is not None else None
    return lib.nnop_fa_fwd_softcap(C.byref(d), op, C.c_void_p(sinks), C.c_float(cap), t, t, t, t, t, t, None, None, None)


def _bwd(lib, d, opts, cap, sinks=None, dsinks=None, tensors=None):
    t = C.c_void_p(tensors) if tensors else C.c_void_p(0)
    op = C.byref(opts) if opts is not None else None
    return lib.nnop_fa_bwd_softcap(C.byref(d), op, C.c_void_p(sinks), C.c_void_p(dsinks), C.c_float(cap), t, t, t, None, t, t, t, t,
                                   t, t, t, None, None, t, C.c_size_t(1 << 40), None)


def _both(lib, d, opts, cap, **kw):
    return _fwd(lib, d, opts, cap, **{k: v for k, v in kw.items() if k != "dsinks"}), _bwd(lib, d, opts, cap, **kw)


BAD_CAPS = [-1.0, -1e-30, float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("cap", BAD_CAPS)
def test_bad_cap_is_err_opts_before_null_pointers(pkg, cap):
    lib = pkg._lib.load()
    E = pkg._lib
    assert _both(lib, fa_desc(pkg), None, cap) == (E.NNOP_ERR_OPTS,) * 2                      # NULL tensors: the cap comes first
    assert _both(lib, fa_desc(pkg), fa_opts(pkg, 3, 0), cap, sinks=0x1001) == (E.NNOP_ERR_OPTS,) * 2   # ... and before alignment


def test_zero_and_positive_caps_pass_the_cap_check(pkg):
    lib = pkg._lib.load()
    E = pkg._lib
    for cap in (0.0, -0.0, 1e-30, 0.5, 50.0, 3e38):
        assert _both(lib, fa_desc(pkg), None, cap) == (E.NNOP_ERR_NULL,) * 2                  # the next check in line
    fake = 0x10000
    assert _fwd(lib, fa_desc(pkg), None, 30.0, sinks=0x1002, tensors=fake) == E.NNOP_ERR_ALIGN
    assert _bwd(lib, fa_desc(pkg), None, 30.0, sinks=0x1000, dsinks=0x2001, tensors=fake) == E.NNOP_ERR_ALIGN
    assert _bwd(lib, fa_desc(pkg), None, 30.0, sinks=0x1000, dsinks=None, tensors=fake) == E.NNOP_ERR_NULL


@pytest.mark.parametrize("kw,status", [
    (dict(emb_k=32), "NNOP_ERR_EMB_MISMATCH"),
    (dict(qh=6, kh=4), "NNOP_ERR_HEADS"),
    (dict(dtype=7), "NNOP_ERR_DTYPE"),
    (dict(ql=0), "NNOP_ERR_SHAPE"),
])
def test_descriptor_then_options_then_cap(pkg, kw, status):
    lib = pkg._lib.load()
    E = pkg._lib
    # a bad descriptor reports its own code whatever the options and the cap are
    assert _both(lib, fa_desc(pkg, **kw), fa_opts(pkg, reserved=[1]), -1.0) == (getattr(E, status),) * 2
    # bad options come before a bad cap: both are NNOP_ERR_OPTS, so tell them apart by fixing one at a time
    assert _both(lib, fa_desc(pkg), fa_opts(pkg, reserved=[0, 2]), 1.0) == (E.NNOP_ERR_OPTS,) * 2
    assert _both(lib, fa_desc(pkg), fa_opts(pkg, left=-3), 1.0) == (E.NNOP_ERR_OPTS,) * 2
    assert _both(lib, fa_desc(pkg), fa_opts(pkg, reserved=[0, 2]), float("nan")) == (E.NNOP_ERR_OPTS,) * 2
    assert _both(lib, fa_desc(pkg), fa_opts(pkg), 1.0) == (E.NNOP_ERR_NULL,) * 2


def test_cap_zero_is_the_sinks_call(pkg):
    lib = pkg._lib.load()
    null = C.c_void_p(0)
    for d, opts in ((fa_desc(pkg), None), (fa_desc(pkg), fa_opts(pkg, 3, 0)), (fa_desc(pkg, emb_k=32), None),
                    (fa_desc(pkg), fa_opts(pkg, reserved=[1]))):
        op = C.byref(opts) if opts is not None else None
        for sinks in (None, 0x1001):
            sk = C.c_void_p(sinks)
            f = lib.nnop_fa_fwd_sinks(C.byref(d), op, sk, null, null, null, null, null, null, null, null, null)
            b = lib.nnop_fa_bwd_sinks(C.byref(d), op, sk, null, *([null] * 13), null, 0, null)
            assert (_fwd(lib, d, opts, 0.0, sinks=sinks), _bwd(lib, d, opts, 0.0, sinks=sinks)) == (f, b)


def test_workspace_queries_take_no_cap(pkg):
    header = strip_c_comments(open(HEADER).read())
    assert re.search(r"size_t nnop_fa_bwd_workspace_bytes\(const nnop_fa_desc\* d\);", header)
    assert re.search(r"size_t nnop_fa_bwd_workspace_bytes_pair\(const nnop_fa_desc\* d\);", header)


# ---- form rules ----------------------------------------------------------------------------------------------------------------
def test_capped_problems_run_the_32_row_or_plain_hip_kernels(pkg):
    lib = pkg._lib.load()
    L = pkg._lib
    for dt in (L.NNOP_BF16, L.NNOP_F16):
        for E in (64, 128):
            for causal in (0, 1):
                d = fa_desc(pkg, dtype=dt, emb=E, ql=4096, kl=4096, qh=8, kh=8, batch=4, causal=causal)
                # without a cap this problem runs the duo / w64 forms and the w64 backward: the cap moves it
                assert lib.nnop_debug_fwd_form_ex(C.byref(d), None, 0, 0) in (2, 4)
                assert lib.nnop_debug_bwd_form_ex(C.byref(d), None, 0, 0) == 3
                for mask in (0, 1):
                    assert lib.nnop_debug_fwd_form_cap(C.byref(d), None, C.c_float(30.0), 0, mask) == 0
                    assert lib.nnop_debug_bwd_form_cap(C.byref(d), None, C.c_float(30.0), 0, mask) == 0
                assert lib.nnop_debug_fwd_form_cap(C.byref(d), None, C.c_float(30.0), 1, 0) == 0
    d8 = fa_desc(pkg, emb=8)
    assert lib.nnop_debug_fwd_form_cap(C.byref(d8), None, C.c_float(1.0), 0, 0) == 3
    assert lib.nnop_debug_bwd_form_cap(C.byref(d8), None, C.c_float(1.0), 0, 0) == 0
    assert pkg._lib.fwd_form(fa_desc(pkg, ql=4096, kl=4096), softcap=30.0) == "fa_fwd_cap_kernel"
    assert pkg._lib.fwd_form(d8, softcap=1.0) == "fa_fwd_generic_cap_kernel"
    assert pkg._lib.bwd_kernels(fa_desc(pkg, ql=4096, kl=4096), softcap=30.0) == ("fa_bwd_dkdv_kernel", "fa_bwd_dq_kernel")


def test_cap_zero_reports_what_ex_reports(pkg):
    lib = pkg._lib.load()
    L = pkg._lib
    for kw in (dict(ql=4096, kl=4096, qh=8, kh=8), dict(emb=128, ql=2048, kl=2048, causal=1), dict(emb=8), dict(dtype=L.NNOP_F32),
               dict(emb=32, ql=2048, kl=2048, qh=8, kh=8, batch=8, causal=1)):
        d = fa_desc(pkg, **kw)
        for opts in (None, fa_opts(pkg, 100, 0)):
            op = C.byref(opts) if opts is not None else None
            for pair, mask in ((0, 0), (1, 0), (0, 1)):
                assert lib.nnop_debug_fwd_form_cap(C.byref(d), op, C.c_float(0.0), pair, mask) == \
                    lib.nnop_debug_fwd_form_ex(C.byref(d), op, pair, mask)
                assert lib.nnop_debug_bwd_form_cap(C.byref(d), op, C.c_float(0.0), pair, mask) == \
                    lib.nnop_debug_bwd_form_ex(C.byref(d), op, pair, mask)
    assert lib.nnop_debug_fwd_form_cap(C.byref(fa_desc(pkg)), None, C.c_float(-1.0), 0, 0) == L.NNOP_ERR_OPTS
    assert lib.nnop_debug_bwd_form_cap(C.byref(fa_desc(pkg)), None, C.c_float(float("nan")), 0, 0) == L.NNOP_ERR_OPTS


# ---- the Julia shim ---------------------------------------------------------------------------------------------------------
def test_julia_shim_has_the_function_its_rule_and_both_calls():
    header = strip_c_comments(open(HEADER).read())
    shim = open(SHIM).read()
    called = set(re.findall(r"ccall\(\(:(nnop_[a-z_]+)", shim))
    assert {"nnop_fa_fwd_softcap", "nnop_fa_bwd_softcap"} <= called
    assert called <= set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header))
    sig = re.search(r"\nsoftcap_flash_attention\(q, k, v, pair = nothing;([^\n]*)\) =", shim)
    assert sig
    for kwarg in ("causal::Bool", "kpad_mask = nothing", "window = nothing", "sinks = nothing", "softcap"):
        assert kwarg in sig.group(1), kwarg
    assert re.search(r"NNop\.CRC\.rrule\(::typeof\(softcap_flash_attention\)", shim)
    assert re.search(r"export [^\n]*\bsoftcap_flash_attention\b", shim)


@pytest.mark.parametrize("name", ["nnop_fa_fwd_softcap", "nnop_fa_bwd_softcap"])
def test_julia_ccall_argument_tuples_match_the_prototypes(name):
    types = jl_ccall_types(open(SHIM).read(), name)
    params = c_params(strip_c_comments(open(HEADER).read()), name)
    assert len(types) == len(params)
    assert [i for i, t in enumerate(types) if t == "Cfloat"] == [i for i, p in enumerate(params) if p.startswith("float softcap")]


# ---- Python argument checks (before any GPU use: CPU tensors never reach the device check) ------------------------------------------
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -5])
def test_python_refuses_a_bad_cap_before_any_gpu_use(pkg, bad):
    q = torch.zeros(1, 2, 4, 8)
    for call in (lambda: pkg.flash_attention(q, q, q, causal=False, softcap=bad),
                 lambda: pkg._flash_attention(q, q, q, causal=False, softcap=bad),
                 lambda: pkg.grad_flash_attention(q, q, q[..., 0], q[..., 0], q, q, q, causal=False, softcap=bad)):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_OPTS


@pytest.mark.parametrize("bad", ["30", (1.0,), True, [50.0]])
def test_python_refuses_a_non_number(pkg, bad):
    q = torch.zeros(1, 2, 4, 8)
    with pytest.raises(TypeError):
        pkg.flash_attention(q, q, q, causal=False, softcap=bad)
    with pytest.raises(TypeError):
        pkg._flash_attention(q, q, q, causal=False, softcap=bad)


def test_python_takes_numpy_and_fraction_numbers(pkg):
    """a cap usually comes from a model config: any real number is one, numpy's scalar types included"""
    import fractions
    for c in (np.float32(30.0), np.float64(30.0), np.int64(30), 30, fractions.Fraction(30)):
        assert pkg._lib.fa_softcap(c) == 30.0 and type(pkg._lib.fa_softcap(c)) is float
    assert pkg._lib.fa_softcap(np.float32(0.0)) == 0.0
    with pytest.raises(TypeError):
        pkg._lib.fa_softcap(np.bool_(True))
    with pytest.raises(pkg.NNopError):
        pkg.flash_attention(torch.zeros(1, 2, 4, 8), torch.zeros(1, 2, 4, 8), torch.zeros(1, 2, 4, 8), causal=False, softcap=np.float32(-1.0))


def test_python_none_and_zero_take_the_call_without_a_cap(pkg, monkeypatch):
    """None / 0 / 0.0 must not reach the softcap entry points: they issue exactly the previous call"""
    att = __import__(pkg.__name__ + ".attention", fromlist=["x"])
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                seen.append(name)
                return 0
            return f
    d = pkg._lib.FaDesc()
    for cap in (None, 0, 0.0):
        c = att._softcap(cap)
        att._fwd_call(Lib(), None, d, softcap=c)
        att._bwd_call(Lib(), None, d, softcap=c)
        att._fwd_call(Lib(), None, d, sinks=None, softcap=c)
    assert set(seen) == {"nnop_fa_fwd", "nnop_fa_bwd"}
    seen.clear()
    att._fwd_call(Lib(), None, d, softcap=att._softcap(30))
    att._bwd_call(Lib(), None, d, softcap=att._softcap(30.0))
    assert seen == ["nnop_fa_fwd_softcap", "nnop_fa_bwd_softcap"]


def test_shard_helpers_pass_the_cap_through(pkg):
    import inspect
    from importlib import import_module
    shard = import_module(pkg.__name__ + ".shard")
    for fn in (shard.flash_attention_sharded, shard.flash_attention_sharded_fwd_bwd):
        assert "softcap" in inspect.signature(fn).parameters
    got = {}

    def attn(q, k, v, p, **kw):
        got.update(kw)
        return q
    q = torch.zeros(2, 2, 3, 4)
    shard.flash_attention_sharded(q, q, q, causal=False, world=1, rank=0, attn_fn=attn, softcap=30.0)
    assert got["softcap"] == 30.0 and "window" not in got
