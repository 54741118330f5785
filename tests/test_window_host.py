"""CPU tests of the sliding-window boundary (ABI version 7): option validation of nnop_fa_fwd_ex / nnop_fa_bwd_ex, the kernel forms a
window selects (no device needed), the window reference against an explicit loop, and the Julia shim's declarations."""
import ctypes as C
import re

import numpy as np
import pytest

from abi_util import HEADER, SHIM, fa_desc, fa_opts, strip_c_comments
from attn_ref import attention_fwd, attention_grads, window_bias, window_keep


def _both(lib, d, opts):
    null = C.c_void_p(0)
    op = C.byref(opts) if opts is not None else None
    st_f = lib.nnop_fa_fwd_ex(C.byref(d), op, null, null, null, null, null, null, null, null, null)
    st_b = lib.nnop_fa_bwd_ex(C.byref(d), op, *([null] * 13), null, 0, null)
    return st_f, st_b


@pytest.mark.parametrize("opts_kw,status", [
    (dict(reserved=[0, 0, 0, 1]), "NNOP_ERR_OPTS"),
    (dict(reserved=[7]), "NNOP_ERR_OPTS"),
    (dict(left=-2), "NNOP_ERR_OPTS"),
    (dict(right=-5), "NNOP_ERR_OPTS"),
    (dict(left=3, right=0), "NNOP_ERR_NULL"),            # valid options, NULL tensors
])
def test_option_validation_codes(pkg, opts_kw, status):
    lib = pkg._lib.load()
    st_f, st_b = _both(lib, fa_desc(pkg), fa_opts(pkg, **opts_kw))
    assert st_f == st_b == getattr(pkg._lib, status)


def test_opts_null_is_the_call_without_options(pkg):
    lib = pkg._lib.load()
    assert _both(lib, fa_desc(pkg), None) == (pkg._lib.NNOP_ERR_NULL, pkg._lib.NNOP_ERR_NULL)


@pytest.mark.parametrize("kw,status", [
    (dict(emb_k=32), "NNOP_ERR_EMB_MISMATCH"),
    (dict(qh=6, kh=4), "NNOP_ERR_HEADS"),
    (dict(dtype=7), "NNOP_ERR_DTYPE"),
    (dict(ql=0), "NNOP_ERR_SHAPE"),
])
def test_bad_descriptor_reports_its_own_code_before_the_options(pkg, kw, status):
    lib = pkg._lib.load()
    st_f, st_b = _both(lib, fa_desc(pkg, **kw), fa_opts(pkg, left=-2, reserved=[1]))
    assert st_f == st_b == getattr(pkg._lib, status)


def test_strerror_names_the_options(pkg):
    assert "option" in pkg._lib.strerror(pkg._lib.NNOP_ERR_OPTS).lower()
    assert pkg._lib.ABI_VERSION == 7


# C2 (bf16 E64 L4096 H4 B4 non-causal: duo forward) and C3 (bf16 causal E128 L8192 H32 B8: w64 backward) and a few others that
# take the duo / w64 / split forms today
FORM_SHAPES = [
    dict(dtype=2, emb=64, ql=4096, kl=4096, qh=4, kh=4, batch=4, causal=0),
    dict(dtype=2, emb=128, ql=8192, kl=8192, qh=32, kh=32, batch=8, causal=1),
    dict(dtype=1, emb=32, ql=2048, kl=2048, qh=8, kh=8, batch=8, causal=1),
    dict(dtype=2, emb=16, ql=1024, kl=1024, qh=8, kh=8, batch=4, causal=0),
    dict(dtype=0, emb=64, ql=4096, kl=4096, qh=4, kh=4, batch=4, causal=1),
    dict(dtype=2, emb=256, ql=2048, kl=2048, qh=8, kh=8, batch=2, causal=0),
    dict(dtype=2, emb=8, ql=512, kl=512, qh=2, kh=2, batch=1, causal=0),
]


@pytest.mark.parametrize("shape", FORM_SHAPES, ids=lambda s: "dt{dtype}-E{emb}-L{ql}-H{qh}-B{batch}-c{causal}".format(**s))
@pytest.mark.parametrize("window", [(1023, 0), (0, 0), (-1, 17), (64, -1)])
def test_windowed_problem_runs_the_32_row_or_plain_kernels(pkg, shape, window):
    d = pkg._lib.FaDesc(**shape)
    if shape["causal"] and window[0] < 0:
        window = (100, window[1])                                          # (-1, r) normalises away under causal
    for has_mask in (False, True):
        form = pkg._lib.fwd_form(d, has_mask=has_mask, window=window)
        assert form == ("fa_fwd_generic_kernel" if shape["emb"] == 8 else "fa_fwd_kernel")
        for has_pair in (False, True):
            assert pkg._lib.bwd_kernels(d, has_pair=has_pair, has_mask=has_mask, window=window) == \
                ("fa_bwd_dkdv_kernel", "fa_bwd_dq_kernel")


def test_the_shapes_above_do_use_the_other_forms_without_a_window(pkg):
    """(so the test above shows the window's rule, not the shapes')"""
    c2, c3 = (pkg._lib.FaDesc(**s) for s in FORM_SHAPES[:2])
    assert pkg._lib.fwd_form(c2) == "fa_fwd_duo_kernel"
    assert pkg._lib.bwd_kernels(c3) == ("fa_bwd_w64_kernel<dK/dV>", "fa_bwd_w64_kernel<dQ>")


@pytest.mark.parametrize("shape", FORM_SHAPES, ids=lambda s: "dt{dtype}-E{emb}-L{ql}-H{qh}-B{batch}-c{causal}".format(**s))
def test_a_window_that_normalises_away_reports_the_unwindowed_form(pkg, shape):
    d = pkg._lib.FaDesc(**shape)
    QL, KL = shape["ql"], shape["kl"]
    windows = [(-1, -1), (QL - 1, -1), (-1, KL - 1), (QL + 5, KL + 100)]
    if shape["causal"]:
        windows += [(-1, 0), (QL - 1, 3), (-1, 5000)]
    for w in windows:
        for has_pair in (False, True):
            for has_mask in (False, True):
                assert pkg._lib.fwd_form(d, has_pair, has_mask, window=w) == pkg._lib.fwd_form(d, has_pair, has_mask), w
                assert pkg._lib.bwd_kernels(d, has_pair, has_mask, window=w) == pkg._lib.bwd_kernels(d, has_pair, has_mask), w


def test_form_hooks_validate_options(pkg):
    d = fa_desc(pkg)
    with pytest.raises(ValueError):
        pkg._lib.fwd_form(d, window=(-2, 0))
    with pytest.raises(TypeError):
        pkg._lib.fwd_form(d, window=(1.5, 0))


# ---- the window reference against an explicit loop ---------------------------------------------------------------------------
def _loop_attention(q, k, v, dO, window, causal, kpad):
    """fp64, one (batch, head, query) at a time, inclusive window bounds, top-left alignment; rows that see no key: o = NaN,
    dq = 0 and no contribution (the library's convention)."""
    B, QH, QL, E = q.shape
    KH, KL = k.shape[1], k.shape[2]
    rep = QH // KH
    left, right = window
    o = np.full(q.shape, np.nan)
    dq, dk, dv = np.zeros(q.shape), np.zeros(k.shape), np.zeros(v.shape)
    for b in range(B):
        for h in range(QH):
            g = h // rep
            for i in range(QL):
                js = [j for j in range(KL)
                      if (left < 0 or j >= i - left) and (right < 0 or j <= i + right) and (not causal or j <= i) and kpad[b, j]]
                if not js:
                    continue
                s = np.array([q[b, h, i] @ k[b, g, j] for j in js]) / np.sqrt(E)
                p = np.exp(s - s.max())
                p /= p.sum()
                o[b, h, i] = sum(pj * v[b, g, j] for pj, j in zip(p, js))
                dp = np.array([dO[b, h, i] @ v[b, g, j] for j in js])
                ds = p * (dp - dO[b, h, i] @ o[b, h, i])
                for pj, dsj, j in zip(p, ds, js):
                    dq[b, h, i] += dsj * k[b, g, j] / np.sqrt(E)
                    dk[b, g, j] += dsj * q[b, h, i] / np.sqrt(E)
                    dv[b, g, j] += pj * dO[b, h, i]
    return o, dq, dk, dv


@pytest.mark.parametrize("QL,KL", [(7, 11), (11, 7), (9, 9), (12, 3)])
@pytest.mark.parametrize("window", [(0, 0), (1, 0), (2, 3), (-1, 1), (3, -1), (0, -1)])
@pytest.mark.parametrize("causal", [False, True])
def test_window_reference_matches_an_explicit_loop(QL, KL, window, causal):
    rng = np.random.default_rng(QL * 100 + KL + 7 * window[0] + window[1] + 1000 * causal)
    B, QH, KH, E = 2, 4, 2, 8
    q, k, v = rng.standard_normal((B, QH, QL, E)), rng.standard_normal((B, KH, KL, E)), rng.standard_normal((B, KH, KL, E))
    dO = rng.standard_normal((B, QH, QL, E))
    kpad = np.ones((B, KL), bool)
    kpad[1, -2:] = False
    o_l, dq_l, dk_l, dv_l = _loop_attention(q, k, v, dO, window, causal, kpad)
    o, ms, ls = attention_fwd(q, k, v, causal=causal, kpad_mask=kpad, window=window)
    dq, dk, dv, dp = attention_grads(q, k, v, dO, causal=causal, kpad_mask=kpad, window=window)
    assert dp is None
    assert (np.isnan(o) == np.isnan(o_l)).all()
    np.testing.assert_allclose(np.nan_to_num(o), np.nan_to_num(o_l), rtol=1e-12, atol=1e-12)
    for a, b in ((dq, dq_l), (dk, dk_l), (dv, dv_l)):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12)
    # the cases cover rows without a visible key where the shape makes them
    if QL > KL and window[0] >= 0 and window[0] < QL - KL:
        assert np.isnan(o).any()


def test_window_bias_layout():
    b = window_bias(2, 5, 6, 3, (1, 2))
    assert b.shape == (2, 6, 5, 3)
    keep = window_keep(5, 6, (1, 2))
    assert keep[3].tolist() == [False, False, True, True, True, True]
    assert (b[:, :, 3, :] == 0).sum() == 2 * 4 * 3 and np.isneginf(b[1, 0, 3, 2])


def test_pair_bias_gradient_is_zero_outside_the_window():
    rng = np.random.default_rng(5)
    q, k, v = rng.standard_normal((1, 2, 9, 8)), rng.standard_normal((1, 2, 9, 8)), rng.standard_normal((1, 2, 9, 8))
    pair, dO = rng.standard_normal((1, 9, 9, 2)), rng.standard_normal((1, 2, 9, 8))
    dq, dk, dv, dp = attention_grads(q, k, v, dO, pair, causal=False, window=(1, 1))
    outside = ~window_keep(9, 9, (1, 1)).T                   # [KL, QL]
    assert (dp[0][outside] == 0).all() and (dp[0][~outside] != 0).any()


# ---- the Julia shim ---------------------------------------------------------------------------------------------------------
def test_julia_shim_calls_only_declared_symbols():
    header = strip_c_comments(open(HEADER).read())
    declared = set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header))
    shim = open(SHIM).read()
    called = set(re.findall(r"ccall\(\(:(nnop_[a-z_]+)", shim))
    assert {"nnop_fa_fwd_ex", "nnop_fa_bwd_ex"} <= called
    assert called <= declared, called - declared
    assert re.search(r"nnop_abi_version.*?\)\s*(==|!=|<)\s*7", shim, re.S) or re.search(r"ABI_VERSION\s*=\s*7", shim)


def test_julia_faopts_matches_the_c_struct():
    header = strip_c_comments(open(HEADER).read())
    body = re.search(r"typedef struct nnop_fa_opts \{(.*?)\} nnop_fa_opts;", header, re.S).group(1)
    c_fields = re.findall(r"(int32_t)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [(n, int(a or 1)) for _, n, a in c_fields] == [("window_left", 1), ("window_right", 1), ("reserved", 6)]
    shim = open(SHIM).read()
    jl = re.search(r"struct FaOpts\b(.*?)\bend\b", shim, re.S).group(1)
    j_fields = re.findall(r"(\w+)::(\w+(?:\{[^}]*\})?)", jl)
    assert j_fields == [("window_left", "Int32"), ("window_right", "Int32"), ("reserved", "NTuple{6, Int32}")]


def test_python_normalises_windows_like_the_library(pkg):
    """a window that removes no key becomes NO options on the host, so that e.g. the pair-bias backward gets the staged workspace
    of the call without a window"""
    d = fa_desc(pkg, ql=100, kl=80, causal=0)
    for w in [(-1, -1), (99, -1), (-1, 79), (500, 500)]:
        assert pkg._lib.fa_opts(w, d) is None, w
    for w in [(98, -1), (-1, 78), (0, 0), (-2, -1)]:
        assert pkg._lib.fa_opts(w, d) is not None, w
    dc = fa_desc(pkg, ql=100, kl=80, causal=1)
    assert pkg._lib.fa_opts((-1, 0), dc) is None and pkg._lib.fa_opts((99, 7), dc) is None
    assert pkg._lib.fa_opts((98, 7), dc) is not None
