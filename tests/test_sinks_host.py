"""CPU tests of learned attention sinks: the sink reference against a literal torch implementation of gpt-oss's formula (cat,
softmax, drop), the validation codes of nnop_fa_fwd_sinks / nnop_fa_bwd_sinks, and the Julia shim's declarations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from abi_util import HEADER, SHIM, c_param_count, fa_desc, fa_opts, jl_ccall_types, strip_c_comments
from attn_ref import attention_fwd, attention_grads, window_keep


# ---- the reference against the literal formula --------------------------------------------------------------------------------
def _gptoss(q, k, v, sinks, pair, causal, kpad_mask, window):
    """torch fp64: logits (+pair, masked), concatenate sigma_h, softmax, drop the sink column, P V."""
    B, QH, QL, E = q.shape
    KH, KL = k.shape[1], k.shape[2]
    ke, ve = k.repeat_interleave(QH // KH, dim=1), v.repeat_interleave(QH // KH, dim=1)
    s = q @ ke.transpose(-1, -2) / np.sqrt(E)
    if pair is not None:
        s = s + pair.permute(0, 3, 2, 1)
    vis = torch.from_numpy(window_keep(QL, KL, window, causal))[None, None]
    if kpad_mask is not None:
        vis = vis & torch.from_numpy(kpad_mask)[:, None, None, :]
    s = s.masked_fill(~vis, float("-inf"))
    col = sinks[None, :, None, None].expand(B, QH, QL, 1)
    p = torch.softmax(torch.cat([s, col], dim=-1), dim=-1)[..., :KL]
    return p @ ve


CASES = [
    # B, QH, KH, QL, KL, E, causal, window, pad, pair, sinks
    (2, 4, 2, 9, 11, 8, False, None, False, False, [0.0, 3.0, -30.0, 30.0]),
    (1, 4, 1, 12, 12, 4, True, (3, 0), True, False, [0.5, -1.0, 2.0, 0.0]),       # GQA, window + causal + kpad
    (2, 2, 2, 7, 10, 8, False, (2, 1), False, True, [1.0, -2.0]),                 # pair bias
    (1, 3, 3, 6, 6, 4, True, None, False, False, [float("-inf"), 0.0, 30.0]),    # sigma = -inf: the plain softmax
]


@pytest.mark.parametrize("case", CASES)
def test_reference_matches_the_gptoss_formula(case):
    B, QH, KH, QL, KL, E, causal, window, pad, has_pair, sk = case
    rng = np.random.default_rng(len(repr(case)))
    q, k, v, do = (rng.standard_normal(s) for s in ((B, QH, QL, E), (B, KH, KL, E), (B, KH, KL, E), (B, QH, QL, E)))
    pair = rng.standard_normal((B, KL, QL, QH)) if has_pair else None
    mask = None
    if pad:
        mask = np.ones((B, KL), bool)
        mask[:, -3:] = False
    sinks = np.array(sk)
    o, ms, ls = attention_fwd(q, k, v, pair, causal=causal, kpad_mask=mask, window=window, sinks=sinks)
    dq, dk, dv, dp, ds = attention_grads(q, k, v, do, pair, causal=causal, kpad_mask=mask, window=window, sinks=sinks)

    t = lambda x: torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tq, tk, tv, ts = t(q), t(k), t(v), t(sinks)
    tp = t(pair) if pair is not None else None
    to = _gptoss(tq, tk, tv, ts, tp, causal, mask, window)
    to.backward(torch.tensor(do))
    np.testing.assert_allclose(o, to.detach().numpy(), rtol=1e-10, atol=1e-12)
    # ms, ls: the row max over the visible logits and sigma, the sum relative to it (sink included)
    s = np.einsum("bhie,bhje->bhij", q, np.repeat(k, QH // KH, axis=1)) / np.sqrt(E)
    if pair is not None:
        s = s + pair.transpose(0, 3, 2, 1)
    vis = np.broadcast_to(window_keep(QL, KL, window, causal)[None, None], s.shape)
    if mask is not None:
        vis = vis & mask[:, None, None, :]
    s = np.where(vis, s, -np.inf)
    full = np.concatenate([s, np.broadcast_to(sinks[None, :, None, None], (B, QH, QL, 1))], axis=-1)
    m_ref = full.max(axis=-1)
    np.testing.assert_allclose(ms, m_ref)
    np.testing.assert_allclose(ls, np.exp(full - m_ref[..., None]).sum(axis=-1), rtol=1e-12)
    for got, ref in ((dq, tq), (dk, tk), (dv, tv), (ds, ts)):
        np.testing.assert_allclose(got, ref.grad.numpy(), rtol=1e-9, atol=1e-11)
    if pair is not None:
        np.testing.assert_allclose(dp, tp.grad.numpy(), rtol=1e-9, atol=1e-11)
    if np.isneginf(sinks).any():
        assert (ds[np.isneginf(sinks)] == 0).all()


def test_dsinks_is_minus_p_sink_times_delta():
    """dsigma_h = -sum_{b,i} exp(sigma_h - ms) / ls * (dO . o): the formula the library's reduction evaluates"""
    rng = np.random.default_rng(5)
    B, QH, KH, QL, KL, E = 2, 4, 2, 10, 13, 8
    q, k, v, do = (rng.standard_normal(s) for s in ((B, QH, QL, E), (B, KH, KL, E), (B, KH, KL, E), (B, QH, QL, E)))
    sinks = np.array([0.3, -1.0, 2.5, 30.0])
    o, ms, ls = attention_fwd(q, k, v, causal=True, sinks=sinks)
    ds = attention_grads(q, k, v, do, causal=True, sinks=sinks)[4]
    want = -(np.exp(sinks[None, :, None] - ms) / ls * (do * o).sum(-1)).sum(axis=(0, 2))
    np.testing.assert_allclose(ds, want, rtol=1e-10)


def test_row_without_keys_sees_only_the_sink():
    """a row that sees no key but a finite sink: o = 0, ms = sigma, ls = 1, and it adds nothing to dq or dsigma"""
    rng = np.random.default_rng(1)
    q, k, v, do = (rng.standard_normal((1, 2, 6, 4)) for _ in range(4))
    mask = np.zeros((1, 6), bool)
    mask[0, 4:] = True                                   # with window (1, 0) rows 0..2 see nothing
    sinks = np.array([0.7, -3.0])
    o, ms, ls = attention_fwd(q, k, v, causal=True, kpad_mask=mask, window=(1, 0), sinks=sinks)
    dq, _, _, _, _ = attention_grads(q, k, v, do, causal=True, kpad_mask=mask, window=(1, 0), sinks=sinks)
    assert (o[:, :, :3] == 0).all() and (dq[:, :, :3] == 0).all()
    np.testing.assert_array_equal(ms[:, :, :3], np.broadcast_to(sinks[None, :, None], (1, 2, 3)))
    np.testing.assert_array_equal(ls[:, :, :3], 1.0)


# ---- C ABI validation (NULL tensors: the checks run before any pointer is used) ------------------------------------------------
def _fwd(lib, d, opts, sinks, tensors=None):
    t = C.c_void_p(tensors) if tensors else C.c_void_p(0)
    op = C.byref(opts) if opts is not None else None
    return lib.nnop_fa_fwd_sinks(C.byref(d), op, C.c_void_p(sinks), t, t, t, t, t, t, None, None, None)


def _bwd(lib, d, opts, sinks, dsinks, tensors=None):
    # (a huge workspace size: the size check comes before the alignment check)
    t = C.c_void_p(tensors) if tensors else C.c_void_p(0)
    op = C.byref(opts) if opts is not None else None
    return lib.nnop_fa_bwd_sinks(C.byref(d), op, C.c_void_p(sinks), C.c_void_p(dsinks), t, t, t, None, t, t, t, t, t, t, t,
                                 None, None, t, C.c_size_t(1 << 40), None)


def _sinks_calls(lib, d, opts, sinks, dsinks):
    """(fwd status, bwd status) of the two new entry points with NULL tensors"""
    return _fwd(lib, d, opts, sinks), _bwd(lib, d, opts, sinks, dsinks)


def test_sinks_null_is_the_ex_call(pkg):
    lib = pkg._lib.load()
    null = C.c_void_p(0)
    for d, opts in ((fa_desc(pkg), None), (fa_desc(pkg), fa_opts(pkg, 3, 0)), (fa_desc(pkg, emb_k=32), None),
                    (fa_desc(pkg), fa_opts(pkg, reserved=[1]))):
        op = C.byref(opts) if opts is not None else None
        ex_f = lib.nnop_fa_fwd_ex(C.byref(d), op, null, null, null, null, null, null, null, null, null)
        ex_b = lib.nnop_fa_bwd_ex(C.byref(d), op, *([null] * 13), null, 0, null)
        assert _sinks_calls(lib, d, opts, None, None) == (ex_f, ex_b)
        assert _sinks_calls(lib, d, opts, None, 0x1003) == (ex_f, ex_b)          # dsinks ignored without sinks


@pytest.mark.parametrize("kw,status", [
    (dict(emb_k=32), "NNOP_ERR_EMB_MISMATCH"),
    (dict(qh=6, kh=4), "NNOP_ERR_HEADS"),
    (dict(dtype=7), "NNOP_ERR_DTYPE"),
    (dict(ql=0), "NNOP_ERR_SHAPE"),
])
def test_bad_descriptor_reports_its_own_code_first(pkg, kw, status):
    lib = pkg._lib.load()
    st = _sinks_calls(lib, fa_desc(pkg, **kw), fa_opts(pkg, reserved=[1]), 0x1001, None)
    assert st == (getattr(pkg._lib, status),) * 2


def test_reserved_options_are_rejected(pkg):
    lib = pkg._lib.load()
    assert _sinks_calls(lib, fa_desc(pkg), fa_opts(pkg, reserved=[0, 2]), 0x1001, None) == (pkg._lib.NNOP_ERR_OPTS,) * 2
    assert _sinks_calls(lib, fa_desc(pkg), fa_opts(pkg, left=-3), 0x1000, 0x2000) == (pkg._lib.NNOP_ERR_OPTS,) * 2


def test_null_pointers_then_alignment(pkg):
    """every call here fails a check before any launch: the fake (never dereferenced) tensor addresses stay on the host"""
    lib = pkg._lib.load()
    d = fa_desc(pkg)
    E = pkg._lib
    # NULL tensors: NNOP_ERR_NULL whatever the sinks are (the NULL check comes before the alignment check)
    assert _sinks_calls(lib, d, None, 0x1001, 0x2001) == (E.NNOP_ERR_NULL, E.NNOP_ERR_NULL)
    fake = 0x10000                                        # 16-byte aligned
    assert _bwd(lib, d, None, 0x1000, None, fake) == E.NNOP_ERR_NULL       # sinks without dsinks
    assert _bwd(lib, d, None, 0x1001, None, fake) == E.NNOP_ERR_NULL       # ... before the alignment of sinks
    assert _fwd(lib, d, None, 0x1002, fake) == E.NNOP_ERR_ALIGN
    assert _bwd(lib, d, None, 0x1002, 0x2000, fake) == E.NNOP_ERR_ALIGN
    assert _bwd(lib, d, None, 0x1000, 0x2001, fake) == E.NNOP_ERR_ALIGN
    assert _fwd(lib, d, None, 0x1002) == E.NNOP_ERR_NULL                   # NULL before alignment in the forward too


def test_workspace_size_is_unchanged_by_construction(pkg):
    """the sink adds no parameter to the workspace queries: the size is the size without sinks, and covers the dsinks partials"""
    lib = pkg._lib.load()
    for kw in (dict(), dict(dtype=pkg._lib.NNOP_F32, emb=8, ql=5, kl=7), dict(ql=4097, qh=64, kh=8)):
        d = fa_desc(pkg, **kw)
        n = lib.nnop_fa_bwd_workspace_bytes(C.byref(d))
        rows = d.batch * d.qh * ((d.ql + 63) // 64 * 64)
        assert n >= 2 * 4 * rows >= 4 * d.batch * d.qh * d.ql
    header = open(HEADER).read()
    assert re.search(r"size_t nnop_fa_bwd_workspace_bytes\(const nnop_fa_desc\* d\);", header)


def test_symbols_are_exported_and_abi_stays_7(pkg):
    assert "nnop_fa_fwd_sinks" in pkg._lib.EXPORTED_SYMBOLS and "nnop_fa_bwd_sinks" in pkg._lib.EXPORTED_SYMBOLS
    lib = pkg._lib.load()
    assert lib.nnop_abi_version() == 7 == pkg._lib.ABI_VERSION


# ---- the Julia shim ---------------------------------------------------------------------------------------------------------
def test_julia_shim_calls_only_declared_symbols():
    header = strip_c_comments(open(HEADER).read())
    declared = set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header))
    shim = open(SHIM).read()
    called = set(re.findall(r"ccall\(\(:(nnop_[a-z_]+)", shim))
    assert {"nnop_fa_fwd_sinks", "nnop_fa_bwd_sinks"} <= called
    assert called <= declared, called - declared
    assert re.search(r"function flash_attention_sinks_fwd\(.*?sinks::ROCVector\{Float32\}", shim, re.S)
    assert re.search(r"NNop\.CRC\.rrule\(::typeof\(flash_attention_sinks\)", shim)


@pytest.mark.parametrize("name", ["nnop_fa_fwd_sinks", "nnop_fa_bwd_sinks"])
def test_julia_ccall_argument_tuples_match_the_prototypes(name):
    header = strip_c_comments(open(HEADER).read())
    shim = open(SHIM).read()
    assert len(jl_ccall_types(shim, name)) == c_param_count(header, name)
