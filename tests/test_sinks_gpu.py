"""Learned attention sinks on the GPU: parity with the fp64 oracle through tests/attn_ref.py on every forward form and backward
path, the properties of include/nnop_hip.h (rows without keys, large sigma, sigma = -inf), a dsinks that is bitwise the same
whichever backward kernels ran, autograd, and a gpt-oss-like layer at full size."""
import numpy as np
import pytest
import torch

from attn_ref import INF, attention_fwd, check_parity, inputs, run
from util import TORCH_DT, assert_close, to64

pytestmark = pytest.mark.gpu


# ---- parity grid: dtype x E x causal x ragged lengths x kpad x window x pair x GQA, pruned ------------------------------------
def _grid():
    out = []
    lens = [(63, 65), (200, 200), (130, 97)]
    i = 0
    for E in (16, 32, 64, 128, 256, 8):
        for dt in ("f32", "bf16", "f16"):
            causal = i % 2 == 0
            QL, KL = lens[i % 3]
            pad = i % 3 == 1
            window = [None, (20, 0), (31, 7)][(i // 2) % 3]
            pair = i % 4 == 3 and E <= 128
            gqa = i % 5 != 4
            out.append((dt, E, causal, QL, KL, pad, window, pair, gqa))
            i += 1
    return out


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "{}-E{}-c{}-L{}x{}-pad{}-w{}-pair{}-gqa{}".format(*c))
def test_sinks_parity(pkg, dev, case):
    dt, E, causal, QL, KL, pad, window, pair, gqa = case
    QH, KH = (5, 5) if not gqa else (6, 2)
    if pair:
        QH, KH = 5, 5
    d = inputs(case, 2, QH, KH, QL, KL, E, dt, dev, pair=pair, pad=pad, sinks="mix")
    check_parity(pkg, d, dt, causal, window=window, sinks=d["sinks"])


# ---- every forward form on purpose, pinned -----------------------------------------------------------------------------------
def _desc(pkg, d, causal):
    from importlib import import_module
    return import_module(pkg.__name__ + ".attention")._desc(d["q"], d["k"], d["v"], causal)


FORMS = [
    # id, knobs, dtype, E, QL, KL, QH, KH, B, causal, window, pad, expected form
    ("duo-nz2", dict(fwd_duo=2), "bf16", 64, 1024, 1024, 4, 2, 2, False, None, False, "fa_fwd_duo_kernel"),
    ("duo-nz1", dict(fwd_duo=3), "bf16", 64, 1024, 1024, 4, 2, 1, True, None, False, "fa_fwd_duo_kernel"),
    ("duo-e32", dict(fwd_duo=1), "f16", 32, 1024, 1100, 4, 4, 1, False, None, True, "fa_fwd_duo_kernel"),
    ("duo-e128", dict(fwd_duo=1), "bf16", 128, 600, 700, 2, 2, 1, True, None, False, "fa_fwd_duo_kernel"),
    ("w64", dict(fwd_duo=0, fwd_w64=1), "bf16", 64, 600, 512, 4, 2, 1, False, None, False, "fa_fwd_w64_kernel"),
    ("w64-masked", dict(fwd_duo=0, fwd_w64=1, fwd_persist=0), "f16", 128, 600, 700, 2, 1, 2, True, None, True, "fa_fwd_w64_kernel"),
    ("w64-folded", dict(fwd_duo=0, fwd_w64=1, fwd_exact_scale=0), "bf16", 64, 512, 512, 2, 2, 1, True, None, False,
     "fa_fwd_w64_kernel"),
    ("w64-e256", dict(fwd_w64=1), "bf16", 256, 300, 256, 2, 2, 1, False, None, False, "fa_fwd_w64_kernel"),
    ("split", dict(fwd_duo=0, fwd_w64=0, fwd_split=1), "bf16", 64, 512, 512, 2, 2, 2, False, None, False, "fa_fwd_split_kernel"),
    ("row32", dict(fwd_duo=0, fwd_w64=0, fwd_split=0), "bf16", 64, 512, 512, 2, 2, 1, False, None, False, "fa_fwd_kernel"),
    ("row32-win", dict(), "f16", 64, 500, 500, 4, 2, 1, True, (127, 0), False, "fa_fwd_kernel"),
    ("row32-f32", dict(), "f32", 128, 300, 333, 2, 1, 1, True, None, True, "fa_fwd_kernel"),
    ("generic", dict(), "bf16", 8, 300, 270, 4, 2, 1, True, None, False, "fa_fwd_generic_kernel"),
]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_every_forward_form(pkg, dev, tune, form):
    name, knobs, dt, E, QL, KL, QH, KH, B, causal, window, pad, want = form
    tune(**knobs)
    d = inputs(form[0], B, QH, KH, QL, KL, E, dt, dev, pad=pad, sinks="mix")
    assert pkg._lib.fwd_form(_desc(pkg, d, causal), has_mask=pad, window=window) == want
    check_parity(pkg, d, dt, causal, window=window, sinks=d["sinks"])


def test_persistent_forward_is_the_one_block_result(pkg, dev, tune):
    """the persistent block-list form (w64 and duo, causal) against the one-block-per-workgroup form: the same rows, bitwise"""
    d = inputs("persist", 2, 8, 2, 8192, 8192, 64, "bf16", dev, sinks="mix")
    for knobs in (dict(fwd_duo=0, fwd_w64=1), dict(fwd_duo=1)):
        outs = []
        for persist in (0, 1):
            tune(fwd_persist=persist, **knobs)
            outs.append(pkg._flash_attention(d["q"], d["k"], d["v"], causal=True, sinks=d["sinks"]))
        for a, b in zip(*outs):
            assert torch.equal(a.nan_to_num(), b.nan_to_num())


# ---- every backward path; dsinks bitwise the same everywhere ---------------------------------------------------------------
W64_BWD = ("fa_bwd_w64_kernel<dK/dV>", "fa_bwd_w64_kernel<dQ>")
TILED_BWD = ("fa_bwd_dkdv_kernel", "fa_bwd_dq_kernel")
BWD = [
    # id, knobs, the (dK/dV, dQ) kernels the launcher reports for them (narrow and persistent are shapes of the w64 kernels)
    ("w64-fused", dict(), W64_BWD),
    ("w64-pre", dict(bwd_w64=4), W64_BWD),
    ("narrow", dict(bwd_narrow=1), W64_BWD),
    ("persist", dict(bwd_persist=1), W64_BWD),
    ("tiled", dict(bwd_w64=0), TILED_BWD),
]


@pytest.mark.parametrize("form", BWD, ids=lambda f: f[0])
def test_every_backward_path(pkg, dev, tune, form):
    """each backward path, pinned, against the reference; dsinks is the same bits whichever path ran (it reads dO, o, ms, ls only)"""
    name, knobs, want = form
    d = inputs("bwd", 2, 8, 2, 700, 700, 64, "bf16", dev, sinks="mix")
    ref = run(pkg, d, True, sinks=d["sinks"])                      # the default path
    tune(**knobs)
    assert pkg._lib.bwd_kernels(_desc(pkg, d, True)) == want
    got = check_parity(pkg, d, "bf16", True, sinks=d["sinks"])
    assert torch.equal(got[7], ref[7])


def test_generic_backward(pkg, dev):
    """E = 8: the plain-HIP backward kernels (fa_generic.hpp; every embedding dim outside the tiled set)"""
    d = inputs("bwd-generic", 2, 4, 2, 300, 280, 8, "f16", dev, pad=True, sinks="mix")
    assert pkg._lib.fwd_form(_desc(pkg, d, True), has_mask=True) == "fa_fwd_generic_kernel"
    check_parity(pkg, d, "f16", True, window=(50, 0), sinks=d["sinks"])


@pytest.mark.parametrize("dt,E", [("bf16", 64), ("f32", 32), ("f16", 128)])
def test_pair_bias_staged_and_direct(pkg, dev, dt, E):
    from importlib import import_module
    att = import_module(pkg.__name__ + ".attention")
    d = inputs(("pair", dt, E), 1, 4, 4, 200, 150, E, dt, dev, pair=True, sinks="mix")
    o, ms, ls, *ref = check_parity(pkg, d, dt, False, sinks=d["sinks"])       # grad_flash_attention: the staged path
    q, k, v = d["q"], d["k"], d["v"]
    small = att.bwd_workspace_bytes(q, k, v, causal=False)
    ws = torch.empty(small, dtype=torch.uint8, device=dev)
    dq, dk, dv, dp = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(d["pair"])
    ds = torch.empty(4, dtype=torch.float32, device=dev)
    att.fa_bwd_into(dq, dk, dv, dp, ws, d["do"], o, ms, ls, q, k, v, d["pair"], causal=False, sinks=d["sinks"], dsinks=ds)
    torch.cuda.synchronize()
    assert torch.equal(ds, ref[4])
    for a, b in zip((dq, dk, dv, dp), ref[:4]):
        assert_close("direct pair", a, to64(b), dt, 2.0, floor=True, kind="grad")


# ---- properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,E", [("bf16", 64), ("f32", 16), ("f16", 8)])
def test_rows_without_keys_see_only_the_sink(pkg, dev, dt, E):
    d = inputs(("dead", dt), 1, 2, 2, 256, 256, E, dt, dev, sinks=[0.5, -2.0])
    mask = torch.zeros(1, 256, dtype=torch.bool, device=dev)
    mask[0, 200:] = True                               # causal + window (10, 0): rows < 200 see nothing
    d["mask"] = mask
    o, ms, ls, dq, *_rest = check_parity(pkg, d, dt, True, window=(10, 0), sinks=d["sinks"])
    assert (o[:, :, :200] == 0).all() and (dq[:, :, :200] == 0).all()
    assert torch.isfinite(ms).all() and torch.isfinite(ls).all()


@pytest.mark.parametrize("dt,E", [("bf16", 64), ("f16", 128), ("f32", 32), ("bf16", 8)])
def test_large_sink_does_not_overflow(pkg, dev, dt, E):
    d = inputs(("big", dt, E), 1, 2, 1, 300, 300, E, dt, dev, sinks=[200.0, 200.0])
    d["q"] = d["q"] * 0.01
    o, ms, ls, *g = run(pkg, d, False, sinks=d["sinks"])
    for t in (o, ms, ls) + tuple(g[:3]) + (g[4],):
        assert torch.isfinite(t).all()
    assert o.float().abs().max() < 1e-30 and ((ms.float() - 200).abs() < 1e-3).all() and ((ls.float() - 1).abs() < 1e-2).all()


@pytest.mark.parametrize("dt,E,causal,pad", [("bf16", 64, False, False), ("f16", 128, True, True), ("f32", 32, True, False),
                                             ("bf16", 8, False, True)])
def test_minus_inf_sinks_are_the_call_without_sinks(pkg, dev, dt, E, causal, pad):
    d = inputs(("noinf", dt, E), 2, 4, 2, 1100, 1100, E, dt, dev, pad=pad, sinks=[-INF] * 4)
    o, ms, ls, dq, dk, dv, _, ds = run(pkg, d, causal, sinks=d["sinks"])
    o2, ms2, ls2 = pkg._flash_attention(d["q"], d["k"], d["v"], causal=causal, kpad_mask=d["mask"])
    dq2, dk2, dv2, _ = pkg.grad_flash_attention(d["do"], o2, ms2, ls2, d["q"], d["k"], d["v"], causal=causal, kpad_mask=d["mask"])
    # the sink kernels are compiled apart from the kernels without sinks (whose code stays exactly as it was), so the two may round
    # differently in the last place (e.g. where the compiler contracts a multiply-add); the NaN pattern and dsinks = 0 are exact
    for name, a, b in (("o", o, o2), ("ms", ms, ms2), ("ls", ls, ls2)):
        assert (torch.isnan(a) == torch.isnan(b)).all()
        assert_close(name, a, to64(b), dt, floor=True)
    for name, a, b in (("dq", dq, dq2), ("dk", dk, dk2), ("dv", dv, dv2)):
        assert_close(name, a, to64(b), dt, floor=True, kind="grad")
    assert (ds == 0).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_autograd_through_flash_attention(pkg, dev, dt):
    d = inputs(("ag", dt), 2, 4, 2, 257, 257, 64, dt, dev, sinks=[0.5, -1.0, 2.0, -INF])
    leaves = [d[n].clone().requires_grad_(True) for n in ("q", "k", "v")]
    s = d["sinks"].to(TORCH_DT[dt]).clone().requires_grad_(True)
    o = pkg.flash_attention(*leaves, causal=True, window=(60, 0), sinks=s)
    o.backward(d["do"])
    o2, ms, ls = pkg._flash_attention(d["q"], d["k"], d["v"], causal=True, window=(60, 0), sinks=s.detach())
    ref = pkg.grad_flash_attention(d["do"], o2, ms, ls, d["q"], d["k"], d["v"], causal=True, window=(60, 0), sinks=s.detach())
    assert torch.equal(o.detach(), o2)
    for leaf, r in zip(leaves, ref[:3]):
        assert torch.equal(leaf.grad, r)
    assert s.grad.dtype == s.dtype and torch.equal(s.grad, ref[4].to(s.dtype))


# ---- a gpt-oss-like layer at full size -------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, (127, 0)])
def test_gptoss_layer(pkg, dev, window):
    """bf16 E64 QH64 KH8 L4096 B1 causal.  Causal rows < 512 depend on keys < 512 only: two (batch, kv-head) slices of those rows are
    checked against the reference, every row's dsinks against the formula on the library's own (o, ms, ls, dO)."""
    L, QH, KH = 4096, 64, 8
    rng = np.random.default_rng(7)
    sk = rng.standard_normal(QH).astype(np.float32)
    d = inputs(("gptoss", window), 1, QH, KH, L, L, 64, "bf16", dev, sinks=list(sk))
    o, ms, ls, dq, dk, dv, _, ds = run(pkg, d, True, window=window, sinks=d["sinks"])
    R = 512
    for kh in (0, 5):
        hs = slice(kh * 8, kh * 8 + 8)
        sub = lambda t: to64(t[:, hs, :R]) if t.shape[1] == QH else to64(t[:, kh:kh + 1, :R])
        o_ref, ms_ref, ls_ref = attention_fwd(sub(d["q"]), sub(d["k"]), sub(d["v"]), causal=True, window=window,
                                              sinks=sk[hs].astype(np.float64))
        assert_close("o", o[:, hs, :R], o_ref, "bf16", floor=True)
        assert_close("ms", to64(ms[:, hs, :R]), ms_ref, "bf16", floor=True)
        assert_close("ls", to64(ls[:, hs, :R]), ls_ref, "bf16", 2.0, floor=True)
    want = -(np.exp(sk.astype(np.float64)[None, :, None] - to64(ms)) / to64(ls) * (to64(d["do"]) * to64(o)).sum(-1)).sum(axis=(0, 2))
    np.testing.assert_allclose(to64(ds), want, rtol=2e-5, atol=1e-3)
