"""Logit soft-capping on the GPU: parity with the fp64 oracle through tests/attn_ref.py, the cap combined with pair bias, key
padding, window, sinks and GQA, a realistic cap on sharp scores, exactness (no cap = the call without the argument, repeatability,
saturation), autograd and sharding.  Semantics: include/nnop_hip.h (nnop_fa_fwd_softcap).  That the cap changes these inputs' results
by far more than the tolerances used here is checked without a GPU in tests/test_softcap_host.py."""
import numpy as np
import pytest
import torch

import softcap_cases
from attn_ref import cap_terms, check_parity, inputs
from util import to64

pytestmark = pytest.mark.gpu


# ---- parity grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", softcap_cases.parity_grid(), ids=lambda c: "{}-E{}-c{}-L{}x{}-cap{}".format(*c))
def test_softcap_parity(pkg, dev, case):
    dt, E, causal, QL, KL, cap = case
    check_parity(pkg, softcap_cases.grid_inputs(case, dev), dt, causal, softcap=cap)


# ---- combinations (E = 64, 517 x 517) ---------------------------------------------------------------------------------------------
COMBO_DT = ["bf16", "f32"]


@pytest.mark.parametrize("dt", COMBO_DT)
def test_cap_with_pair_bias(pkg, dev, dt):
    """dpair = dS: against the reference, and NOT scaled by the tanh derivative.  At q x 64 most scores sit at +-c, where
    1 - tanh^2 is ~0: a dpair that went through it would be ~0 where the true one is largest."""
    d = inputs(("pair", dt), 1, 2, 1, 517, 517, 64, dt, dev, pair=True)
    check_parity(pkg, d, dt, False, softcap=1.0)
    d["q"] = d["q"] * 64.0
    dp = to64(check_parity(pkg, d, dt, False, softcap=1.0, label="saturated ")[6])
    _, t, _ = cap_terms(to64(d["q"]), to64(d["k"]), 1.0)
    wrong = dp * np.transpose(1.0 - t * t, (0, 3, 2, 1))
    assert np.abs(dp - wrong).max() > 0.5 * np.abs(dp).max()


@pytest.mark.parametrize("dt", COMBO_DT)
def test_cap_with_key_padding_and_dead_rows(pkg, dev, dt):
    d = inputs(("pad", dt), 1, 2, 1, 517, 517, 64, dt, dev)
    mask = torch.ones(1, 517, dtype=torch.bool)
    mask[0, :5] = False                                       # under the causal rule rows 0 .. 4 see no key
    mask[0, 400:] = False
    d["mask"] = mask.to(dev)
    o = check_parity(pkg, d, dt, True, softcap=2.0)[0]
    assert torch.isnan(o[:, :, :5]).all() and torch.isfinite(o[:, :, 5:]).all()


@pytest.mark.parametrize("dt", COMBO_DT)
def test_cap_with_window(pkg, dev, dt):
    d = inputs(("win", dt), 1, 2, 1, 517, 517, 64, dt, dev)
    check_parity(pkg, d, dt, False, softcap=1.0, window=(100, 37))


@pytest.mark.parametrize("dt", COMBO_DT)
def test_cap_with_sinks(pkg, dev, dt):
    """the sink is not capped: sinks of 3 and -2 under a cap of 1 (a capped sink could never exceed 1)"""
    d = inputs(("sinks", dt), 1, 2, 1, 517, 517, 64, dt, dev)
    sinks = torch.tensor([3.0, -2.0], device=dev)
    check_parity(pkg, d, dt, True, softcap=1.0, sinks=sinks)


@pytest.mark.parametrize("dt", COMBO_DT)
def test_cap_with_causal_pair_and_padding(pkg, dev, dt):
    d = inputs(("all", dt), 1, 2, 1, 517, 517, 64, dt, dev, pair=True, pad=True)
    check_parity(pkg, d, dt, True, softcap=0.5)


@pytest.mark.parametrize("dt", COMBO_DT)
def test_cap_with_gqa(pkg, dev, dt):
    d = inputs(("gqa", dt), 1, 4, 1, 517, 517, 64, dt, dev)
    check_parity(pkg, d, dt, True, softcap=2.0)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_cap_with_pair_on_the_plain_hip_and_e128_kernels(pkg, dev, dt):
    """the pair-bias bodies that the E = 64 cases above do not run: E = 128 (32-key tiles) and E = 8 (plain HIP)"""
    for E in (128, 8):
        d = inputs(("pair", dt, E), 1, 2, 1, 160, 130, E, dt, dev, pair=True)
        check_parity(pkg, d, dt, True, softcap=1.0, window=(64, -1), label=f"E{E} ")


# ---- realistic cap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", softcap_cases.REALISTIC, ids=lambda c: "{}-E{}-L{}x{}-cap{}".format(*c))
def test_realistic_cap_on_sharp_scores(pkg, dev, case):
    """c = 30 (Grok-1) on scores of std 8"""
    dt, E, QL, KL, cap = case
    check_parity(pkg, softcap_cases.realistic_inputs(case, dev), dt, False, softcap=cap)


# ---- exactness ---------------------------------------------------------------------------------------------------------------------
def _eq(a, b):
    return torch.equal(a, b) or ((torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num()))


@pytest.mark.parametrize("shape", [("bf16", 64, 2048, 2048, 4, 4, 4, False), ("f32", 64, 600, 700, 2, 2, 2, True)],
                         ids=["bf16-duo-w64", "f32"])
def test_no_cap_is_bitwise_the_call_without_the_argument(pkg, dev, shape):
    dt, E, QL, KL, QH, KH, B, causal = shape
    d = inputs(shape, B, QH, KH, QL, KL, E, dt, dev)
    q, k, v, do = d["q"], d["k"], d["v"], d["do"]
    if dt == "bf16":                                           # the shape does run the fast forms without a cap
        desc = pkg._lib.FaDesc(dtype=pkg._lib.NNOP_BF16, emb=E, ql=QL, kl=KL, qh=QH, kh=KH, batch=B, causal=int(causal))
        assert pkg._lib.fwd_form(desc) in ("fa_fwd_duo_kernel", "fa_fwd_w64_kernel")
        assert pkg._lib.bwd_kernels(desc) == ("fa_bwd_w64_kernel<dK/dV>", "fa_bwd_w64_kernel<dQ>")
    ref_f = pkg._flash_attention(q, k, v, causal=causal)
    ref_b = pkg.grad_flash_attention(do, *ref_f, q, k, v, causal=causal)[:3]
    for cap in (None, 0.0, 0):
        got_f = pkg._flash_attention(q, k, v, causal=causal, softcap=cap)
        got_b = pkg.grad_flash_attention(do, *got_f, q, k, v, causal=causal, softcap=cap)[:3]
        for name, a, b in zip(("o", "ms", "ls", "dq", "dk", "dv"), tuple(got_f) + tuple(got_b), tuple(ref_f) + tuple(ref_b)):
            assert _eq(a, b), (cap, name)
        assert torch.equal(pkg.flash_attention(q, k, v, causal=causal, softcap=cap), ref_f[0])


@pytest.mark.parametrize("dt,E,causal,pad", [("bf16", 64, True, False), ("f32", 128, False, True), ("f16", 8, False, False)])
def test_capped_runs_are_repeatable(pkg, dev, dt, E, causal, pad):
    d = inputs(("rep", dt, E), 2, 4, 2, 700, 650, E, dt, dev, pad=pad)
    runs = []
    for _ in range(2):
        o, ms, ls = pkg._flash_attention(d["q"], d["k"], d["v"], causal=causal, kpad_mask=d["mask"], softcap=1.0)
        g = pkg.grad_flash_attention(d["do"], o, ms, ls, d["q"], d["k"], d["v"], causal=causal, kpad_mask=d["mask"], softcap=1.0)
        runs.append([o, ms, ls] + list(g[:3]))
    for a, b in zip(*runs):
        assert torch.equal(a.nan_to_num(), b.nan_to_num())


@pytest.mark.parametrize("dt,E", [("bf16", 64), ("f32", 64), ("f16", 8), ("bf16", 128)])
def test_saturated_cap_is_finite_and_right(pkg, dev, dt, E):
    """q x 64 under c = 1: every score sits at +-c; no inf or NaN comes out of the tanh"""
    d = inputs(("sat", dt, E), 1, 2, 1, 300, 333, E, dt, dev, qscale=64.0)
    out = check_parity(pkg, d, dt, True, softcap=1.0)
    for t in out[:6]:
        assert torch.isfinite(t).all()


# ---- other layers --------------------------------------------------------------------------------------------------------------
def test_autograd_matches_grad_flash_attention(pkg, dev):
    d = inputs("autograd", 2, 4, 2, 333, 333, 64, "bf16", dev, pair=True)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0], device=dev)
    leaves = [d[n].clone().requires_grad_(True) for n in ("q", "k", "v", "pair")] + [sinks.clone().requires_grad_(True)]
    o = pkg.flash_attention(*leaves[:4], causal=True, sinks=leaves[4], softcap=1.0)
    o.backward(d["do"])
    o2, ms, ls = pkg._flash_attention(d["q"], d["k"], d["v"], d["pair"], causal=True, sinks=sinks, softcap=1.0)
    ref = pkg.grad_flash_attention(d["do"], o2, ms, ls, d["q"], d["k"], d["v"], d["pair"], causal=True, sinks=sinks, softcap=1.0)
    assert torch.equal(o.detach(), o2)
    for leaf, r in zip(leaves, ref):
        assert torch.equal(leaf.grad, r)
    # and the cap is in it: the uncapped call differs
    assert not torch.equal(o2, pkg._flash_attention(d["q"], d["k"], d["v"], d["pair"], causal=True, sinks=sinks)[0])


def test_sharded_cap_is_bitwise_the_unsharded_call(pkg, dev):
    from importlib import import_module
    shard = import_module(pkg.__name__ + ".shard")
    world = 2
    d = inputs(("shard", world), 3, 4, 2, 400, 400, 64, "bf16", dev)
    q, k, v, do = d["q"], d["k"], d["v"], d["do"]
    o, ms, ls = pkg._flash_attention(q, k, v, causal=True, softcap=2.0)
    dq, dk, dv, _ = pkg.grad_flash_attention(do, o, ms, ls, q, k, v, causal=True, softcap=2.0)
    rep = q.shape[1] // k.shape[1]
    seen = 0
    for rank in range(world):
        for rect, o_r, dq_r, dk_r, dv_r, _ in shard.flash_attention_sharded_fwd_bwd(q, k, v, do, causal=True, world=world,
                                                                                    rank=rank, softcap=2.0):
            qs = (slice(rect.b0, rect.b1), slice(rect.kh0 * rep, rect.kh1 * rep))
            ks = (slice(rect.b0, rect.b1), slice(rect.kh0, rect.kh1))
            assert torch.equal(o_r, o[qs]) and torch.equal(dq_r, dq[qs])
            assert torch.equal(dk_r, dk[ks]) and torch.equal(dv_r, dv[ks])
            seen += rect.units
        local = shard.flash_attention_sharded(q, k, v, causal=True, world=world, rank=rank, softcap=2.0)
        rects = shard.rectangles(3, 2, world, rank)
        want = [o[r.b0:r.b1, r.kh0 * rep:r.kh1 * rep].reshape(r.units, rep, *o.shape[2:]) for r in rects]
        assert torch.equal(local, torch.cat(want, dim=0))
    assert seen == 3 * 2
