"""GPU tests of the cross-entropy loss (include/nnop_hip.h, nnop_cross_entropy / nnop_cross_entropy_bwd) against the fp64 reference of
tests/xent_ref.py, under the gates stated there.  Inputs are s * N(0, 1), s in {1, 4}, drawn in fp32 from a seeded numpy generator and
cast (the project's convention); the reference sees the rounded inputs.  Every test prints its worst error / gate ratio.

Measured on an MI355X: the whole file (55 cases) runs in 5.3 - 5.6 s, most of it the fp64 references on the CPU.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import xent_ref as ref

pytestmark = pytest.mark.gpu

DTS = ["f32", "f16", "bf16"]
# both sides of the launch rule's crossover (a row of 16384 bytes: n = 4096 in fp32, 8192 in 16 bits) are in the grid, with neighbours
GRID_N = [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 520, 1000, 4088, 4095, 4096, 4104, 8184, 8191, 8192, 8200, 32768, 50257, 128256,
          201088, 262152]
ALL = dict(eps=0.1, zeta=1e-4, cap=30.0)
KW = lambda o: dict(label_smoothing=o.get("eps", 0.0), z_loss=o.get("zeta", 0.0), softcap=o.get("cap", 0.0))


def make(dev, dt, rows, n, seed, s=1.0, ld=None, offset=0, index=torch.int64):
    """(x view [rows, n] on the device with row stride ld and a base `offset` elements into its buffer, targets, g, buffer)"""
    rng = np.random.default_rng(seed)
    ld = n if ld is None else ld
    buf = torch.from_numpy((s * rng.standard_normal((rows * ld + offset,))).astype(np.float32)).to(dev).to(ref.DT[dt])
    x = buf[offset:].view(rows, ld)[:, :n] if ld != n or offset else buf.view(rows, n)
    t = torch.from_numpy(rng.integers(0, n, rows)).to(dev).to(index)
    g = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(dev)
    return x, t, g, buf


def check(pkg, x, t, g, dt, opts=None, ignore_index=-100, what=""):
    """forward + pullback through the Python entry points against the reference; returns (loss, lse, dx) and the worst ratio"""
    opts = opts or {}
    loss, lse = pkg._cross_entropy(x, t, ignore_index=ignore_index, **KW(opts))
    dx = pkg.grad_cross_entropy(g, lse, x, t, ignore_index=ignore_index, **KW(opts))
    r = ref.xent_ref(x, t, ignore_index=ignore_index, **opts)
    dr = ref.xent_grad_ref(g, x, t, ignore_index=ignore_index, **opts)
    ratios = (ref.loss_ratio(loss, r["loss"], r["lse"], r["z"]), ref.loss_ratio(lse, r["lse"], r["lse"], r["z"]),
              ref.grad_ratio(dx, dr, g, r["lse"], opts.get("zeta", 0.0), dt))
    assert max(ratios) <= 1.0, f"{what} {dt} {tuple(x.shape)} {opts}: error / gate loss {ratios[0]:.3f} lse {ratios[1]:.3f} dlogits {ratios[2]:.3f}"
    return (loss, lse, dx), ratios


@pytest.mark.parametrize("s", [1.0, 4.0])
@pytest.mark.parametrize("dt", DTS)
def test_parity_grid(pkg, dev, dt, s):
    worst = np.zeros(3)
    for i, n in enumerate(GRID_N):
        for rows in ((1, 5, 37) if n <= 8200 else (3,)):
            x, t, g, _ = make(dev, dt, rows, n, 1000 * i + rows, s)
            worst = np.maximum(worst, check(pkg, x, t, g, dt, what="grid")[1])
    print(f"RATIO grid {dt} s={s:g}: loss {worst[0]:.3f} lse {worst[1]:.3f} dlogits {worst[2]:.3f}")


OPTION_SETS = [("ignore_some", {}), ("ignore_all", {}), ("eps", dict(eps=0.1)), ("zeta", dict(zeta=1e-4)), ("cap", dict(cap=30.0)),
               ("all", ALL), ("all_ignore_some", ALL)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [37, 1000, 50257])
def test_options(pkg, dev, dt, n):
    worst = np.zeros(3)
    for k, (name, opts) in enumerate(OPTION_SETS):
        x, t, g, _ = make(dev, dt, 6, n, 7 * n + k, 4.0)
        if "ignore_some" in name:
            t[1] = t[4] = -100
        if name == "ignore_all":
            t[:] = -100
        (loss, lse, dx), ratios = check(pkg, x, t, g, dt, opts, what=name)
        worst = np.maximum(worst, ratios)
        if name == "ignore_all":
            assert (dx == 0).all() and (loss == 0).all() and torch.isfinite(lse).all()
            assert torch.isnan(pkg.cross_entropy(x, t)) and pkg.cross_entropy(x, t, reduction="sum") == 0
    print(f"RATIO options {dt} n={n}: loss {worst[0]:.3f} lse {worst[1]:.3f} dlogits {worst[2]:.3f}")


def raw(pkg, x, t, g, lse, out, *, index_base=0, ignore_index=-100, opts=None, fwd=True):
    """the C entry points on explicit views (row strides from the tensors)"""
    L, o = pkg.losses, KW(opts or {})
    rows, n = x.shape
    d = L._desc(x, rows, n, x.stride(0) if rows > 1 else n, (out.stride(0) if rows > 1 else n) if out is not None else n, t, ignore_index,
                o["label_smoothing"], o["z_loss"], o["softcap"], index_base)
    if fwd:
        loss, lse = torch.empty(rows, dtype=torch.float32, device=x.device), torch.empty(rows, dtype=torch.float32, device=x.device)
        L._launch("nnop_cross_entropy", d, x, loss.data_ptr(), lse.data_ptr(), x.data_ptr(), t.data_ptr())
        return loss, lse
    L._launch("nnop_cross_entropy_bwd", d, x, out.data_ptr(), g.data_ptr(), lse.data_ptr(), x.data_ptr(), t.data_ptr())
    return out


@pytest.mark.parametrize("dt", DTS)
def test_target_types_index_base_and_positive_ignore_index(pkg, dev, dt):
    x, t, g, _ = make(dev, dt, 6, 1000, 11, 4.0)
    base, _ = check(pkg, x, t, g, dt, ALL)
    got32, _ = check(pkg, x, t.to(torch.int32), g, dt, ALL)
    assert all(torch.equal(a, b) for a, b in zip(base, got32))
    # index_base = 1 through the raw C call: stored targets one higher give bitwise the same results
    for index in (torch.int32, torch.int64):
        t1 = (t + 1).to(index)
        loss, lse = raw(pkg, x, t1, g, None, None, index_base=1, opts=ALL)
        dx = raw(pkg, x, t1, g, lse, torch.empty_like(x), index_base=1, opts=ALL, fwd=False)
        assert torch.equal(loss, base[0]) and torch.equal(lse, base[1]) and torch.equal(dx, base[2])
    # a stored 0 with index_base = 1 is invalid (NaN), and ignore_index is compared with the stored value
    t1 = (t + 1).clone()
    t1[2], t1[3] = 0, 5
    loss, lse = raw(pkg, x, t1, g, None, None, index_base=1, ignore_index=5)
    assert torch.isnan(loss[2]) and loss[3] == 0 and torch.isfinite(loss[[0, 1, 4, 5]]).all()
    # ignore_index positive and inside [0, n)
    t2 = t.clone()
    t2[0] = t2[3] = 7
    (loss, _, dx), _ = check(pkg, x, t2, g, dt, ALL, ignore_index=7)
    assert (loss[[0, 3]] == 0).all() and (dx[[0, 3]] == 0).all() and (loss[[1, 2, 4, 5]] != 0).all()


SENTINEL = {"f32": 0x7FC12345, "f16": 0x7E5A, "bf16": 0x7FC5}


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,ld,ld_grad,offset", [(50257, 50304, 50304, 0), (50257, 50304, 50264, 0), (1000, 1003, 1003, 0), (1000, 1003, 1024, 0),
                                                 (1000, 1024, 1024, 1), (1000, 1000, 1008, 0), (50257, 50257, 50257, 0), (4099, 4104, 4104, 1)])
def test_layouts_write_only_the_row_and_in_place_equals_out_of_place(pkg, dev, dt, n, ld, ld_grad, offset):
    rows, band = 5, 64
    x, t, g, xbuf = make(dev, dt, rows, n, n + ld + offset, 4.0, ld=ld, offset=offset)
    assert x.data_ptr() % 16 == (offset * x.element_size()) % 16
    (loss, lse, dx), ratios = check(pkg, x, t, g, dt, ALL, what="layout")
    print(f"RATIO layout {dt} n={n} ld={ld} ld_grad={ld_grad} offset={offset}: loss {ratios[0]:.3f} lse {ratios[1]:.3f} dlogits {ratios[2]:.3f}")
    # out of place into a sentinel-filled buffer with its own stride and a band on either side
    sent = torch.full((band + offset + rows * ld_grad + band,), SENTINEL[dt], dtype=_bits(x).dtype, device=dev)
    obuf = sent.clone().view(ref.DT[dt])
    out = obuf[band + offset: band + offset + rows * ld_grad].view(rows, ld_grad)[:, :n]
    pkg.grad_cross_entropy(g, lse, x, t, out=out, **KW(ALL))
    assert torch.equal(_bits(out), _bits(dx)), "a strided dlogits differs from the dense one"
    keep = torch.ones(obuf.numel(), dtype=torch.bool, device=dev)
    keep[band + offset: band + offset + rows * ld_grad].view(rows, ld_grad)[:, :n] = False
    assert torch.equal(_bits(obuf)[keep], sent[keep]), "bytes outside the rows of dlogits were written"
    # in place: bitwise the out-of-place gradient, the padding of the logits untouched
    before = _bits(xbuf).clone()
    same = pkg.grad_cross_entropy(g, lse, x, t, out=x, **KW(ALL))
    assert same is x and torch.equal(_bits(x), _bits(dx))
    keep = torch.ones(xbuf.numel(), dtype=torch.bool, device=dev)
    keep[offset:].view(rows, ld)[:, :n] = False
    assert torch.equal(_bits(xbuf)[keep], before[keep])


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_extremes(pkg, dev, dt):
    big = 65504.0 if dt == "f16" else 1e4
    inf = float("inf")
    for n in (1000, 8200):
        x, t, g, _ = make(dev, dt, 8, n, n, 1.0)
        x[0, :] = -big; x[0, 5] = big; t[0] = 5                  # the target holds all the mass
        x[1, :] = -big; x[1, 5] = big; t[1] = 6                  # ... and a target that holds none
        x[2, 3] = x[2, n - 1] = x[2, n // 2] = -inf; t[2] = 9    # -inf away from the target: p = 0, gradient 0
        x[3, 17] = -inf; t[3] = 17                               # -inf at the target: +inf loss
        x[4, :] = -inf                                           # all -inf: NaN, and row 5 stays finite
        x[6, :] = big                                            # all equal and huge
        (loss, lse, dx), ratios = check(pkg, x, t, g, dt, what="extremes")
        print(f"RATIO extremes {dt} n={n}: loss {ratios[0]:.3f} lse {ratios[1]:.3f} dlogits {ratios[2]:.3f}")
        assert (dx[2, [3, n - 1, n // 2]] == 0).all()
        assert loss[3] == inf and torch.isfinite(lse[3])
        assert torch.isnan(loss[4]) and torch.isnan(dx[4]).all()
        rest = [0, 1, 2, 5, 6, 7]
        assert torch.isfinite(loss[rest]).all() and torch.isfinite(lse[rest]).all() and torch.isfinite(dx[rest + [3]]).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [1000, 50257])
def test_invalid_targets_give_nan_rows_and_touch_nothing_else(pkg, dev, dt, n):
    x, t, g, _ = make(dev, dt, 5, n, 3 * n, 4.0)
    good, _ = check(pkg, x, t, g, dt, ALL)
    tb = t.clone()
    tb[1], tb[3] = n, -5
    (loss, lse, dx), _ = check(pkg, x, tb, g, dt, ALL, what="invalid")
    assert torch.isnan(loss[[1, 3]]).all() and torch.isnan(dx[[1, 3]]).all()
    for a, b in zip((loss, lse, dx), good):
        assert torch.equal(a[[0, 2, 4]], b[[0, 2, 4]])
    assert torch.equal(lse, good[1])                             # lse does not depend on the target
    assert torch.isnan(pkg.cross_entropy(x, tb, **KW(ALL)))


def test_offsets_past_2_31_elements(pkg, dev):
    rows, n = 65538, 32768                                       # 2^31 + 2^16 elements, 4 GiB of bf16
    x = torch.zeros(rows, n, dtype=torch.bfloat16, device=dev)
    rng = np.random.default_rng(5)
    t = torch.from_numpy(rng.integers(0, n, rows)).to(dev)
    g = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(dev)
    loss, lse = pkg._cross_entropy(x, t)
    want = torch.full((rows,), math.log(n), dtype=torch.float64)
    z = torch.zeros(rows, 1, dtype=torch.float64)
    assert ref.loss_ratio(loss, want, want, z) <= 1.0 and ref.loss_ratio(lse, want, want, z) <= 1.0
    pkg.grad_cross_entropy(g, lse, x, t, out=x)
    tail, tt, gt = x[-2:], t[-2:].cpu(), g[-2:].double().cpu()
    want_dx = torch.full((2, n), 2.0 ** -15, dtype=torch.float64)
    want_dx[torch.arange(2), tt] -= 1.0
    want_dx *= gt[:, None]
    ratio = ref.grad_ratio(tail, want_dx, gt, want[-2:], 0.0, "bf16")
    print(f"RATIO offsets bf16: dlogits {ratio:.3f}")
    assert ratio <= 1.0
    assert (x[0] != 0).any() and (x[rows // 2] != 0).any()
    del x


@pytest.mark.parametrize("dt", DTS)
def test_autograd_end_to_end(pkg, dev, dt):
    B, Lq, n = 3, 5, 1000
    x, t, _, _ = make(dev, dt, B * Lq, n, 21, 4.0)
    x, t = x.view(B, Lq, n), t.view(B, Lq)
    t[0, 1] = t[2, 3] = -100
    xr = x.detach().double().cpu()
    tr = t.cpu()
    up = {"mean": torch.tensor(1.7), "sum": torch.tensor(-0.6), "none": torch.from_numpy(np.random.default_rng(2).standard_normal((B, Lq)))}
    for reduction in ("mean", "sum", "none"):
        xd = xr.clone().requires_grad_(True)
        rows = ref.textbook(xd.view(-1, n), tr.view(-1), **ALL).view(B, Lq)
        want = {"mean": lambda: rows.sum() / (tr != -100).sum(), "sum": rows.sum, "none": lambda: rows}[reduction]()
        want.backward(up[reduction].double())
        grads = []
        for inplace in (False, True):
            xg = x.clone().requires_grad_(True)
            h = xg * 1.0                                          # a non-leaf, as the LM head's output is
            seen = []
            h.register_hook(lambda gr: seen.append(gr.data_ptr()))
            loss = pkg.cross_entropy(h, t, reduction=reduction, inplace_grad=inplace, **KW(ALL))
            assert loss.dtype == torch.float32 and loss.shape == want.shape
            # the loss gate of every row (magnitudes up to the cap, 30), summed for "sum"
            tol = ref.LOSS_RTOL * 30.0 * (B * Lq if reduction == "sum" else 1)
            assert (loss.double().cpu() - want.detach()).abs().max() <= tol
            loss.backward(up[reduction].to(dev).float())
            assert (seen[0] == h.data_ptr()) == inplace          # in place really aliases the logits
            grads.append(xg.grad)
            g_rows = (up[reduction].double() / ((tr != -100).sum() if reduction == "mean" else 1)).expand(B, Lq).reshape(-1)
            ratio = ref.grad_ratio(xg.grad.view(-1, n), xd.grad.view(-1, n), g_rows, torch.logsumexp(ref.capped(xr, 30.0), -1).view(-1), 1e-4, dt)
            assert ratio <= 1.0, (reduction, inplace, ratio)
        assert torch.equal(grads[0], grads[1])
    # no autograd path without requires_grad, or under no_grad
    assert pkg.cross_entropy(x, t).grad_fn is None and not pkg.cross_entropy(x, t).requires_grad
    with torch.no_grad():
        assert pkg.cross_entropy(x.clone().requires_grad_(True), t).grad_fn is None


def test_reproducible_and_sane_at_scale(pkg, dev):
    rows, n = 8192, 32768
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((64, n)).astype(np.float32)).to(dev).to(torch.bfloat16).repeat(rows // 64, 1)
    x = x * torch.linspace(0.5, 4.0, rows, device=dev)[:, None].to(torch.bfloat16)
    t = torch.from_numpy(rng.integers(0, n, rows)).to(dev)
    g = torch.ones(rows, device=dev)
    loss, lse = pkg._cross_entropy(x, t)
    dx = pkg.grad_cross_entropy(g, lse, x, t)
    loss2, lse2 = pkg._cross_entropy(x, t)
    dx2 = pkg.grad_cross_entropy(g, lse2, x, t)
    assert torch.equal(loss, loss2) and torch.equal(lse, lse2) and torch.equal(dx, dx2)
    assert (loss >= 0).all()
    # sum_j dx_j = sum p - 1 = 0 before rounding: n roundings to bf16 (2^-9 relative each) of terms with sum |dx_j| <= 2 (g = 1)
    assert (dx.sum(-1, dtype=torch.float64).abs() <= 2.0 ** -9 * 2 + 1e-5).all()
    xf = x.float()
    want = torch.nn.functional.cross_entropy(xf, t, reduction="none")
    ratio = ref.loss_ratio(loss.cpu(), want.double().cpu(), torch.logsumexp(xf, -1).double().cpu(), xf.abs().amax(-1, keepdim=True).double().cpu())
    print(f"RATIO scale bf16 vs F.cross_entropy in fp32: loss {ratio:.3f}")
    assert ratio <= 1.0
    assert abs(float(pkg.cross_entropy(x, t)) - float(want.double().mean())) <= ref.LOSS_RTOL * float(max(xf.abs().max(), lse.max()))
