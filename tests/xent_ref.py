"""Reference of the cross-entropy loss (test infrastructure, not a test file).

include/nnop_hip.h (nnop_cross_entropy), written out by hand in fp64 on the CPU (torch double), evaluated on the inputs AS GIVEN -- a
test rounds them to the element type first, so the only error left in the library's result is its own fp32 arithmetic and the one
rounding on store.  For a row x[0..n) with target t:
    z = x | c tanh(x / c);  lse = log sum exp z;  p = exp(z - lse)
    loss = (1 - eps)(lse - z_t) + eps (lse - mean z) + zeta lse^2
    dx_j = g [p_j (1 + 2 zeta lse) - (1 - eps)[j = t] - eps / n] (1 - (z_j / c)^2)
Ignored rows (stored target == ignore_index): loss 0, dx 0.  Any other target outside [0, n) after index_base is subtracted: NaN loss,
NaN dx row.  tests/test_z_xent_host.py checks the gradient against autograd of torch's own cross_entropy and finite differences.

The gates (derived in the issue that introduced the operator, not fitted to the library):
    loss, lse   |got - ref| <= 4e-6 max(1, |ref|, |lse_ref|, max_j |z_j|)
    dlogits     |got - ref| <= r |ref| + 2e-6 |g| (1 + 2 zeta |lse_ref|) + TINY[T],   r = 2^-7 (bf16), 2^-10 (fp16), 1e-5 (fp32)
"""
import math

import torch

from glu_ref import TINY, f64

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
R_GRAD = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10, "f32": 1e-5}
LOSS_RTOL = 4e-6
GRAD_ATOL = 2e-6


def capped(x, cap):
    x = f64(x)
    return cap * torch.tanh(x / cap) if cap else x


def xent_ref(x, t, *, ignore_index=-100, eps=0.0, zeta=0.0, cap=0.0, index_base=0):
    """-> dict(loss, lse, z, tt, ignored, bad): fp64 [rows], z [rows, n]; tt the zero-based class clamped into the row"""
    z = capped(x, cap)
    n = z.shape[-1]
    t = t.detach().to("cpu", torch.int64)
    ignored = t == ignore_index
    tt = t - index_base
    bad = ~ignored & ((tt < 0) | (tt >= n))
    tt = torch.where(ignored | bad, torch.zeros_like(tt), tt)
    lse = torch.logsumexp(z, -1)
    zt = z.gather(-1, tt[..., None])[..., 0]
    loss = lse - zt
    if eps:
        loss = (1 - eps) * loss + eps * (lse - z.mean(-1))
    if zeta:
        loss = loss + zeta * lse * lse
    loss = torch.where(ignored, torch.zeros_like(loss), loss)
    loss = torch.where(bad, torch.full_like(loss, math.nan), loss)
    return dict(loss=loss, lse=lse, z=z, tt=tt, ignored=ignored, bad=bad)


def xent_grad_ref(g, x, t, *, ignore_index=-100, eps=0.0, zeta=0.0, cap=0.0, index_base=0):
    """dx in fp64, the closed form"""
    r = xent_ref(x, t, ignore_index=ignore_index, eps=eps, zeta=zeta, cap=cap, index_base=index_base)
    z, lse = r["z"], r["lse"][..., None]
    n = z.shape[-1]
    g = f64(g)[..., None]
    p = torch.exp(z - lse)
    a = p * (1 + 2 * zeta * lse) if zeta else p
    onehot = torch.zeros_like(z).scatter_(-1, r["tt"][..., None], 1.0)
    dx = g * (a - (1 - eps) * onehot - eps / n)
    if cap:
        dx = dx * (1 - (z / cap) ** 2)
    dx = torch.where(r["ignored"][..., None], torch.zeros_like(dx), dx)
    dx = torch.where(r["bad"][..., None], torch.full_like(dx, math.nan), dx)
    return dx


def textbook(x, t, *, ignore_index=-100, eps=0.0, zeta=0.0, cap=0.0):
    """per-row losses as a trainer writes them (differentiable torch, any float dtype): what the fused call replaces"""
    z = cap * torch.tanh(x / cap) if cap else x
    loss = torch.nn.functional.cross_entropy(z, t, ignore_index=ignore_index, label_smoothing=eps, reduction="none")
    if zeta:
        loss = loss + zeta * torch.logsumexp(z, -1) ** 2 * (t != ignore_index)
    return loss


def _same_nonfinite(got, ref):
    """positions where ref is not finite must hold the same kind of value in got"""
    nf = ~torch.isfinite(ref)
    ok = (torch.isnan(got) == torch.isnan(ref)) & (torch.isfinite(got) == torch.isfinite(ref))
    ok &= ~(torch.isinf(ref)) | (got == ref)
    return nf, bool(ok.all())


def loss_ratio(got, ref, lse_ref, z):
    """worst |got - ref| / gate for loss or lse ([rows], ref in fp64); <= 1 passes; inf when a NaN / inf is not where the reference has it"""
    got, ref, lse_ref = f64(got), f64(ref), f64(lse_ref)
    nf, ok = _same_nonfinite(got, ref)
    if not ok:
        return math.inf
    zmax = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z)).amax(-1)
    mag = torch.stack([torch.ones_like(ref), torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0),
                       torch.nan_to_num(lse_ref.abs(), nan=0.0, posinf=0.0, neginf=0.0), zmax]).amax(0)
    err = torch.where(nf, torch.zeros_like(ref), (got - ref).abs())
    return float((err / (LOSS_RTOL * mag)).max())


def grad_ratio(got, ref, g, lse_ref, zeta, dt):
    """worst |got - ref| / gate for dlogits ([rows, n], ref in fp64, g and lse_ref [rows]); <= 1 passes"""
    got, ref = f64(got), f64(ref)
    nf, ok = _same_nonfinite(got, ref)
    if not ok:
        return math.inf
    lse_mag = torch.nan_to_num(f64(lse_ref).abs(), nan=0.0, posinf=0.0)
    bound = R_GRAD[dt] * torch.nan_to_num(ref.abs(), nan=0.0) + (GRAD_ATOL * f64(g).abs() * (1 + 2 * zeta * lse_mag))[..., None] + TINY[dt]
    err = torch.where(nf, torch.zeros_like(ref), (got - ref).abs())
    return float((err / bound).max())
