"""Reference of the decode expert forward with the gated activation in its epilogue (include/nnop_hip_moe_mx_decode_glu.h) and the gate
its tests use (test infrastructure, not a test file).  It stands on tests/moe_linear_ref.py (linear_ref: the fp64 pre-activations and
the sums of absolute values their bound needs), tests/mx_ref.py (dequant: the weights a code and a scale byte mean) and tests/glu_ref.py
(glu_ref / act_ref: the activations in fp64).

The gate is derived, not calibrated.  The kernel holds the pre-activations p in fp32; by moe_linear_ref's bound without its rounding
term each is within
    delta = (K + 3) 2^-23 (A + |b|)
of the fp64 value, A the sum of the absolute values of the K products.  The activation h = a(gate) * upside(up) is then evaluated in
fp32 and rounded once.  With dg, du the delta of the gate and the up element and L = 1.13 a bound of |a'| for all four activations
(SiLU's maximum 1.0998 at any alpha, since a(g) = s(alpha g) / alpha with s the SiLU; GELU's 1.129), and the Lipschitz constant 1 of the
clamps,
    |a(gate~) - a(gate)| <= L dg          |upside(up~) - upside(up)| <= du
    |got - ref| <= 2 u |ref| + 2e-6 max|ref| + L (|upside| + du) dg + (|a| + L dg) du + floor
The first two terms are glu_ref.gate_ok's own (the fp32 activation arithmetic and the one rounding), floor is glu_ref.TINY.  L and the
clamp's constant are global, so the bound holds across the kinks at +-limit, where a local derivative would not.  Nothing in it depends
on a summation order."""
import numpy as np
import torch

import glu_ref
import moe_gemm_ref as g
import moe_linear_ref as lin
import mx_ref
from moe_linear_ref import EPS_MM, offsets_of, ranges, round_to, rows_of  # noqa: F401  (re-exported)

L_ACT = 1.13
LAYOUTS = ("interleaved", "halves")


def split(p, layout):
    """[..., 2 I] -> (gate, up), each [..., I]"""
    I = p.shape[-1] // 2
    return (p[..., 0::2], p[..., 1::2]) if layout == "interleaved" else (p[..., :I], p[..., I:])


def to_halves(a, axis):
    """rows (or columns) 2j, 2j+1 of an interleaved array -> j, I + j: the same weights laid out the other way"""
    a = np.asarray(a)
    idx = np.concatenate([np.arange(0, a.shape[axis], 2), np.arange(1, a.shape[axis], 2)])
    return np.ascontiguousarray(np.take(a, idx, axis=axis))


def gather(x, perm, k):
    """xs[s] = x[perm[s] // k], a row of zeros for an entry outside [0, T k): moe_permute's formula"""
    x, perm = np.asarray(x), np.asarray(perm).astype(np.int64)
    ok = (perm >= 0) & (perm < x.shape[0] * k)
    xs = np.zeros((perm.size, x.shape[1]), x.dtype)
    xs[ok] = x[perm[ok] // k]
    return xs


def upside_ref(up, act, limit):
    up = np.asarray(up, np.float64)
    return np.clip(up, -limit, limit) + 1 if act == "swiglu_oai" else up


def glu_decode_ref(xs, w, offsets, bias, act, layout, alpha=glu_ref.OAI_ALPHA, limit=glu_ref.OAI_LIMIT):
    """xs [S, K] (slot order: gather first), w [E, 2 I, K] the dequantised weights -> dict(h fp64 [S, I], tol terms, gate, up)"""
    K = np.asarray(xs).shape[1]
    p, A, B = lin.linear_ref(xs, w, offsets, bias)
    delta = (K + 3) * EPS_MM * (A + B)
    gate, up = split(p, layout)
    dg, du = split(delta, layout)
    tg, tu = torch.tensor(np.ascontiguousarray(gate)), torch.tensor(np.ascontiguousarray(up))
    h = glu_ref.glu_ref(tg, tu, act, alpha, limit).numpy()
    a = glu_ref.act_ref(tg, act, alpha, limit)[0].numpy()
    return dict(h=h, a=a, upside=upside_ref(up, act, limit), dg=dg, du=du, gate=gate, up=up, p=p)


def tol(r, dt):
    h = np.abs(r["h"])
    return (glu_ref.R_T[dt] * h + 2e-6 * (h.max() if h.size else 0.0) + L_ACT * (np.abs(r["upside"]) + r["du"]) * r["dg"]
            + (np.abs(r["a"]) + L_ACT * r["dg"]) * r["du"] + glu_ref.TINY[dt])


def ratios(got, r, dt):
    return lin._ratios(got, r["h"], tol(r, dt))


def worst(got, r, dt):
    return lin.worst(ratios(got, r, dt))


def rms(got, r):
    d = np.asarray(got, np.float64) - r["h"]
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def x_scale(xs, w, offsets, layout="interleaved", target=5.0, limit=glu_ref.OAI_LIMIT):
    """the power of two by which unit-scale rows are to be multiplied so that the pre-activations of the rows inside the experts have a
    standard deviation near `target`: with unit-scale rows every swiglu_oai element saturates and a test sees nothing.  It is chosen from
    the fp64 reference alone.  Where the rows inside the experts hold at least 1024 outputs and, at that scale, one of gate > limit,
    up > limit, up < -limit holds for fewer than 3 % of them (a shape with a handful of weight rows, whose scale bytes differ by up to
    2^12, has a handful of very different column deviations), the scale is doubled, at most four times, until each does"""
    p, _, _ = lin.linear_ref(xs, w, offsets, None)
    inside = rows_of(offsets, p.shape[0]) >= 0
    sd = float(p[inside].std()) if inside.any() else 1.0
    n = int(np.round(np.log2(target / max(sd, 1e-30))))
    gate, up = split(p[inside], layout)
    if gate.size >= 1024:
        for _ in range(4):
            s = 2.0 ** n
            if min((s * gate > limit).mean(), (s * up > limit).mean(), (s * up < -limit).mean()) >= 0.03:
                break
            n += 1
    return 2.0 ** n


def saturation(r, limit=glu_ref.OAI_LIMIT, inside=None):
    """fractions of (gate > limit, up > limit, up < -limit) among the elements of the rows inside the experts"""
    gate, up = (r["gate"], r["up"]) if inside is None else (r["gate"][inside], r["up"][inside])
    return float((gate > limit).mean()), float((up > limit).mean()), float((up < -limit).mean())


# ---- fp32 evaluations on the CPU (the host tests hold the gate against them, and against wrong ones) ------------------------------------
def _act_f32(gate, up, act, alpha, limit, plus1=True, clamp=True):
    gate, up = torch.tensor(np.ascontiguousarray(gate, np.float32)), torch.tensor(np.ascontiguousarray(up, np.float32))
    if act == "swiglu_oai":
        if clamp:
            gate, up = gate.clamp(max=limit), up.clamp(-limit, limit)
        y = gate * torch.sigmoid(gate * np.float32(alpha)) * (up + 1 if plus1 else up)
    else:
        y = glu_ref.textbook(gate, up, act)
    return y.numpy().astype(np.float32)


def glu_decode_f32(xs, w, offsets, dt, bias, act, layout, alpha=glu_ref.OAI_ALPHA, limit=glu_ref.OAI_LIMIT, order="blas", short=0,
                   shift=0, swap=False, plus1=True, clamp=True, round_p=False):
    """the formula in fp32: the product in BLAS order or one sequential chain, the bias added in fp32, the activation in fp32, one
    rounding to dt.  Wrong forms: short = 8 (the last 8 terms dropped), shift = 1 (expert e uses the weights of expert e + 1), swap (gate
    and up exchanged), plus1 = False, clamp = False.  round_p: p rounded to dt in front of the activation (the two-call form)."""
    xs, w = np.asarray(xs, np.float32), np.asarray(w, np.float32)
    p = np.zeros((xs.shape[0], w.shape[1]), np.float32)
    for e, lo, hi in ranges(offsets, xs.shape[0]):
        acc = g._dot_f32(xs[lo:hi], w[(e + shift) % w.shape[0]], order, short)
        if bias is not None:
            acc = (acc + np.asarray(bias, np.float32)[e]).astype(np.float32)
        p[lo:hi] = acc
    if round_p:
        p = round_to(p, dt).astype(np.float32)
    gate, up = split(p, layout)
    if swap:
        gate, up = up, gate
    return round_to(_act_f32(gate, up, act, alpha, limit, plus1, clamp), dt)


def dequant(blocks, scales, dt):
    return mx_ref.dequant(blocks, scales, dt)
