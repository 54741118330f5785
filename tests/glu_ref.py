"""Reference of the gated MLP activations (test infrastructure, not a test file).

include/nnop_hip.h (nnop_glu): y = a(gate) * up and its pullback dgate = dy * up * a'(gate), dup = dy * a(gate), here in fp64 on the CPU
(torch double: numpy has no erf), evaluated on the inputs AS GIVEN -- a test rounds them to the element type first, so the only error
left in the library's result is its own fp32 arithmetic and the one rounding on store.  a' is written out by hand, not taken from
autograd; tests/test_z_glu_host.py checks it against finite differences and against autograd of the textbook formulas.
"""
import math

import torch

ACTS = ("silu", "gelu_tanh", "gelu_erf", "swiglu_oai")
OAI_ALPHA, OAI_LIMIT = 1.702, 7.0
K = math.sqrt(2.0 / math.pi)
C3 = 0.044715

# unit roundoff of the 16-bit element types; the fp32 figure is the project's YTOL["f32"] (tests/test_norms_gpu.py)
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
R_T = {"bf16": 2 * U16["bf16"], "f16": 2 * U16["f16"], "f32": 2e-6}


def f64(t):
    return t.detach().to("cpu", torch.float64)


def act_ref(g, act, alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """(a(g), a'(g)) in fp64; for swiglu_oai a = g' sigmoid(alpha g') with g' = min(g, limit) and a' = 0 beyond the bound"""
    g = f64(g)
    if act == "silu":
        s = torch.sigmoid(g)
        return g * s, s * (1 + g * (1 - s))
    if act == "gelu_tanh":
        t = torch.tanh(K * (g + C3 * g ** 3))
        return 0.5 * g * (1 + t), 0.5 * (1 + t) + 0.5 * g * (1 - t * t) * K * (1 + 3 * C3 * g * g)
    if act == "gelu_erf":
        cdf = 0.5 * torch.special.erfc(-g / math.sqrt(2.0))
        return g * cdf, cdf + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    if act == "swiglu_oai":
        gp = torch.clamp(g, max=limit)
        s = torch.sigmoid(alpha * gp)
        return gp * s, torch.where(g <= limit, s * (1 + alpha * gp * (1 - s)), torch.zeros_like(g))
    raise ValueError(act)


def glu_ref(gate, up, act, alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """y in fp64"""
    a, _ = act_ref(gate, act, alpha, limit)
    u = f64(up)
    if act == "swiglu_oai":
        u = torch.clamp(u, -limit, limit) + 1
    return a * u


def glu_grads_ref(dy, gate, up, act, alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """(dgate, dup) in fp64"""
    a, da = act_ref(gate, act, alpha, limit)
    dy, u = f64(dy), f64(up)
    if act == "swiglu_oai":
        inside = ((u >= -limit) & (u <= limit)).to(torch.float64)
        return dy * (torch.clamp(u, -limit, limit) + 1) * da, dy * a * inside
    return dy * u * da, dy * a


def textbook(gate, up, act, alpha=OAI_ALPHA, limit=OAI_LIMIT):
    """the formulas as a model's code writes them (differentiable torch, any dtype): what the fused call replaces"""
    F = torch.nn.functional
    if act == "silu":
        return F.silu(gate) * up
    if act == "gelu_tanh":
        return F.gelu(gate, approximate="tanh") * up
    if act == "gelu_erf":
        return F.gelu(gate, approximate="none") * up
    if act == "swiglu_oai":                      # gpt-oss
        gate = gate.clamp(min=None, max=limit)
        up = up.clamp(min=-limit, max=limit)
        glu = gate * torch.sigmoid(gate * alpha)
        return (up + 1) * glu
    raise ValueError(act)


# spacing of the subnormal numbers of each element type: a result below the normal range cannot be rounded with a RELATIVE
# error (fp16 cannot hold 1e-21 at all), so the gate allows one such spacing on top of the relative terms
TINY = {"f32": 2.0 ** -149, "f16": 2.0 ** -24, "bf16": 2.0 ** -133}


def gate_ok(got, ref, dt):
    """worst ratio of |got - ref| to the gate r_T |ref| + 2e-6 max|ref| (+ one subnormal spacing of the element type, which only
    matters where a result underflows); <= 1 passes.  got, ref: tensors, ref in fp64"""
    got, ref = f64(got), f64(ref)
    bound = R_T[dt] * ref.abs() + 2e-6 * ref.abs().max() + TINY[dt]
    err = (got - ref).abs()
    if not torch.isfinite(got).all():
        return float("inf")
    return float((err / bound.clamp_min(1e-300)).max()) if err.max() > 0 else 0.0


def interleave(g, u):
    """[..., n], [..., n] -> [..., 2n] with gate at even and up at odd positions"""
    return torch.stack((g, u), dim=-1).reshape(*g.shape[:-1], 2 * g.shape[-1])
