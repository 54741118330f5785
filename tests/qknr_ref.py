"""Reference of the fused QK-norm + RoPE (include/nnop_hip_ext.h) and the gates its GPU tests use (test infrastructure, not a test file).

The header's formulas in fp64 numpy, evaluated on the ROUNDED inputs: q, k, w, cos, sin (and the incoming gradients) as the device sees
them.  Layouts: q [B, QH, L, D], k [B, KH, L, D], cos / sin [B, L, D] (first D/2 of a row read), wq / wk [D]."""
import numpy as np

from test_rope_gpu import TOL          # the project's RoPE gate (importing the module touches no GPU): q_out, k_out, dq, dk


def _f64(*a):
    return tuple(np.asarray(x, np.float64) for x in a)


def _rotate(x, cos, sin, sin_sign):
    """x [B, H, L, D]; cos, sin [B, L, D]: y1 = x1 c - x2 s, y2 = x2 c + x1 s with s = sin_sign * sin"""
    h = x.shape[-1] // 2
    c, s = cos[:, None, :, :h], sin_sign * sin[:, None, :, :h]
    x1, x2 = x[..., :h], x[..., h:]
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1)


def _rstd(x, eps):
    return 1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps)


def qknr_ref(q, k, wq, wk, cos, sin, eps=1e-6, offset=0.0):
    q, k, wq, wk, cos, sin = _f64(q, k, wq, wk, cos, sin)
    return tuple(_rotate(x * _rstd(x, eps) * (w + offset), cos, sin, 1.0) for x, w in ((q, wq), (k, wk)))


def qknr_grad_ref(dq2, dk2, q, k, wq, wk, cos, sin, eps=1e-6, offset=0.0):
    """-> (dq, dk, dwq, dwk)"""
    dq2, dk2, q, k, wq, wk, cos, sin = _f64(dq2, dk2, q, k, wq, wk, cos, sin)
    dx, dw = [], []
    for dy, x, w in ((dq2, q, wq), (dk2, k, wk)):
        D = x.shape[-1]
        rstd = _rstd(x, eps)
        dn = _rotate(dy, cos, sin, -1.0)
        m = dn * (w + offset)
        dd = (m * x).sum(axis=-1, keepdims=True)
        dx.append(rstd * m - rstd ** 3 * (dd / D) * x)
        dw.append((dn * x * rstd).reshape(-1, D).sum(axis=0))
    return dx[0], dx[1], dw[0], dw[1]


# ---- gates: worst |got - ref| / tolerance, <= 1 passes; a NaN or infinity where the reference has none is inf ----------------------------
def _ratio(got, ref, atol, rtol):
    got, ref = _f64(got, ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def out_ratio(got, ref, dt):
    """q_out, k_out, dq, dk: TOL of tests/test_rope_gpu.py, atol scaled by max(1, max|ref|)"""
    ref = np.asarray(ref, np.float64)
    return _ratio(got, ref, TOL[dt]["atol"] * max(1.0, float(np.abs(ref).max())), TOL[dt]["rtol"])


def dw_ratio(got, ref, rows):
    """dwq, dwk: the RMSNorm dw gate of tests/test_norms_gpu.py"""
    ref = np.asarray(ref, np.float64)
    return _ratio(got, ref, 1e-5 * float(np.abs(ref).max()) + 1e-6 * rows, 1e-4)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def positions(B, L, start=1000):
    """position ids that start at `start` and differ per batch"""
    return np.stack([np.arange(L, dtype=np.float32) + start + 17 * b for b in range(B)])


def make_inputs(seed, B, QH, KH, L, D, scale=1.0):
    """fp32 numpy: q, k, dq2, dk2 ~ N(0, scale^2) (q shifted by 0.25 scale), wq != wk ~ N(0, 1), cos / sin of positions()"""
    from oracle.naive_rope import llama_rotary_embedding
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    cos, sin = llama_rotary_embedding(D, positions(B, L))
    return dict(q=scale * (n(B, QH, L, D) + 0.25), k=scale * n(B, KH, L, D), dq2=n(B, QH, L, D), dk2=n(B, KH, L, D), wq=n(D), wk=n(D),
                cos=cos.astype(np.float32), sin=sin.astype(np.float32))
