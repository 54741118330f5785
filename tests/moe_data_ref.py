"""Reference of the mixture-of-experts permute and weighted combine (include/nnop_hip_moe_data.h) and the gates their GPU tests use (test
infrastructure, not a test file).

The header's four formulas in fp64 numpy, evaluated on the ROUNDED inputs (the rows as the device sees them).  An entry v of perm / slot
is valid iff 0 <= v < S = T k; every other entry is skipped: a row of zeros, no term in a sum, a zero in dw.

The gates are derived, not calibrated, from the unit roundoffs u (f32 2^-24, f16 2^-11, bf16 2^-8) and the contract "fp32 sums in
ascending j, one rounding on the store".  A k-term fp32 sum of products, each product rounded once or fused, is within
(k + 2) 2^-24 A of the exact one to first order, A = sum_j |w_j| |ys_j| element-wise (k - 1 additions, one product rounding, and one
unit of slack for the second-order terms); rounding that to the output type adds u |ref|, and in f16 a result below the normal range
adds half the subnormal spacing, 2^-25 (the other two types have the exponent range of fp32, where that floor is negligible but kept):
    y, dx   |got - ref| <= u |ref| + (k + 2) 2^-24 A + floor                 A = sum_j |w_j ys_j|  (dx: sum_j |dxs_j|)
    dys     the same with k = 1 and A = |w dy|: a single product rounded once
    dw      |got - ref| <= 2^-24 |ref| + D 2^-24 sum_c |dy_c ys_c|            the any-order bound of a D-term fp32 sum; dw is fp32
    xs      exact
The dw bound holds for every summation tree (sequential, pairwise, per lane and then across lanes), so it does not pin the kernel's
reduction order.  A NaN pattern that differs from the reference's is an infinite error, as in moe_ref._ratio."""
import numpy as np
import torch

import moe_ref

U = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
FLOOR = {"f32": 2.0 ** -150, "f16": 2.0 ** -25, "bf16": 2.0 ** -134}      # half the subnormal spacing of the type
EPS32 = 2.0 ** -24
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def valid(v, S):
    v = np.asarray(v).astype(np.int64)
    return (v >= 0) & (v < S)


# ---- the four formulas ---------------------------------------------------------------------------------------------------------------
def permute_ref(x, perm, k):
    """xs [S, D] = x[perm // k], zeros for a skipped slot; in the dtype of x (a copy)"""
    x, perm = np.asarray(x), np.asarray(perm).astype(np.int64)
    ok = valid(perm, perm.size)
    xs = x[np.where(ok, perm, 0) // k].copy()
    xs[~ok] = 0
    return xs


def _terms(rows, w, slot):
    """[T, k, D] fp64: w[t, j] rows[slot[t, j]], 0 for a skipped j"""
    rows, slot = np.asarray(rows, np.float64), np.asarray(slot).astype(np.int64)
    ok = valid(slot, rows.shape[0])
    g = rows[np.where(ok, slot, 0)]
    if w is not None:
        with np.errstate(invalid="ignore"):
            g = np.where(ok[..., None], np.asarray(w, np.float64)[..., None] * g, 0.0)
    return np.where(ok[..., None], g, 0.0)


def combine_ref(ys, w, slot):
    """-> (y [T, D] fp64, A [T, D] = sum_j |w_j ys_j|);  w = None: every weight 1 (the pullback of the permute)"""
    t = _terms(ys, w, slot)
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def permute_bwd_ref(dxs, slot):
    return combine_ref(dxs, None, slot)


def combine_bwd_ref(dy, ys, w, perm, slot):
    """-> (dys [S, D], dw [T, k], B [T, k] = sum_c |dy_c ys_c|) in fp64"""
    dy, ys, w = np.asarray(dy, np.float64), np.asarray(ys, np.float64), np.asarray(w, np.float64)
    perm, slot = np.asarray(perm).astype(np.int64), np.asarray(slot).astype(np.int64)
    S, k = perm.size, slot.shape[-1]
    okp = valid(perm, S)
    p = np.where(okp, perm, 0)
    dys = np.where(okp[:, None], w.reshape(-1)[p][:, None] * dy[p // k], 0.0)
    oks = valid(slot, S)
    prod = dy[:, None, :] * ys[np.where(oks, slot, 0)]
    dw = np.where(oks, prod.sum(axis=-1), 0.0)
    B = np.where(oks, np.abs(prod).sum(axis=-1), 0.0)
    return dys, dw, B


# ---- gates: worst |got - ref| / tolerance, <= 1 passes ---------------------------------------------------------------------------------
def _ratio(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    tol = np.broadcast_to(tol, ref.shape)[ok]
    got, ref = got[ok], ref[ok]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / tol)
    return float("inf") if np.isnan(r).any() else float(r.max())


def sum_tol(ref, A, k, dt):
    return U[dt] * np.abs(ref) + (k + 2) * EPS32 * np.asarray(A, np.float64) + FLOOR[dt]


def y_ratio(got, ref, A, k, dt):
    """y and dx"""
    return _ratio(got, ref, sum_tol(np.asarray(ref, np.float64), A, k, dt))


def dys_ratio(got, ref, dt):
    ref = np.asarray(ref, np.float64)
    return _ratio(got, ref, sum_tol(ref, np.abs(ref), 1, dt))


def dw_ratio(got, ref, B, D):
    ref = np.asarray(ref, np.float64)
    return _ratio(got, ref, EPS32 * np.abs(ref) + D * EPS32 * np.asarray(B, np.float64))


def exact(got, ref):
    """0 if bitwise equal as numbers with the same NaN pattern, else inf"""
    return 0.0 if np.array_equal(np.asarray(got), np.asarray(ref), equal_nan=True) else float("inf")


# ---- an fp32 evaluation on the CPU, as the contract words it (the host tests hold the gates against it) --------------------------------
def round_to(a, dt):
    """fp32 numpy -> the values of dtype dt, as fp64"""
    return torch.tensor(np.asarray(a, np.float32)).to(TORCH_DT[dt]).double().numpy()


def combine_f32(ys, w, slot, dt, drop=None):
    """fp32 accumulation in ascending j, rounded once by torch; drop = j: that term is left out (a wrong kernel)"""
    ys32, slot = np.asarray(ys, np.float32), np.asarray(slot).astype(np.int64)
    ok = valid(slot, ys32.shape[0])
    acc = np.zeros((slot.shape[0], ys32.shape[1]), np.float32)
    for j in range(slot.shape[1]):
        if j == drop:
            continue
        wj = np.float32(1.0) if w is None else np.asarray(w, np.float32)[:, j, None]
        term = (wj * ys32[np.where(ok[:, j], slot[:, j], 0)]).astype(np.float32)
        acc = np.where(ok[:, j, None], (acc + term).astype(np.float32), acc)
    return round_to(acc, dt)


def dw_f32(dy, ys, slot, order="sequential", drop=None):
    """the fp32 dot products, summed sequentially or pairwise; drop = c: that column is left out"""
    dy32, ys32, slot = np.asarray(dy, np.float32), np.asarray(ys, np.float32), np.asarray(slot).astype(np.int64)
    ok = valid(slot, ys32.shape[0])
    prod = (dy32[:, None, :] * ys32[np.where(ok, slot, 0)]).astype(np.float32)
    if drop is not None:
        prod = np.delete(prod, drop, axis=-1)
    s = np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1] if order == "sequential" else prod.sum(axis=-1, dtype=np.float32)
    return np.where(ok, s, np.float32(0)).astype(np.float64)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_plan(seed, T, k, E, skip=0.0, idx=None):
    """(idx [T, k], perm [T k], slot [T, k]) int32 from random expert ids, a fraction `skip` of them -1 (not local)"""
    rng = np.random.default_rng(seed)
    if idx is None:
        idx = rng.integers(0, E, size=(T, k))
        if skip:
            idx[rng.random((T, k)) < skip] = -1
    idx = np.asarray(idx).astype(np.int32)
    _, _, perm, slot = moe_ref.plan_ref(idx, E)
    return idx, perm, slot


def make_rows(seed, n, D, dt, ld=None):
    """N(0, 1) rows rounded to dt, as fp32 numpy [n, ld]; the padding columns D ... ld-1 hold 7.0"""
    rng = np.random.default_rng(seed)
    a = np.full((n, ld or D), 7.0, np.float32)
    a[:, :D] = round_to(rng.standard_normal((n, D)).astype(np.float32), dt)
    return a


def make_weights(seed, T, k):
    """a normalised positive vector per token, fp32"""
    rng = np.random.default_rng(seed)
    w = rng.random((T, k)).astype(np.float32) + np.float32(0.05)
    return (w / w.sum(-1, keepdims=True)).astype(np.float32)
