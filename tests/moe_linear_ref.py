"""Reference of the expert linear layers (include/nnop_hip_moe_linear.h) and the gates their tests use (test infrastructure, not a test
file).  It stands on tests/moe_gemm_ref.py: the same offsets, the same three products, the same way of deriving a gate.

The header's four formulas in fp64 numpy, evaluated on the ROUNDED inputs, in both weight layouts: "nk" is w [E, N, K], "kn" is
w [E, K, N]; dw has the layout of w.  W_e(n, c) is w[e, n, c] or w[e, c, n].

The gates are derived, not calibrated.  u is the unit roundoff of the type that is stored (u_g for a gradient: that of grad_dtype), floor
half its subnormal spacing, 2^-23 the roundoff of an fp32 operation of undocumented rounding mode (moe_gemm_ref.EPS_MM), A the sum of the
absolute values of the terms:
    forward      |got - ref| <= u |ref| + (K + 3) 2^-23 (A + |b|) + floor      K products, K - 1 additions, the bias addition, slack
    dw           |got - ref| <= u_g |ref| + (R_e + 2) 2^-23 A + floor          R_e the expert's row count; moe_gemm_ref's bound
    db           the same with A = sum |dys|                                    no products, so the bound has a unit to spare
    accumulate   one more term, (R + 3) 2^-23 (A + |old|): `old` enters with its own magnitude, and the sum that is added to it
                 carries the error of its R terms into an addition more; ref is old + sum
dxs is moe_gemm_ref's bwd_x with its gate.  None of the bounds depends on a summation order."""
import numpy as np

import moe_gemm_ref as g
from moe_gemm_ref import EPS_MM, FLOOR, U, clamp_offsets, make, make_ints, offsets_of, ranges, round_to  # noqa: F401  (re-exported)


def as_nk(w, layout):
    """w of either layout -> [E, N, K]"""
    assert layout in ("nk", "kn")
    w = np.asarray(w)
    return w if layout == "nk" else w.transpose(0, 2, 1)


def to_layout(w_nk, layout):
    return w_nk if layout == "nk" else np.ascontiguousarray(np.asarray(w_nk).transpose(0, 2, 1))


def rows_of(offsets, S):
    """[S] the expert of each row, -1 outside every expert"""
    e_of = np.full(S, -1, np.int64)
    for e, lo, hi in ranges(offsets, S):
        e_of[lo:hi] = e
    return e_of


# ---- the four formulas -----------------------------------------------------------------------------------------------------------------
def linear_ref(xs, w, offsets, bias=None, layout="nk"):
    """-> (ys [S, N] fp64, A [S, N] = sum_c |xs W|, B [S, N] = |bias| of the row's expert, 0 outside);  R = K"""
    ys, A = g.gemm_ref(xs, as_nk(w, layout), offsets)
    B = np.zeros_like(ys)
    if bias is not None:
        bias = np.asarray(bias, np.float64)
        for e, lo, hi in ranges(offsets, ys.shape[0]):
            ys[lo:hi] += bias[e]
            B[lo:hi] = np.abs(bias[e])
    return ys, A, B


def bwd_x_ref(dys, w, offsets, layout="nk"):
    return g.bwd_x_ref(dys, as_nk(w, layout), offsets)


def bwd_w_ref(dys, xs, offsets, layout="nk"):
    """-> (dw fp64 in the layout, A likewise, R [E, 1, 1])"""
    dw, A, R = g.bwd_w_ref(dys, xs, offsets)
    return to_layout(dw, layout), to_layout(A, layout), R


def bwd_b_ref(dys, offsets):
    """-> (db [E, N] fp64, A = sum |dys|, R [E, 1])"""
    dys = np.asarray(dys, np.float64)
    E = np.asarray(offsets).size - 1
    db, A, R = np.zeros((E, dys.shape[1])), np.zeros((E, dys.shape[1])), np.zeros((E, 1))
    for e, lo, hi in ranges(offsets, dys.shape[0]):
        db[e], A[e], R[e] = dys[lo:hi].sum(0), np.abs(dys[lo:hi]).sum(0), hi - lo
    return db, A, R


# ---- the gates: |got - ref| / tolerance per element, <= 1 passes ----------------------------------------------------------------------
def fwd_tol(ref, A, B, K, dt):
    return U[dt] * np.abs(ref) + (K + 3) * EPS_MM * (np.asarray(A, np.float64) + np.asarray(B, np.float64)) + FLOOR[dt]


def grad_tol(ref, A, R, gdt, old=None):
    """dw and db; `old`: what the gradient was added to (ref = old + sum)"""
    R, A = np.asarray(R, np.float64), np.asarray(A, np.float64)
    t = U[gdt] * np.abs(ref) + (R + 2) * EPS_MM * A + FLOOR[gdt]
    if old is not None:
        t = t + (R + 3) * EPS_MM * (A + np.abs(np.asarray(old, np.float64)))
    return t


def _ratios(got, ref, t):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    t = np.broadcast_to(t, ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / t)
    r = np.where(np.isnan(got) & np.isnan(ref), 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def fwd_ratios(got, ref, A, B, K, dt):
    return _ratios(got, ref, fwd_tol(np.asarray(ref, np.float64), A, B, K, dt))


def grad_ratios(got, ref, A, R, gdt, old=None):
    return _ratios(got, ref, grad_tol(np.asarray(ref, np.float64), A, R, gdt, old))


def worst(r):
    return float(r.max()) if r.size else 0.0


# ---- fp32 evaluations on the CPU (the host tests hold the gates against them, and against wrong ones) -----------------------------------
def linear_f32(xs, w, offsets, dt, bias=None, layout="nk", order="blas", short=0, bias_mode="ok"):
    """the forward in fp32, the bias added in fp32, rounded once to dt.  bias_mode: "ok", "omit" (a kernel that forgets it), "next" (one
    that adds the bias of expert e + 1)"""
    xs, w = np.asarray(xs, np.float32), np.asarray(as_nk(w, layout), np.float32)
    ys = np.zeros((xs.shape[0], w.shape[1]), np.float32)
    for e, lo, hi in ranges(offsets, xs.shape[0]):
        acc = g._dot_f32(xs[lo:hi], w[e], order, short)
        if bias is not None and bias_mode != "omit":
            b = np.asarray(bias, np.float32)[(e + (bias_mode == "next")) % w.shape[0]]
            acc = (acc + b).astype(np.float32)
        ys[lo:hi] = acc
    return round_to(ys, dt)


def bwd_w_f32(dys, xs, offsets, gdt, layout="nk", order="blas", short=0, old=None, old_mode="ok"):
    """dw in fp32, rounded once to gdt; old_mode: "ok", "omit" (old is overwritten), "twice" (old is added twice)"""
    dys, xs = np.asarray(dys, np.float32), np.asarray(xs, np.float32)
    E = np.asarray(offsets).size - 1
    dw = np.zeros((E, dys.shape[1], xs.shape[1]), np.float32)
    for e, lo, hi in ranges(offsets, dys.shape[0]):
        if hi - lo > short:
            dw[e] = g._dot_f32(dys[lo:hi].T, xs[lo:hi].T, order, short)
    return _add_old(to_layout(dw, layout), offsets, dys.shape[0], gdt, old, old_mode)


def bwd_b_f32(dys, offsets, gdt, order="blas", short=0, old=None, old_mode="ok"):
    dys = np.asarray(dys, np.float32)
    E = np.asarray(offsets).size - 1
    db = np.zeros((E, dys.shape[1]), np.float32)
    for e, lo, hi in ranges(offsets, dys.shape[0]):
        rows = dys[lo:hi - short] if hi - lo > short else dys[lo:lo]
        db[e] = rows.sum(0, dtype=np.float32) if order == "blas" else (np.cumsum(rows, 0, dtype=np.float32)[-1] if len(rows) else 0)
    return _add_old(db, offsets, dys.shape[0], gdt, old, old_mode)


def _add_old(new, offsets, S, gdt, old, old_mode):
    if old is None:
        return round_to(new, gdt)
    old32 = np.asarray(old, np.float32)
    out = old32.copy()
    for e, _, _ in ranges(offsets, S):                                           # an expert without rows keeps what it holds
        times = {"ok": 1, "omit": 0, "twice": 2}[old_mode]
        out[e] = (np.float32(times) * old32[e] + new[e]).astype(np.float32)
    return round_to(out, gdt)
