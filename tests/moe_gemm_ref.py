"""Reference of the grouped expert GEMM (include/nnop_hip_moe_gemm.h) and the gates its tests use (test infrastructure, not a test file).

The header's three formulas in fp64 numpy, evaluated on the ROUNDED inputs (the arrays as the device sees them).  Every offset is clamped
into [0, S]; expert e owns the rows lo_e = offsets[e] <= s < hi_e = offsets[e+1], none where hi_e <= lo_e; rows outside every expert are
zero, and so is dw of an expert without rows.

The gate is derived, not calibrated.  u is the unit roundoff of the output type (f32 2^-24, f16 2^-11, bf16 2^-8), R the reduction length
(K for the forward, N for bwd_x, the expert's row count for bwd_w), A the same sum over absolute values, floor = FLOOR[dt] of
moe_data_ref (half the subnormal spacing of the type):
    |got - ref| <= u |ref| + (R + 2) 2^-23 A + floor
The middle term is the any-order bound of an R-term fp32 sum of products (R - 1 additions, one rounding per product, one unit of slack
for the second-order terms), so neither a summation order nor the order inside a matrix core can fail it.  It is taken at 2^-23, not
2^-24: the rounding mode of the adder inside the matrix core is not documented, and a chopping adder has that roundoff.  A NaN pattern
that differs from the reference's is an infinite error, as in moe_data_ref._ratio."""
import numpy as np

from moe_data_ref import FLOOR, TORCH_DT, U, exact, round_to  # noqa: F401  (re-exported for the tests)

EPS_MM = 2.0 ** -23


def clamp_offsets(offsets, S):
    return np.clip(np.asarray(offsets).astype(np.int64), 0, S)


def ranges(offsets, S):
    """[(e, lo, hi)] of the experts that own rows"""
    off = clamp_offsets(offsets, S)
    return [(e, int(off[e]), int(off[e + 1])) for e in range(off.size - 1) if off[e + 1] > off[e]]


def offsets_of(counts, lead=0):
    """[E+1] int32 from per-expert row counts; `lead` rows in front of the first expert"""
    return np.concatenate([[lead], lead + np.cumsum(counts)]).astype(np.int32)


# ---- the three formulas ----------------------------------------------------------------------------------------------------------------
def gemm_ref(xs, w, offsets):
    """-> (ys [S, N] fp64, A [S, N] = sum_c |xs w|);  R = K"""
    xs, w = np.asarray(xs, np.float64), np.asarray(w, np.float64)
    ys, A = np.zeros((xs.shape[0], w.shape[1])), np.zeros((xs.shape[0], w.shape[1]))
    for e, lo, hi in ranges(offsets, xs.shape[0]):
        ys[lo:hi] = xs[lo:hi] @ w[e].T
        A[lo:hi] = np.abs(xs[lo:hi]) @ np.abs(w[e]).T
    return ys, A


def bwd_x_ref(dys, w, offsets):
    """-> (dxs [S, K] fp64, A);  R = N"""
    dys, w = np.asarray(dys, np.float64), np.asarray(w, np.float64)
    dxs, A = np.zeros((dys.shape[0], w.shape[2])), np.zeros((dys.shape[0], w.shape[2]))
    for e, lo, hi in ranges(offsets, dys.shape[0]):
        dxs[lo:hi] = dys[lo:hi] @ w[e]
        A[lo:hi] = np.abs(dys[lo:hi]) @ np.abs(w[e])
    return dxs, A


def bwd_w_ref(dys, xs, offsets):
    """-> (dw [E, N, K] fp64, A, R [E, 1, 1] = the experts' row counts)"""
    dys, xs = np.asarray(dys, np.float64), np.asarray(xs, np.float64)
    E = np.asarray(offsets).size - 1
    dw, A, R = np.zeros((E, dys.shape[1], xs.shape[1])), np.zeros((E, dys.shape[1], xs.shape[1])), np.zeros((E, 1, 1))
    for e, lo, hi in ranges(offsets, dys.shape[0]):
        dw[e] = dys[lo:hi].T @ xs[lo:hi]
        A[e] = np.abs(dys[lo:hi]).T @ np.abs(xs[lo:hi])
        R[e] = hi - lo
    return dw, A, R


# ---- the gate: |got - ref| / tolerance per element, <= 1 passes ----------------------------------------------------------------------
def tol(ref, A, R, dt):
    return U[dt] * np.abs(np.asarray(ref, np.float64)) + (np.asarray(R, np.float64) + 2) * EPS_MM * np.asarray(A, np.float64) + FLOOR[dt]


def ratios(got, ref, A, R, dt):
    """element-wise |got - ref| / tol; inf where exactly one of the two is NaN, 0 where both are"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    t = np.broadcast_to(tol(ref, A, R, dt), ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / t)
    r = np.where(np.isnan(got) & np.isnan(ref), 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def ratio(got, ref, A, R, dt):
    r = ratios(got, ref, A, R, dt)
    return float(r.max()) if r.size else 0.0


# ---- fp32 evaluations on the CPU (the host tests hold the gate against them) ----------------------------------------------------------
def _dot_f32(a, b, order, short=0):
    """a [M, R] b [P, R]^T in fp32: BLAS order, or one sequential chain over r; `short` = 8: the last 8 terms are left out"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    R = a.shape[1] - short
    if order == "blas":
        return (a[:, :R] @ b[:, :R].T).astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for r in range(R):
        acc = (acc + (a[:, r, None] * b[None, :, r]).astype(np.float32)).astype(np.float32)
    return acc


def gemm_f32(xs, w, offsets, dt, order="blas", short=0, shift=0):
    """the forward in fp32, rounded once to dt; shift = 1: expert e uses the weights of expert e + 1 (a wrong kernel)"""
    xs, w = np.asarray(xs, np.float32), np.asarray(w, np.float32)
    ys = np.zeros((xs.shape[0], w.shape[1]), np.float32)
    for e, lo, hi in ranges(offsets, xs.shape[0]):
        ys[lo:hi] = _dot_f32(xs[lo:hi], w[(e + shift) % w.shape[0]], order, short)
    return round_to(ys, dt)


def bwd_x_f32(dys, w, offsets, dt, order="blas", short=0, shift=0):
    dys, w = np.asarray(dys, np.float32), np.asarray(w, np.float32)
    dxs = np.zeros((dys.shape[0], w.shape[2]), np.float32)
    for e, lo, hi in ranges(offsets, dys.shape[0]):
        dxs[lo:hi] = _dot_f32(dys[lo:hi], w[(e + shift) % w.shape[0]].T, order, short)
    return round_to(dxs, dt)


def bwd_w_f32(dys, xs, offsets, dt, order="blas", short=0, shift=0):
    """shift = 1: expert e sums the rows of expert e + 1"""
    dys, xs = np.asarray(dys, np.float32), np.asarray(xs, np.float32)
    E = np.asarray(offsets).size - 1
    dw = np.zeros((E, dys.shape[1], xs.shape[1]), np.float32)
    own = {e: (lo, hi) for e, lo, hi in ranges(offsets, dys.shape[0])}
    for e in own:
        lo, hi = own.get((e + shift) % E, (0, 0)) if shift else own[e]
        if hi - lo > short:
            dw[e] = _dot_f32(dys[lo:hi].T, xs[lo:hi].T, order, short)
    return round_to(dw, dt)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make(seed, shape, dt, ld=None, scale=1.0):
    """N(0, scale^2) values rounded to dt, as fp32 numpy of shape[:-1] + (ld,); the padding columns hold 7.0"""
    rng = np.random.default_rng(seed)
    a = np.full(tuple(shape[:-1]) + (ld or shape[-1],), 7.0, np.float32)
    a[..., :shape[-1]] = round_to((scale * rng.standard_normal(shape)).astype(np.float32), dt)
    return a


def make_ints(seed, shape, lo=-2, hi=2):
    """integers in [lo, hi] as fp32: exact in every type, and so is every product sum the exact-data tests build from them"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32)
