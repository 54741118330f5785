"""Reference of the mixture-of-experts gate and dispatch plan (include/nnop_hip_moe.h) and the gates their GPU tests use (test
infrastructure, not a test file).

The header's formulas in fp64 numpy, evaluated on the ROUNDED inputs (the logits as the device sees them).  Selection is a lexicographic
sort on (is-NaN, value, -index): NaN first, then the larger value, then the lower expert index, with -0 == +0.  The plan is a stable
argsort of the flat assignment ids by expert with the skip rule for entries outside [0, E)."""
import numpy as np

from test_softmax_gpu import GTOL, TOL          # the project's softmax gates (importing the module touches no GPU)

W_RTOL, W_ATOL = TOL["f32"]["rtol"], 1e-7       # w is fp32 whatever the logits are; 1e-7: one fp32 ulp of the largest weight
NORMS = ("topk", "all")


def select(x, k):
    """x [T, E] -> idx [T, k] int32, in selection order"""
    x = np.asarray(x, np.float64)
    nan = np.isnan(x)
    v = np.where(nan, 0.0, x) + 0.0                                  # -0 + 0 = +0
    cols = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    order = np.lexsort((cols, -v, ~nan), axis=-1)                    # the last key is the primary one; False (a NaN) sorts first
    return order[:, :k].astype(np.int32)


def router_ref(x, k, norm):
    """-> (w [T, k], idx [T, k] int32, lse [T]) in fp64; a row whose formulas give NaN in IEEE arithmetic has NaN weights"""
    x = np.asarray(x, np.float64)
    idx = select(x, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=-1, keepdims=True)                            # NaN if the row holds one
        lse = (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[:, 0]
        xs = np.take_along_axis(x, idx.astype(np.int64), axis=-1)
        if norm == "topk":
            e = np.exp(xs - xs[:, :1])
            w = e / e.sum(axis=-1, keepdims=True)
        else:
            w = np.exp(xs - lse[:, None])
    return w, idx, lse


def router_grad_ref(dw, x, k, norm, dlse=None):
    """dlogits [T, E] in fp64 from the cotangents dw [T, k] and dlse [T] (or None), everything else recomputed from x"""
    x, dw = np.asarray(x, np.float64), np.asarray(dw, np.float64)
    w, idx, lse = router_ref(x, k, norm)
    S = (w * dw).sum(axis=-1, keepdims=True)
    c = np.zeros((x.shape[0], 1)) if dlse is None else np.asarray(dlse, np.float64)[:, None]
    if norm == "topk":
        sel = w * (dw - S)
    else:
        sel, c = w * dw, c - S
    dl = np.zeros_like(x) if (norm == "topk" and dlse is None) else c * np.exp(x - lse[:, None])
    np.add.at(dl, (np.arange(x.shape[0])[:, None], idx.astype(np.int64)), sel)
    return dl


def plan_ref(idx, E):
    """-> (counts [E], offsets [E + 1], perm [T k], slot like idx), int32"""
    idx = np.asarray(idx)
    flat = idx.reshape(-1).astype(np.int64)
    valid = (flat >= 0) & (flat < E)
    order = np.argsort(np.where(valid, flat, E), kind="stable")
    n = int(valid.sum())
    perm = np.full(flat.size, -1, np.int32)
    perm[:n] = order[:n]
    slot = np.full(flat.size, -1, np.int32)
    slot[order[:n]] = np.arange(n, dtype=np.int32)
    counts = np.bincount(flat[valid], minlength=E).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return counts, offsets, perm, slot.reshape(idx.shape)


# ---- gates: worst |got - ref| / tolerance, <= 1 passes; a NaN pattern that differs, or an infinity, is inf -----------------------------
def _ratio(got, ref, atol, rtol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    atol = np.broadcast_to(atol, ref.shape)[ok]
    got, ref = got[ok], ref[ok]
    same = got == ref                                                # (equal infinities)
    with np.errstate(invalid="ignore"):
        r = np.where(same, 0.0, np.abs(got - ref) / (atol + rtol * np.abs(ref)))
    return float("inf") if np.isnan(r).any() else float(r.max())


def w_ratio(got, ref):
    return _ratio(got, ref, W_ATOL, W_RTOL)


def lse_ratio(got, ref):
    ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        atol = 2e-6 * np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 1.0)))
    return _ratio(got, ref, atol, W_RTOL)


def dl_ratio(got, ref, dt):
    """dlogits: GTOL of tests/test_softmax_gpu.py, atol scaled by max(1, max|ref|)"""
    ref = np.asarray(ref, np.float64)
    fin = ref[np.isfinite(ref)]
    return _ratio(got, ref, GTOL[dt]["atol"] * max(1.0, float(np.abs(fin).max()) if fin.size else 1.0), GTOL[dt]["rtol"])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_logits(seed, T, E, ld=None):
    """fp32 numpy [T, ld] ~ N(0, 3^2); the padding columns E ... ld-1 hold 1e30 (reading one would change every result)"""
    rng = np.random.default_rng(seed)
    x = np.full((T, ld or E), 1e30, np.float32)
    x[:, :E] = 3.0 * rng.standard_normal((T, E))
    return x
