"""Logit soft-capping reference for the tests (test infrastructure, not a test file).

With scale = 1/sqrt(E) and a cap c > 0 (include/nnop_hip.h, nnop_fa_fwd_softcap):
    s = scale q.k      z = c tanh(s / c)      x = z + pair, masked      P = softmax(x [, the sink])      o = P v
Here the cap becomes an additive bias: x = s + (pair + (z - s)), with s and z computed in fp64, so the fp64 oracle the whole suite is
judged against (oracle.naive_attention, through tests/window_ref.py and tests/sink_ref.py for windows, dead rows and sinks) is also the
cap's reference.  Its (o, ms, ls, dv) are the capped ones and the dpair it returns is dS, the gradient with respect to x.  The
oracle's own dq / dk differentiate the linear s only, so they are recomputed here through the tanh:
    dS' = dS (1 - tanh^2(s / c))      dq = scale dS' K      dk = scale dS'^T Q  (summed over the GQA group)

The inputs and case lists of tests/test_softcap_gpu.py live here too, so that the CPU tests (tests/test_softcap_host.py) can check on
the very same inputs that the cap changes the result by much more than the parity tolerance.
"""
import zlib

import numpy as np
import torch

from sink_ref import sink_fwd, sink_grads
from window_ref import window_fwd, window_grads


def _terms(q, k, c):
    """s [B, QH, QL, KL] (fp64, scaled), tanh(s / c), K repeated over the GQA group"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    rep = q.shape[1] // k.shape[1]
    ke = np.repeat(k, rep, axis=1)
    s = np.einsum("bhie,bhje->bhij", q, ke) / np.sqrt(q.shape[-1])
    return s, np.tanh(s / c), ke


def _total_pair(s, t, c, pair):
    adj = np.ascontiguousarray(np.transpose(c * t - s, (0, 3, 2, 1)))          # [B, KL, QL, QH]
    return adj if pair is None else adj + np.asarray(pair, np.float64)


def softcap_fwd(q, k, v, pair=None, *, softcap, causal, kpad_mask=None, window=None, sinks=None):
    """(o, ms, ls) of the capped formula (fp64).  Rows that see no key (and no sink): NaN in o, ms = -inf."""
    s, t, _ = _terms(q, k, softcap)
    tot = _total_pair(s, t, softcap, pair)
    if sinks is not None:
        return sink_fwd(q, k, v, sinks, tot, causal=causal, kpad_mask=kpad_mask, window=window)
    return window_fwd(q, k, v, tot, causal=causal, kpad_mask=kpad_mask, window=window)


def softcap_grads(q, k, v, dO, pair=None, *, softcap, causal, kpad_mask=None, window=None, sinks=None):
    """(dq, dk, dv, dpair|None[, dsinks]) of the capped formula (fp64), with window_ref's convention for rows that see no key."""
    s, t, ke = _terms(q, k, softcap)
    tot = _total_pair(s, t, softcap, pair)
    if sinks is not None:
        _, _, dv, dS, dsinks = sink_grads(q, k, v, dO, sinks, tot, causal=causal, kpad_mask=kpad_mask, window=window)
    else:
        _, _, dv, dS = window_grads(q, k, v, dO, tot, causal=causal, kpad_mask=kpad_mask, window=window)
    q = np.asarray(q, np.float64)
    B, QH, QL, E = q.shape
    KH = np.asarray(k).shape[1]
    scale = 1.0 / np.sqrt(E)
    dSc = np.transpose(dS, (0, 3, 2, 1)) * (1.0 - t * t)                         # [B, QH, QL, KL], through the tanh
    dq = scale * np.einsum("bhij,bhje->bhie", dSc, ke)
    dk = scale * np.einsum("bhij,bhie->bhje", dSc, q).reshape(B, KH, QH // KH, -1, E).sum(axis=2)
    out = (dq, dk, dv, (dS if pair is not None else None))
    return out + (dsinks,) if sinks is not None else out


# ---- inputs and cases of the GPU tests -------------------------------------------------------------------------------------------
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def inputs(key, B, QH, KH, QL, KL, E, dt, dev, pair=False, pad=False, qscale=1.0):
    """N(0,1) inputs, rounded to bf16 first so that every dtype sees the same values (as tests/test_window_gpu.py makes them);
    q times `qscale` (a power of two: exact in every dtype)."""
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32)).to(torch.bfloat16).to(TORCH_DT[dt]).to(dev)
    d = dict(q=mk(B, QH, QL, E) * qscale, k=mk(B, KH, KL, E), v=mk(B, KH, KL, E), do=mk(B, QH, QL, E))
    d["pair"] = mk(B, KL, QL, QH) if pair else None
    d["mask"] = None
    if pad:
        lens = rng.integers(max(1, KL // 3), KL + 1, size=B)
        d["mask"] = torch.tensor(np.arange(KL)[None, :] < lens[:, None]).to(dev)
    return d


DTYPES = ["f32", "bf16", "f16"]
EMBS = [16, 32, 64, 128, 256, 8]                 # 8: the plain-HIP kernels
CAPS = [0.5, 1.0, 2.0]
LENS = [(63, 65), (65, 63), (517, 517), (1, 63), (300, 1100)]


def parity_grid():
    """every E meets every dtype and both causal settings; caps and lengths cycle over the grid (as test_window_gpu._grid prunes).
    Cases: (dt, E, causal, QL, KL, cap)."""
    out = []
    i = 0
    for E in EMBS:
        for dt in DTYPES:
            for causal in (False, True):
                QL, KL = LENS[(i + EMBS.index(E)) % len(LENS)]
                if E >= 128 and QL * KL > 600 * 600:
                    QL, KL = (QL // 2 + 1, KL // 2 + 1)          # the window grid's rule (none of LENS is that large today)
                out.append((dt, E, causal, QL, KL, CAPS[i % len(CAPS)]))
                i += 1
    return out


def grid_inputs(case, dev):
    dt, E, causal, QL, KL, cap = case
    return inputs(case, 1, 2, 1, QL, KL, E, dt, dev)


# realistic cap: scores of std 8 (q x 8) under c = 30.  fp32 only: at row maxima of 25 .. 40 a bf16 ms is rounded by up to 0.0625
# (0.125 past 32) and ls is stored relative to the ROUNDED ms, so ls alone is up to 6.6 % (13 %) off the exact row's while
# ms + log(ls) is right to 6e-3.  Measured on an MI355X on these very inputs, the unchanged ls gate is missed by the capped call
# (err / tol 1.37 at E = 64, 1.35 at E = 128) and equally by the uncapped one (1.21, 1.29); o, ms, dq, dk, dv are inside their
# gates (err / tol <= 0.24) either way (tools/measure_softcap_realistic.py, profiles/r05/softcap_realistic.txt).  It is the
# residual format, not the cap: DESIGN.md section 4.4d.
REALISTIC = [("f32", E, 130, 517, 30.0) for E in (64, 128)]


def realistic_inputs(case, dev):
    dt, E, QL, KL, cap = case
    return inputs(("real",) + case, 1, 2, 1, QL, KL, E, dt, dev, qscale=8.0)
