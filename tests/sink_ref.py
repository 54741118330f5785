"""Learned attention sink reference for the tests (test infrastructure, not a test file).

A sink sigma_h joins every row's softmax as one more column with no value vector (include/nnop_hip.h, nnop_fa_fwd_sinks).  Here
it becomes one more KEY at index KL with k = 0, v = 0 whose pair bias is sigma_h for every row: its logit is scale * q.0 + sigma_h
= sigma_h and it adds nothing to o.  What the real keys can see (causal rule, window, key padding) becomes a 0 / -inf bias, as in
tests/window_ref.py, plus the user's pair; the oracle then runs with causal=False and no mask.  So the fp64 oracle the whole suite
is judged against (oracle.naive_attention) is also the sinks' reference: its (o, ms, ls) are the sink semantics, dsigma_h is the
sum over (batch, row) of the sink column's dpair.

Heads with sigma = -inf whose rows see no key give NaN here, as such rows do today; compare those with window_ref's dead-row
convention (window_fwd / window_grads).
"""
import numpy as np

from oracle.naive_attention import naive_attention, naive_attention_grads
from window_ref import window_keep


def _extend(q, k, v, pair, sinks, causal, kpad_mask, window):
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    B, QH, QL, E = q.shape
    KH, KL = k.shape[1], k.shape[2]
    z = np.zeros((B, KH, 1, E))
    k1, v1 = np.concatenate([k, z], axis=2), np.concatenate([v, z], axis=2)
    vis = np.broadcast_to(window_keep(QL, KL, window, causal)[None], (B, QL, KL))
    if kpad_mask is not None:
        vis = vis & np.asarray(kpad_mask, bool)[:, None, :]
    bias = np.empty((B, KL + 1, QL, QH))
    bias[:, :KL] = np.where(vis, 0.0, -np.inf).transpose(0, 2, 1)[..., None]
    if pair is not None:
        bias[:, :KL] += np.asarray(pair, np.float64)
    bias[:, KL] = np.asarray(sinks, np.float64)[None, None, :]
    return q, k1, v1, bias


def sink_fwd(q, k, v, sinks, pair=None, *, causal, kpad_mask=None, window=None):
    """(o, ms, ls) with sinks (fp64)."""
    q, k1, v1, bias = _extend(q, k, v, pair, sinks, causal, kpad_mask, window)
    return naive_attention(q, k1, v1, bias, causal=False, return_stats=True)


def sink_grads(q, k, v, dO, sinks, pair=None, *, causal, kpad_mask=None, window=None):
    """(dq, dk, dv, dpair|None, dsinks) with sinks (fp64)."""
    KL = np.asarray(k).shape[2]
    q, k1, v1, bias = _extend(q, k, v, pair, sinks, causal, kpad_mask, window)
    dq, dk, dv, dp = naive_attention_grads(q, k1, v1, np.asarray(dO, np.float64), bias, causal=False)
    dsinks = dp[:, KL].sum(axis=(0, 1))                      # [B, QL, QH] -> [QH]
    return dq, dk[:, :, :KL], dv[:, :, :KL], (np.ascontiguousarray(dp[:, :KL]) if pair is not None else None), dsinks
