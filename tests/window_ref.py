"""Sliding-window (local) attention reference for the tests (test infrastructure, not a test file).

A window (left, right) -- flash-attn's `window_size`, -1 = unbounded side -- lets query i see key j iff
    (left < 0 or j >= i - left) and (right < 0 or j <= i + right)
on top of the causal rule and the key padding, top-left aligned whatever QL and KL are.  Here it becomes an additive
[B][KL][QL][QH] bias of 0 / -inf that is handed to the existing fp64 oracle (oracle.naive_attention), so the oracle the whole
suite is judged against is also the window's reference.
"""
import numpy as np

from oracle.naive_attention import naive_attention, naive_attention_grads


def window_keep(QL, KL, window, causal=False):
    """bool [QL, KL]: which key each query sees by the window and the causal rule (key padding aside)."""
    i = np.arange(QL)[:, None]
    j = np.arange(KL)[None, :]
    keep = np.ones((QL, KL), dtype=bool)
    if window is not None:
        left, right = window
        if left >= 0:
            keep &= j >= i - left
        if right >= 0:
            keep &= j <= i + right
    if causal:
        keep &= j <= i
    return keep


def window_bias(B, QL, KL, QH, window, causal=False):
    """The window (and causal rule) as an additive pair bias [B][KL][QL][QH]: 0 where a query sees a key, -inf elsewhere."""
    keep = window_keep(QL, KL, window, causal)
    bias = np.where(keep, 0.0, -np.inf)                      # [QL, KL]
    return np.ascontiguousarray(np.broadcast_to(bias.T[None, :, :, None], (B, KL, QL, QH)))


def _total_pair(q, k, pair, window, causal):
    B, QH, QL, _ = q.shape
    KL = k.shape[2]
    bias = window_bias(B, QL, KL, QH, window, causal)
    return bias if pair is None else np.asarray(pair, np.float64) + bias


def window_fwd(q, k, v, pair=None, *, causal, kpad_mask=None, window):
    """(o, ms, ls) of the naive formula under the window (fp64).  Rows that see no key: NaN in o (0 / 0), ms = -inf."""
    tot = _total_pair(q, k, pair, window, False)
    return naive_attention(q, k, v, tot, causal=causal, kpad_mask=kpad_mask, return_stats=True)


def dead_rows(q, k, *, causal, kpad_mask=None, window):
    """bool [B, QH, QL]: query rows that see no key at all."""
    B, QH, QL, _ = q.shape
    KL = k.shape[2]
    keep = window_keep(QL, KL, window, causal)[None]          # [1, QL, KL]
    if kpad_mask is not None:
        keep = keep & np.asarray(kpad_mask, bool)[:, None, :]
    else:
        keep = np.broadcast_to(keep, (B, QL, KL))
    return np.broadcast_to(~keep.any(axis=-1)[:, None, :], (B, QH, QL))


def window_grads(q, k, v, dO, pair=None, *, causal, kpad_mask=None, window):
    """(dq, dk, dv, dpair|None) of the naive formula under the window (fp64), with the library's convention for rows that see
    no key (deviation 3): dq = 0 and no contribution to dk, dv, dpair.  Such rows are given every key and a
    zero cotangent here, which is exactly that (P finite, dP = delta = 0 -> dS = 0), instead of the NaN the naive formula
    spreads over the whole (batch, kv-head)."""
    q, k, v, dO = (np.asarray(x, np.float64) for x in (q, k, v, dO))
    B, QH, QL, _ = q.shape
    KL = k.shape[2]
    dead = dead_rows(q, k, causal=causal, kpad_mask=kpad_mask, window=window)
    keep = window_keep(QL, KL, window, causal)
    mask = np.ones((B, KL), bool) if kpad_mask is None else np.asarray(kpad_mask, bool)
    # [B, QH, QL, KL]: visible pairs; dead rows see everything (and carry no cotangent)
    vis = keep[None, None] & mask[:, None, None, :]
    vis = vis | dead[..., None]
    bias = np.transpose(np.where(vis, 0.0, -np.inf), (0, 3, 2, 1))            # [B, KL, QL, QH]
    tot = bias if pair is None else np.asarray(pair, np.float64) + bias
    dO = np.where(dead[..., None], 0.0, dO)
    dq, dk, dv, dp = naive_attention_grads(q, k, v, dO, tot, causal=False, kpad_mask=None)
    return dq, dk, dv, (dp if pair is not None else None)
