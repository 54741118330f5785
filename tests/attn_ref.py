"""The attention reference of the tests, for every per-call option at once (test infrastructure, not a test file).

flash_attention's options (include/nnop_hip.h: nnop_fa_opts, nnop_fa_fwd_sinks, nnop_fa_fwd_softcap) are lowered ONCE to an additive
[B][KL][QL][QH] bias and handed to the fp64 oracle (oracle.naive_attention) with causal=False and no mask, so the oracle the whole
suite is judged against is also the reference of every option and of every combination of them:

  visibility  a window (left, right) -- flash-attn's `window_size`, -1 = unbounded side -- lets query i see key j iff
                  (left < 0 or j >= i - left) and (right < 0 or j <= i + right)
              on top of the causal rule and the key padding, top-left aligned whatever QL and KL are: a bias of 0 / -inf.
  pair        the user's bias is added as it is.
  softcap     with scale = 1/sqrt(E) and a cap c > 0:  s = scale q.k,  z = c tanh(s / c),  x = z + pair, masked.  The cap becomes the
              extra bias z - s (s and z in fp64).  The oracle's (o, ms, ls, dv) are then the capped ones and the dpair it returns
              is dS, the gradient with respect to x.  Its own dq / dk differentiate the linear s only, so they are recomputed through
              the tanh:  dS' = dS (1 - tanh^2(s / c)),  dq = scale dS' K,  dk = scale dS'^T Q  (summed over the GQA group).
  sinks       sigma_h joins every row's softmax as one more column with no value vector: one more KEY at index KL with k = v = 0
              whose bias is sigma_h for every row (its logit is scale q.0 + sigma_h, it adds nothing to o, it is never capped).
              dsigma_h is that column's dpair summed over (batch, row).

A row is DEAD when it sees no key and its head has no sink (no sinks, or sigma_h = -inf).  Forward: what the formula gives, NaN
in o (0 / 0) and ms = -inf.  Gradients: the library's convention (deviation 3), dq = 0 and no contribution
to dk, dv, dpair, dsinks.  Dead rows are given every key and a zero cotangent, which is exactly that (P finite, dP = delta = 0 ->
dS = 0), instead of the NaN the naive formula spreads over the whole (batch, kv-head).

Below the reference: the one input generator and the one parity check of the window / sinks / softcap GPU tests.
"""
import zlib

import numpy as np
import torch

from oracle.naive_attention import naive_attention, naive_attention_grads
from util import TORCH_DT, assert_close, to64


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
    bias = np.where(window_keep(QL, KL, window, causal), 0.0, -np.inf)           # [QL, KL]
    return np.ascontiguousarray(np.broadcast_to(bias.T[None, :, :, None], (B, KL, QL, QH)))


def _visible(B, QL, KL, causal, kpad_mask, window):
    """bool [B, QL, KL]: window, causal rule and key padding together"""
    vis = np.broadcast_to(window_keep(QL, KL, window, causal)[None], (B, QL, KL))
    return vis if kpad_mask is None else vis & np.asarray(kpad_mask, bool)[:, None, :]


def dead_rows(q, k, *, causal, kpad_mask=None, window=None, sinks=None):
    """bool [B, QH, QL]: query rows that see no key and whose head has no sink."""
    B, QH, QL, _ = q.shape
    dead = ~_visible(B, QL, k.shape[2], causal, kpad_mask, window).any(axis=-1)
    dead = np.broadcast_to(dead[:, None, :], (B, QH, QL))
    return dead if sinks is None else dead & np.isneginf(np.asarray(sinks, np.float64))[None, :, None]


def cap_terms(q, k, c):
    """s [B, QH, QL, KL] (fp64, scaled), tanh(s / c), K repeated over the GQA group"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    ke = np.repeat(k, q.shape[1] // k.shape[1], axis=1)
    s = np.einsum("bhie,bhje->bhij", q, ke) / np.sqrt(q.shape[-1])
    return s, np.tanh(s / c), ke


def _lower(q, k, v, pair, causal, kpad_mask, window, sinks, softcap, opened=None):
    """(q, k, v, bias) for the oracle (k, v, bias one key longer with sinks) and the cap's (tanh, repeated K) or None.
    `opened` [B, QH, QL]: rows that see every key whatever the visibility says."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    B, QH, QL, E = q.shape
    KH, KL = k.shape[1], k.shape[2]
    vis = np.broadcast_to(_visible(B, QL, KL, causal, kpad_mask, window)[:, None], (B, QH, QL, KL))
    if opened is not None:
        vis = vis | opened[..., None]
    bias = np.transpose(np.where(vis, 0.0, -np.inf), (0, 3, 2, 1))               # [B, KL, QL, QH]
    user = None if pair is None else np.asarray(pair, np.float64)
    cap = None
    if softcap is not None:
        s, t, ke = cap_terms(q, k, softcap)
        adj = np.ascontiguousarray(np.transpose(softcap * t - s, (0, 3, 2, 1)))
        user = adj if user is None else adj + user
        cap = (t, ke)
    if user is not None:
        bias = user + bias
    if sinks is not None:
        z = np.zeros((B, KH, 1, E))
        k, v = np.concatenate([k, z], axis=2), np.concatenate([v, z], axis=2)
        col = np.broadcast_to(np.asarray(sinks, np.float64)[None, None, None, :], (B, 1, QL, QH))
        bias = np.concatenate([bias, col], axis=1)
    return q, k, v, bias, cap


def attention_fwd(q, k, v, pair=None, *, causal, kpad_mask=None, window=None, sinks=None, softcap=None):
    """(o, ms, ls) of the naive formula under the options (fp64).  Dead rows: NaN in o, ms = -inf."""
    q, k, v, bias, _ = _lower(q, k, v, pair, causal, kpad_mask, window, sinks, softcap)
    return naive_attention(q, k, v, bias, causal=False, return_stats=True)


def attention_grads(q, k, v, dO, pair=None, *, causal, kpad_mask=None, window=None, sinks=None, softcap=None):
    """(dq, dk, dv, dpair|None[, dsinks]) of the naive formula under the options (fp64), with the dead-row convention above."""
    KH, KL = np.asarray(k).shape[1:3]
    dead = dead_rows(np.asarray(q), np.asarray(k), causal=causal, kpad_mask=kpad_mask, window=window, sinks=sinks)
    dO = np.where(dead[..., None], 0.0, np.asarray(dO, np.float64))
    q, k1, v1, bias, cap = _lower(q, k, v, pair, causal, kpad_mask, window, sinks, softcap, opened=dead)
    dq, dk, dv, dS = naive_attention_grads(q, k1, v1, dO, bias, causal=False)
    if sinks is not None:
        dsinks = dS[:, KL].sum(axis=(0, 1))                                      # [B, QL, QH] -> [QH]
        dk, dv, dS = dk[:, :, :KL], dv[:, :, :KL], np.ascontiguousarray(dS[:, :KL])
    if cap is not None:
        t, ke = cap
        B, QH, QL, E = q.shape
        scale = 1.0 / np.sqrt(E)
        dSc = np.transpose(dS, (0, 3, 2, 1)) * (1.0 - t * t)                     # [B, QH, QL, KL], through the tanh
        dq = scale * np.einsum("bhij,bhje->bhie", dSc, ke)
        dk = scale * np.einsum("bhij,bhie->bhje", dSc, q).reshape(B, KH, QH // KH, -1, E).sum(axis=2)
    out = (dq, dk, dv, (dS if pair is not None else None))
    return out + (dsinks,) if sinks is not None else out


# ---- the GPU tests' inputs and parity check --------------------------------------------------------------------------------------
INF = float("inf")
MIX = [-INF, -30.0, 0.0, 3.0, 30.0]


def inputs(key, B, QH, KH, QL, KL, E, dt, dev, pair=False, pad=False, qscale=1.0, sinks=None):
    """N(0,1) inputs keyed by `key`, rounded to bf16 first so that every dtype sees the same values; q times `qscale` (a power of
    two: exact in every dtype).  sinks: None, the fp32 values per head, or "mix": MIX cycled over the heads from a start that
    depends on the key."""
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32)).to(torch.bfloat16).to(TORCH_DT[dt]).to(dev)
    d = dict(q=mk(B, QH, QL, E) * qscale, k=mk(B, KH, KL, E), v=mk(B, KH, KL, E), do=mk(B, QH, QL, E))
    d["pair"] = mk(B, KL, QL, QH) if pair else None
    d["mask"] = None
    if pad:
        lens = rng.integers(max(1, KL // 3), KL + 1, size=B)
        d["mask"] = torch.tensor(np.arange(KL)[None, :] < lens[:, None]).to(dev)
    if sinks is not None:
        s = [MIX[(i + len(repr(key))) % len(MIX)] for i in range(QH)] if isinstance(sinks, str) else sinks
        d["sinks"] = torch.tensor(s, dtype=torch.float32, device=dev)
    return d


def run(pkg, d, causal, **opts):
    """(o, ms, ls, dq, dk, dv, dpair|None[, dsinks]) of the library on the inputs `d` under opts (window, sinks, softcap)"""
    q, k, v, pair = d["q"], d["k"], d["v"], d["pair"]
    fwd = pkg._flash_attention(q, k, v, pair, causal=causal, kpad_mask=d["mask"], **opts)
    grads = pkg.grad_flash_attention(d["do"], *fwd, q, k, v, pair, causal=causal, kpad_mask=d["mask"], **opts)
    torch.cuda.synchronize()
    return tuple(fwd) + tuple(grads)


def check_parity(pkg, d, dt, causal, *, window=None, sinks=None, softcap=None, label=""):
    """The library against the reference above, the same gates under every option; returns what run() returns."""
    out = run(pkg, d, causal, window=window, sinks=sinks, softcap=softcap)
    o, ms, ls, dq, dk, dv, dp = out[:7]
    q, k, v, do, pair = (to64(d[n]) for n in ("q", "k", "v", "do", "pair"))
    kw = dict(causal=causal, kpad_mask=None if d["mask"] is None else d["mask"].cpu().numpy(), window=window, sinks=to64(sinks))
    o_ref, ms_ref, ls_ref = attention_fwd(q, k, v, pair, softcap=softcap, **kw)
    ref = attention_grads(q, k, v, do, pair, softcap=softcap, **kw)
    dead = dead_rows(q, k, **kw)
    live = ~dead
    assert np.isnan(to64(o)[dead]).all() and np.isneginf(to64(ms)[dead]).all()
    assert_close(label + "o", o, o_ref, dt, floor=True)
    assert_close(label + "ms", to64(ms)[live], ms_ref[live], dt, floor=True)
    assert_close(label + "ls", to64(ls)[live], ls_ref[live], dt, 2.0, floor=True)
    sc = 1.0 if dt == "f32" else 2.0
    assert (to64(dq)[dead] == 0).all()
    for name, got, want in zip(("dq", "dk", "dv"), (dq, dk, dv), ref):
        assert_close(label + name, got, want, dt, sc, floor=True, kind="grad")
    if pair is not None:
        assert_close(label + "dpair", dp, ref[3], dt, sc, floor=True, kind="grad")
        outside = ~window_keep(q.shape[2], k.shape[2], window, causal).T         # [KL, QL]
        assert (to64(dp)[:, outside, :] == 0).all()
    if sinks is not None:
        assert_close(label + "dsinks", out[7], ref[4], dt, sc, floor=True, kind="grad")
        assert (to64(out[7])[np.isneginf(kw["sinks"])] == 0).all()
    return out
