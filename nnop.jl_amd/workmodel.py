"""Algorithmic work of one call: the FLOPs / bytes that bench.py and the perf tools divide by the
measured time.  Pure arithmetic on shapes; part of the product so that measurement code never needs the test oracle."""
from __future__ import annotations

__all__ = ["attention_flops", "attention_bytes", "rope_bytes", "softmax_bytes", "norm_bytes", "add_norm_bytes", "glu_bytes", "xent_bytes",
           "qknr_bytes"]


def attention_flops(E, QL, KL, QH, B, *, causal: bool, mode: str = "fwd", kv_lens=None):
    """fwd non-causal 4*E*QL*KL*QH*B; causal counts the visible (query, key) pairs; with kv_lens (key padding) the key
    count per batch is sum(len_b); bwd = 2.5x fwd; fwd+bwd = 3.5x fwd."""
    if kv_lens is not None:
        f = 4 * E * QH * QL * int(sum(int(x) for x in kv_lens))
    elif causal:
        n = min(QL, KL)
        pairs = n * (n + 1) // 2 + max(QL - KL, 0) * KL
        f = 4 * E * QH * B * pairs
    else:
        f = 4 * E * QL * KL * QH * B
    return {"fwd": f, "bwd": f * 5 // 2, "fwd+bwd": f * 7 // 2}[mode]


def attention_bytes(E, QL, KL, QH, KH, B, itemsize, *, mode: str = "fwd"):
    """Every tensor touched once: fwd reads q, k, v and writes o, ms, ls; bwd reads q, k, v, o, dO, ms, ls and writes
    dq, dk, dv."""
    nq, nk, st = B * QH * QL * E, B * KH * KL * E, 2 * B * QH * QL
    fwd = itemsize * (nq + 2 * nk + nq + st)
    bwd = itemsize * (nq + 2 * nk + nq + nq + nq + 2 * nk + st)
    return {"fwd": fwd, "bwd": bwd, "fwd+bwd": fwd + bwd}[mode]


def rope_bytes(D, L, QH, KH, B, itemsize):
    """q and k read once and written once, the D/2-wide cos / sin rows (fp32) read once."""
    return 2 * itemsize * B * L * D * (QH + KH) + 2 * 4 * B * L * (D // 2)


def softmax_bytes(N, batch, itemsize, bwd=False):
    """forward reads x and writes y; pullback reads dy, y and writes dx."""
    return (3 if bwd else 2) * N * batch * itemsize


def norm_bytes(emb, n, itemsize, bwd=False):
    """forward reads x, writes y; pullback reads dy, x, writes dx (w, b, statistics are O(emb + n))."""
    return (3 if bwd else 2) * emb * n * itemsize


def add_norm_bytes(emb, n, itemsize, bwd=False):
    """residual add fused into the norm: forward reads x, residual and writes h, y; pullback (with dh) reads dy, h, dh and
    writes dx -- four row-sized arrays either way."""
    return 4 * emb * n * itemsize


def glu_bytes(n, rows, itemsize, bwd=False):
    """gated activation y = act(gate) * up: forward reads gate, up and writes y; pullback reads dy, gate, up and writes dgate, dup."""
    return (5 if bwd else 3) * n * rows * itemsize


def xent_bytes(n, rows, itemsize, index_bytes=8, bwd=False):
    """cross-entropy over rows of n logits: forward reads the logits and the targets and writes loss and lse (8 bytes per row);
    pullback reads the logits, the targets, dloss and lse and writes dlogits."""
    return (2 if bwd else 1) * n * rows * itemsize + 8 * rows + index_bytes * rows


def qknr_bytes(D, L, QH, KH, B, itemsize, *, cs_itemsize=4, w_itemsize=4, bwd=False, n_parts=0):
    """fused QK-norm + RoPE: forward reads q, k and writes q', k' -- 2 (|q| + |k|) -- plus the tables: the D/2-wide cos / sin
    rows and the two weights, read once; pullback reads dq', dk', q, k and writes dq, dk -- 3 (|q| + |k|) -- plus the tables, dwq
    and dwk (fp32), and the `n_parts` fp32 partial rows per tensor, written once and read once by the fold."""
    qk = itemsize * B * L * D * (QH + KH)
    tables = 2 * cs_itemsize * B * L * (D // 2) + 2 * w_itemsize * D
    if not bwd:
        return 2 * qk + tables
    return 3 * qk + tables + 2 * 4 * D + 2 * 2 * n_parts * 4 * D
