"""Time prefill attention over a paged KV cache (nnop_paged_prefill, the thirteenth library) against what a caller has without it.

    python tools/perf_paged_prefill.py [--out profiles/r11/paged_prefill.jsonl] [--only llama] [--arm pure|chunked]

bf16, the Llama-3-70B (QH 64, KH 8, E 128) and gpt-oss-120b (QH 64, KH 8, E 64, sinks) head shapes, pages of 16 in the vLLM layout with a
shuffled table.  Arms:

    pure      prefix 0, uniform lengths 2048 (B = 8) and 8192 (B = 2): paged_prefill_attention_into beside flash_attention(causal=True)
              on the same keys held dense [B, KH, L, E] -- the project's own forward, which needs no table and no packing
    chunked   512 and 2048 new tokens over prefixes of 8192 and 32768, B = 1: beside torch's scaled_dot_product_attention on the keys
              gathered through the table with an explicit mask, the gather included -- what a caller with pages must do today.  torch
              has no sink, so the gpt-oss shape runs without one here

The method is tools/perf_paged_attn.py's: the arms alternate in one process, per repeat `--iters` back-to-back calls between HIP events,
`--reps` >= 10 repeats after `--warmup` untimed calls.  Before timing each arm's last 64 tokens of sequence 0 are held against an fp64
softmax under the bf16 gate of tests/util.py.  One JSON line per shape: microseconds (median, min, max) and TFLOP/s (4 E QH visible
(query, key) pairs over the median) of the arms, baseline / paged with the spread of that ratio over the paired repeats.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from perf_moe_gemm import time_arms  # noqa: E402
from util import ATOL_FRAC, RTOL  # noqa: E402

MODELS = (("llama-3-70b", 64, 8, 128, False), ("gpt-oss-120b", 64, 8, 64, True))
SHAPES = {"pure": ((8, 2048, 0), (2, 8192, 0)), "chunked": ((1, 512, 8192), (1, 2048, 8192), (1, 512, 32768), (1, 2048, 32768))}   # (B, new, prefix)
PAGE, TAIL = 16, 64


def inside_gate(o_tail, q_tail, k, v, sinks):
    """the last TAIL tokens of sequence 0, o_tail and q_tail [TAIL, QH, E], against fp64 on its dense keys k, v [KH, L, E]; worst error / gate"""
    G, L = q_tail.shape[1] // k.shape[0], k.shape[1]
    kk, vv = (t.double().repeat_interleave(G, 0) for t in (k, v))
    x = torch.einsum("the,hje->htj", q_tail.double(), kk) / q_tail.shape[-1] ** 0.5
    seen = torch.arange(L, device=k.device)[None] <= (L - TAIL + torch.arange(TAIL, device=k.device))[:, None]
    x = x.masked_fill(~seen, float("-inf"))
    if sinks is not None:
        x = torch.cat([x, sinks.double()[:, None, None].expand(-1, TAIL, 1)], -1)
    ref = torch.einsum("htj,hje->the", torch.softmax(x, -1)[..., :L], vv)
    tol = ATOL_FRAC["bf16"] * ref.abs().max() + RTOL["bf16"] * ref.abs()
    return float(((o_tail.double() - ref).abs() / tol).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the model name")
    ap.add_argument("--arm", default="", help="pure or chunked; both by default")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev, dt = "cuda", torch.bfloat16
    lines = []
    for (name, QH, KH, E, has_sink), (arm, (B, n, c)) in ((m, (a, s)) for m in MODELS for a in SHAPES for s in SHAPES[a]):
        if args.only not in name or args.arm not in arm:
            continue
        L, pages = c + n, (c + n) // PAGE
        torch.manual_seed(B + L)
        q = torch.randn(B * n, QH, E, device=dev).to(dt)
        k, v = (torch.randn(B, KH, L, E, device=dev).to(dt) for _ in range(2))
        table = torch.randperm(B * pages, device=dev).to(torch.int32).view(B, pages)
        pools = []
        for t in (k, v):
            pool = torch.empty(B * pages, PAGE, KH, E, dtype=dt, device=dev)
            pool[table.long()] = t.view(B, KH, pages, PAGE, E).permute(0, 2, 3, 1, 4)
            pools.append(pool)
        kp, vp = (p.transpose(1, 2) for p in pools)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        sinks = torch.randn(QH, device=dev) if has_sink and arm == "pure" else None
        o = torch.empty_like(q)
        paged = lambda: pkg.paged_prefill_attention_into(o, None, q, kp, vp, table, cu, lens, sinks=sinks)
        if arm == "pure":
            qd = q.view(B, n, QH, E).transpose(1, 2).contiguous()            # [B, QH, L, E], made once: the dense forward's own layout

            def base():
                with torch.no_grad():
                    return pkg.flash_attention(qd, k, v, causal=True, sinks=sinks)
            tail = lambda r: r[0, :, -TAIL:].transpose(0, 1)
        else:
            mask = torch.arange(L, device=dev)[None] <= (c + torch.arange(n, device=dev))[:, None]

            def base():                                                      # the gather, then torch's attention with the mask
                kd, vd = (p[table.long()].permute(0, 3, 1, 2, 4).reshape(B, KH, L, E) for p in pools)
                return torch.nn.functional.scaled_dot_product_attention(q.view(B, n, QH, E).transpose(1, 2), kd, vd, attn_mask=mask, enable_gqa=True)
            tail = lambda r: r[0, :, -TAIL:].transpose(0, 1)
        gates = {"paged": inside_gate(paged()[n - TAIL:n], q[n - TAIL:n], k[0], v[0], sinks),
                 "base": inside_gate(tail(base()), q[n - TAIL:n], k[0], v[0], sinks)}
        assert max(gates.values()) <= 1.0, f"{name} {arm} B{B} n{n} c{c}: an arm is outside the gate: {gates}"
        t = time_arms({"base": base, "paged": paged}, args.warmup, args.iters, args.reps)
        med = {a: statistics.median(x) for a, x in t.items()}
        flops = 4 * E * QH * B * (n * c + n * (n + 1) // 2)
        ratios = [b / p for b, p in zip(t["base"], t["paged"])]
        rec = {"shape": f"{name} bf16 {arm} B{B} new{n} prefix{c} QH{QH} KH{KH} E{E} page{PAGE}", "reps": args.reps, "iters": args.iters,
               "baseline": "flash_attention(causal=True), dense keys" if arm == "pure" else "gather + torch SDPA with a mask",
               "error_over_gate": {a: round(g, 4) for a, g in gates.items()}, "flops": flops,
               **{a: {"us_median": round(med[a], 1), "us_min": round(min(x), 1), "us_max": round(max(x), 1),
                      "tflops": round(flops / med[a] / 1e6, 1)} for a, x in t.items()},
               "base_over_paged": round(med["base"] / med["paged"], 3), "base_over_paged_min": round(min(ratios), 3),
               "base_over_paged_max": round(max(ratios), 3)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del k, v, pools, kp, vp, q, o
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
