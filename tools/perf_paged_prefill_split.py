"""Time split-KV prefill attention over a paged KV cache (nnop_paged_prefill_split, the sixteenth library) against the unsplit call
(nnop_paged_prefill, the thirteenth library, which this work leaves as it was) on the same inputs.

    python tools/perf_paged_prefill_split.py [--out profiles/r14/paged_prefill_split.jsonl] [--only llama] [--shapes short|bind|spec|full]

bf16, the Llama-3-70B (QH 64, KH 8, E 128) and gpt-oss-120b (QH 64, KH 8, E 64, sinks) head shapes, pages of 16 in the vLLM layout with a
shuffled table whose max_pages page_size is the context.  Shapes:

    short   chunks of 64, 128 and 512 new tokens behind 8192, 32768 and 131072 keys, B = 1
    bind    64 new tokens behind 1024, 2048 and 4096 keys, B = 1: contexts short enough for the least chunk of the automatic rule to bind
    spec    B = 8 sequences of 24 new tokens behind 32768 keys: speculative verification
    full    a chunk of 2048 behind 32768 and a pure prefill of 8 x 2048: the automatic rule resolves to one split here, and the ratio
            shows the run-to-run spread of two calls of the same kernel

Arms: `base`, paged_prefill_attention_into; `auto`, paged_prefill_attention_split_into with the library's automatic count; and
`mct4`, `mct8`, `mct16`, the count the automatic rule would give with a least chunk of 4, 8 or 16 tiles, forced -- wherever that count
differs from the arms already there.  The method is tools/perf_paged_prefill.py's: the arms alternate in one process, per repeat
`--iters` back-to-back calls between HIP events, `--reps` >= 10 repeats after `--warmup` untimed calls; the split arms bring their
workspace.  Before timing, every arm's last 8 tokens of sequence 0 are held against an fp64 softmax under the bf16 gate of tests/util.py.
One JSON line per shape: the resolved counts, the workspace bytes, microseconds (median, min, max) and TFLOP/s of the arms, and
base / arm with the spread of that ratio over the paired repeats.  Pass 1 and the merge are one timed interval: not separated here.
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
SHAPES = {"short": tuple((1, n, c) for c in (8192, 32768, 131072) for n in (64, 128, 512)),
          "bind": ((1, 64, 1024), (1, 64, 2048), (1, 64, 4096)), "spec": ((8, 24, 32768),),
          "full": ((1, 2048, 32768), (8, 2048, 0))}                                                        # (B, new, prefix)
PAGE, TAIL = 16, 8


def rule(T, B, G, KH, cap, least):
    """the automatic count of include/nnop_hip_paged_prefill_split.h with `least` tiles a chunk, no window"""
    groups = KH * (T // (128 // G) + B)
    return max(1, min(-(-512 // groups), -(-cap // 32) // least, 64))


def inside_gate(o_tail, q_tail, k, v, sinks):
    """the last TAIL tokens of sequence 0, o_tail and q_tail [TAIL, QH, E], against fp64 on its dense keys k, v [KH, L, E]; worst error / gate"""
    (KH, L, E), worst = k.shape, 0.0
    G = q_tail.shape[1] // KH
    seen = torch.arange(L, device=k.device)[None] <= (L - TAIL + torch.arange(TAIL, device=k.device))[:, None]
    for h in range(KH):
        x = torch.einsum("tge,je->gtj", q_tail[:, h * G:(h + 1) * G].double(), k[h].double()) / E ** 0.5
        x = x.masked_fill(~seen, float("-inf"))
        if sinks is not None:
            x = torch.cat([x, sinks[h * G:(h + 1) * G].double()[:, None, None].expand(-1, TAIL, 1)], -1)
        ref = torch.einsum("gtj,je->tge", torch.softmax(x, -1)[..., :L], v[h].double())
        tol = ATOL_FRAC["bf16"] * ref.abs().max() + RTOL["bf16"] * ref.abs()
        worst = max(worst, float(((o_tail[:, h * G:(h + 1) * G].double() - ref).abs() / tol).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the model name")
    ap.add_argument("--shapes", default="", help="short, bind, spec or full; all by default")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev, dt = "cuda", torch.bfloat16
    lines = []
    for (name, QH, KH, E, has_sink), (kind, (B, n, c)) in ((m, (a, s)) for m in MODELS for a in SHAPES for s in SHAPES[a]):
        if args.only not in name or args.shapes not in kind:
            continue
        L, pages = c + n, -(-(c + n) // PAGE)
        torch.manual_seed(B + L)
        q = torch.randn(B * n, QH, E, device=dev).to(dt)
        k, v = (torch.randn(B, KH, pages * PAGE, E, device=dev).to(dt) for _ in range(2))
        table = torch.randperm(B * pages, device=dev).to(torch.int32).view(B, pages)
        pools = []
        for t in (k, v):
            pool = torch.empty(B * pages, PAGE, KH, E, dtype=dt, device=dev)
            pool[table.long()] = t.view(B, KH, pages, PAGE, E).permute(0, 2, 3, 1, 4)
            pools.append(pool)
        kp, vp = (p.transpose(1, 2) for p in pools)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        sinks = torch.randn(QH, device=dev) if has_sink else None
        auto = pkg.paged_prefill_attention_split_plan(q, kp, vp, table)[0]
        counts = {"auto": auto}
        for least in (4, 8, 16):
            s = rule(B * n, B, QH // KH, KH, pages * PAGE, least)
            if s not in counts.values():
                counts[f"mct{least}"] = s
        nbytes = {a: pkg.paged_prefill_attention_split_plan(q, kp, vp, table, num_splits=s)[1] for a, s in counts.items()}
        ws = torch.empty(max(nbytes.values()) // 4 + 1, dtype=torch.float32, device=dev)
        outs = {a: torch.empty_like(q) for a in ("base", *counts)}
        arms = {"base": lambda: pkg.paged_prefill_attention_into(outs["base"], None, q, kp, vp, table, cu, lens, sinks=sinks)}
        for a, s in counts.items():
            arms[a] = lambda a=a, s=s: pkg.paged_prefill_attention_split_into(outs[a], None, q, kp, vp, table, cu, lens, sinks=sinks,
                                                                               num_splits=s, workspace=ws)
        gates = {}
        for a, f in arms.items():
            f()
            gates[a] = inside_gate(outs[a][n - TAIL:n], q[n - TAIL:n], k[0, :, :L], v[0, :, :L], sinks)
        assert max(gates.values()) <= 1.0, f"{name} {kind} B{B} n{n} c{c}: an arm is outside the gate: {gates}"
        t = time_arms(arms, args.warmup, args.iters, args.reps)
        med = {a: statistics.median(x) for a, x in t.items()}
        flops = 4 * E * QH * B * (n * c + n * (n + 1) // 2)
        rec = {"shape": f"{name} bf16 {kind} B{B} new{n} prefix{c} QH{QH} KH{KH} E{E} page{PAGE}", "reps": args.reps, "iters": args.iters,
               "baseline": "paged_prefill_attention_into, the unsplit call", "groups_unsplit": KH * (B * n // (128 // (QH // KH)) + B),
               "splits": counts, "workspace_bytes": nbytes, "error_over_gate": {a: round(g, 4) for a, g in gates.items()}, "flops": flops,
               **{a: {"us_median": round(med[a], 1), "us_min": round(min(x), 1), "us_max": round(max(x), 1),
                      "tflops": round(flops / med[a] / 1e6, 1)} for a, x in t.items()}}
        for a in counts:
            ratios = [b / s for b, s in zip(t["base"], t[a])]
            rec[f"base_over_{a}"] = [round(med["base"] / med[a], 3), round(min(ratios), 3), round(max(ratios), 3)]   # of medians, min, max
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del k, v, pools, kp, vp, q, outs, ws
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
