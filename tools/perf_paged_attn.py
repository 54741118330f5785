"""Time decode attention over a paged KV cache (nnop_paged_attn, the twelfth library) against the dense call (nnop_decode_attn, the tenth)
on the same keys gathered into a dense cache: what reading the pages where they lie costs beside a cache that is already dense -- the
copy a caller with a paged pool had to make per step before is not timed.

    python tools/perf_paged_attn.py [--out profiles/r10/paged_attn.jsonl] [--only llama]

The shapes are tools/perf_decode_attn_fp8.py's with 128 MiB or more of visible K + V: bf16 queries; gpt-oss-120b (QH 64, KH 8, E 64,
sinks) and Llama-3-70B (QH 64, KH 8, E 128), dense; B = 1, 8, 64; every sequence as long as its table.  Arms:

    paged16    paged_decode_attention_into on a [P, 16, KH, E] pool (the vLLM layout) with a shuffled table: every 16 keys elsewhere
    paged128   the same keys in pages of 128
    dense      decode_attention_into on those keys gathered into [B, KH, L, E]; the same splits and workspace

The method is that tool's: the arms alternate in one process, per repeat `--iters` back-to-back calls between HIP events, `--reps` >= 10
repeats after `--warmup` untimed calls; each arm rotates over two copies of its cache so that L2 does not hold it.  Before timing the
dense arm is held against an fp64 softmax over sequence 0 under the bf16 gate of tests/util.py and each paged arm against the dense
arm's bits.  One JSON line per shape: microseconds (median, min, max) of the arms, the visible K + V bytes over the median in TB/s,
dense / paged with the spread of that ratio over the paired repeats, and whether the paged median lies inside the dense arm's spread.
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

from perf_decode_attn import BATCHES, LENGTHS, MODELS, inside_gate  # noqa: E402
from perf_moe_gemm import time_arms  # noqa: E402

PAGES = (16, 128)
MIN_VISIBLE = 128 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the model name")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev, dt = "cuda", torch.bfloat16
    lines = []
    for (name, QH, KH, E, window, has_sink), B, L in ((m, b, n) for m in MODELS for n in LENGTHS for b in BATCHES):
        visible = 2 * B * KH * L * E * 2
        if args.only not in name or window is not None or visible < MIN_VISIBLE or (L == 65536 and B > 8):
            continue
        torch.manual_seed(B + L)
        q = torch.randn(B, QH, 1, E, device=dev).to(dt)
        dense = [tuple(torch.randn(B, KH, L, E, device=dev).to(dt) for _ in range(2)) for _ in range(2)]
        paged = {}
        for page in PAGES:                               # the same keys, every page somewhere else in a pool of exactly B L / page pages
            n = L // page
            paged[page] = []
            for kv in dense:
                table = torch.randperm(B * n, device=dev).to(torch.int32).view(B, n)
                pools = []
                for t in kv:
                    pool = torch.empty(B * n, page, KH, E, dtype=dt, device=dev)
                    pool[table.long()] = t.view(B, KH, n, page, E).permute(0, 2, 3, 1, 4)
                    pools.append(pool.transpose(1, 2))
                paged[page].append((*pools, table))
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        sinks = torch.randn(QH, device=dev) if has_sink else None
        splits, nbytes = pkg.decode_attention_plan(q, *dense[0])
        assert all((splits, nbytes) == pkg.paged_decode_attention_plan(q, *paged[p][0]) for p in PAGES)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        o, turn = torch.empty_like(q), {}

        def nxt(arm, caches, i):
            turn[arm] = turn.get(arm, 0) + (i is None)
            return caches[turn[arm] % 2 if i is None else i]

        def dense_arm(i=None):
            k, v = nxt("dense", dense, i)
            return pkg.decode_attention_into(o, None, q, k, v, lens, sinks=sinks, workspace=ws)

        def paged_arm(page):
            def arm(i=None):
                k, v, table = nxt(page, paged[page], i)
                return pkg.paged_decode_attention_into(o, None, q, k, v, table, lens, sinks=sinks, workspace=ws)
            return arm

        arms = {"dense": dense_arm, **{f"paged{p}": paged_arm(p) for p in PAGES}}
        want = dense_arm(0).clone()
        gate = inside_gate(want, q, *dense[0], 0, L, sinks)
        assert gate <= 1.0, f"{name} B{B} L{L}: the dense arm is outside the gate: {gate}"
        for p in PAGES:
            assert torch.equal(arms[f"paged{p}"](0), want), f"{name} B{B} L{L}: page size {p} does not give the dense call's bits"
        t = time_arms(arms, args.warmup, args.iters, args.reps)
        med = {n: statistics.median(v) for n, v in t.items()}
        rec = {"shape": f"{name} bf16 B{B} L{L} QH{QH} KH{KH} E{E}", "reps": args.reps, "iters": args.iters, "splits": splits,
               "visible_kv_bytes": visible, "dense_error_over_gate": round(gate, 4)}
        for n, v in t.items():
            rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                      "tb_per_s": round(visible / med[n] / 1e6, 3)}
            if n != "dense":                             # the arms alternate: repeat r of one stands beside repeat r of the other
                ratios = [d / x for d, x in zip(t["dense"], v)]
                rec[n].update(dense_over_paged=round(med["dense"] / med[n], 3), dense_over_paged_min=round(min(ratios), 3),
                              dense_over_paged_max=round(max(ratios), 3), median_inside_dense_spread=min(t["dense"]) <= med[n] <= max(t["dense"]))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del dense, paged
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
