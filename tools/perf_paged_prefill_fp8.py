"""Time prefill attention over a paged FP8 (E4M3) KV cache (nnop_paged_prefill_fp8, the fifteenth library) against the two things a caller
has without it.

    python tools/perf_paged_prefill_fp8.py [--out profiles/r13/paged_prefill_fp8.jsonl] [--only llama]

bf16 queries, the Llama-3-70B (QH 64, KH 8, E 128) and gpt-oss-120b (QH 64, KH 8, E 64) head shapes, pages of 16 in the vLLM layout with
a shuffled table, a scale per KV head that is no power of two; tools/perf_paged_prefill.py's shapes: 512 and 2048 new tokens behind
prefixes of 8192 and 32768 (B = 1), and the no-prefix shapes 8 x 2048 and 2 x 8192.  Three arms alternate in one process:

    fp8      paged_prefill_attention_fp8_into on the E4M3 pool
    bf16     paged_prefill_attention_into on a bf16 pool that holds the same values (code value x scale): (a), what the staging path costs
             or saves beside the 16-bit kernel, which is its own text behind the staging
    gather   the visible codes gathered through the table and dequantised into a bf16 pool of their own, then paged_prefill_attention_into
             on that: (b), what a caller with an E4M3 pool does today
    bf16_b   the bf16 arm once more: the ratio bf16_b / bf16 is the spread of the 16-bit call against itself, which (a) is read against

The method is tools/perf_paged_attn.py's: per repeat `--iters` back-to-back calls between device events and a synchronise, `--reps` >= 10
repeats after `--warmup` untimed calls of every arm.  Before timing, the fp8 arm's last 64 tokens of sequence 0 are held against an fp64
softmax on the dequantised keys under the bf16 gate of tests/util.py.  One JSON line per shape: microseconds (median, min, max) of the
arms, and bf16 / fp8, gather / fp8 and bf16_b / bf16 with the min and max of each ratio over the paired repeats.  Fails without a GPU.
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
from perf_paged_prefill import PAGE, TAIL, inside_gate  # noqa: E402

MODELS = (("llama-3-70b", 64, 8, 128), ("gpt-oss-120b", 64, 8, 64))
SHAPES = ((1, 512, 8192), (1, 2048, 8192), (1, 512, 32768), (1, 2048, 32768), (8, 2048, 0), (2, 8192, 0))   # (B, new, prefix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the model name")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"
    assert torch.cuda.is_available(), "this tool times kernels: it needs a GPU"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev, dt, f8 = "cuda", torch.bfloat16, torch.float8_e4m3fn
    lines = []
    for (name, QH, KH, E), (B, n, c) in ((m, s) for m in MODELS for s in SHAPES):
        if args.only not in name:
            continue
        L, pages = c + n, (c + n) // PAGE
        torch.manual_seed(B + L)
        q = torch.randn(B * n, QH, E, device=dev).to(dt)
        ks, vs = (torch.linspace(lo, 2 * lo, KH, device=dev) for lo in (0.75, 0.013))
        table = torch.randperm(B * pages, device=dev).to(torch.int32).view(B, pages)
        pools8, pools16, dense = [], [], []
        for s in (ks, vs):
            codes = (torch.randn(B, KH, L, E, device=dev) / s[None, :, None, None]).to(f8)
            pool = torch.empty(B * pages, PAGE, KH, E, dtype=f8, device=dev)
            pool.view(torch.uint8)[table.long()] = codes.view(torch.uint8).view(B, KH, pages, PAGE, E).permute(0, 2, 3, 1, 4)
            pools8.append(pool)
            pools16.append((pool.float() * s[None, None, :, None]).to(dt))      # the same values, each rounded once to bf16
            dense.append(codes[0].float() * s[:, None, None])                   # sequence 0's keys for the gate
            del codes
        kp8, vp8 = (p.transpose(1, 2) for p in pools8)
        kp16, vp16 = (p.transpose(1, 2) for p in pools16)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        ident = torch.arange(B * pages, dtype=torch.int32, device=dev).view(B, pages)      # the gathered pool lies in table order
        o = torch.empty_like(q)
        fp8 = lambda: pkg.paged_prefill_attention_fp8_into(o, None, q, kp8, vp8, table, cu, lens, k_scale=ks, v_scale=vs)
        bf16 = lambda: pkg.paged_prefill_attention_into(o, None, q, kp16, vp16, table, cu, lens)

        def gather():                                                           # gather, dequantise, then the 16-bit call
            kg, vg = ((p.view(torch.uint8)[table.long()].view(f8).float() * s[None, None, None, :, None]).to(dt).view(B * pages, PAGE, KH, E).transpose(1, 2)
                      for p, s in ((pools8[0], ks), (pools8[1], vs)))
            return pkg.paged_prefill_attention_into(o, None, q, kg, vg, ident, cu, lens)
        gate = inside_gate(fp8()[n - TAIL:n], q[n - TAIL:n], dense[0], dense[1], None)
        assert gate <= 1.0, f"{name} B{B} n{n} c{c}: the fp8 arm is outside the gate: {gate}"
        assert torch.equal(gather()[n - TAIL:n].clone(), bf16()[n - TAIL:n]), "the gather arm does not compute what the bf16 arm computes"
        t = time_arms({"bf16": bf16, "fp8": fp8, "gather": gather, "bf16_b": bf16}, args.warmup, args.iters, args.reps)
        med = {a: statistics.median(x) for a, x in t.items()}
        rec = {"shape": f"{name} bf16 B{B} new{n} prefix{c} QH{QH} KH{KH} E{E} page{PAGE}", "reps": args.reps, "iters": args.iters,
               "error_over_gate": round(gate, 4),
               **{a: {"us_median": round(med[a], 1), "us_min": round(min(x), 1), "us_max": round(max(x), 1)} for a, x in t.items()}}
        for key, (num, den) in (("bf16_over_fp8", ("bf16", "fp8")), ("gather_over_fp8", ("gather", "fp8")), ("bf16_b_over_bf16", ("bf16_b", "bf16"))):
            ratios = [a / b for a, b in zip(t[num], t[den])]
            rec[key] = {"median": round(med[num] / med[den], 3), "min": round(min(ratios), 3), "max": round(max(ratios), 3)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del pools8, pools16, dense, kp8, vp8, kp16, vp16, q, o
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
