"""Time decode attention over an E4M3 KV cache (nnop_decode_attn_fp8, the eleventh library) against the 16-bit call (nnop_decode_attn, the
tenth) on the same cache dequantised to bf16: what the 8-bit cache buys a decode step, in the same process.

    python tools/perf_decode_attn_fp8.py [--out profiles/r09/decode_attn_fp8.jsonl] [--only llama]

The shapes are tools/perf_decode_attn.py's: bf16 queries; gpt-oss-120b (QH 64, KH 8, E 64, sinks) dense and with its window of 128,
Llama-3-70B (QH 64, KH 8, E 128) dense; B = 1, 8, 64; every sequence as long as its cache, 1024, 8192 and (up to B = 8) 65536 keys.  Arms:

    fp8        decode_attention_fp8_into on the E4M3 cache with a scale per KV head, automatic splits, caller-owned workspace
    bf16       decode_attention_into on that cache times its scales, rounded to bf16; the same splits and workspace

The method is that tool's: the arms alternate in one process, per repeat `--iters` back-to-back calls between HIP events, `--reps` >= 10
repeats after `--warmup` untimed calls; each arm rotates over two copies of its cache so that L2 does not hold it.  Before timing each
arm is held against an fp64 softmax over the visible keys of sequence 0 of ITS cache under the bf16 gate of tests/util.py.  One JSON line
per shape: microseconds (median, min, max) of both arms, the visible K + V bytes of each and those bytes over the median in TB/s,
bf16 / fp8 with the spread of that ratio over the repeats, and whether fp8's median lies below bf16's fastest repeat.
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
        if args.only not in name or (L == 65536 and B > 8):
            continue
        torch.manual_seed(B + L)
        q = torch.randn(B, QH, 1, E, device=dev).to(dt)
        ks, vs = (torch.linspace(0.6, 1.7, KH, device=dev), torch.linspace(1.3, 0.4, KH, device=dev))
        c8 = [tuple((torch.randn(B, KH, L, E, device=dev) / s[None, :, None, None]).to(torch.float8_e4m3fn) for s in (ks, vs)) for _ in range(2)]
        c16 = [tuple((c.float() * s[None, :, None, None]).to(dt) for c, s in zip(kv, (ks, vs))) for kv in c8]
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        sinks = torch.randn(QH, device=dev) if has_sink else None
        lo = 0 if window is None else max(0, L - 1 - window)
        splits, nbytes = pkg.decode_attention_fp8_plan(q, *c8[0], window_left=window)
        assert (splits, nbytes) == pkg.decode_attention_plan(q, *c16[0], window_left=window)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        o, turn = torch.empty_like(q), {"fp8": 0, "bf16": 0}

        def nxt(arm, caches, i):
            turn[arm] += i is None
            return caches[turn[arm] % 2 if i is None else i]

        def fp8(i=None):
            k, v = nxt("fp8", c8, i)
            return pkg.decode_attention_fp8_into(o, None, q, k, v, lens, k_scale=ks, v_scale=vs, window_left=window, sinks=sinks, workspace=ws)

        def bf16(i=None):
            k, v = nxt("bf16", c16, i)
            return pkg.decode_attention_into(o, None, q, k, v, lens, window_left=window, sinks=sinks, workspace=ws)

        deq = tuple(c[:1].double() * s.double()[None, :, None, None] for c, s in zip(c8[0], (ks, vs)))
        gate = {"fp8": inside_gate(fp8(0), q, *deq, lo, L, sinks), "bf16": inside_gate(bf16(0), q, *c16[0], lo, L, sinks)}
        assert max(gate.values()) <= 1.0, f"{name} B{B} L{L}: outside the gate: {gate}"
        t = time_arms({"fp8": fp8, "bf16": bf16}, args.warmup, args.iters, args.reps)
        med = {n: statistics.median(v) for n, v in t.items()}
        ratios = [b / f for b, f in zip(t["bf16"], t["fp8"])]                # the arms alternate: repeat r of one stands beside repeat r of the other
        visible = {"fp8": 2 * B * KH * (L - lo) * E, "bf16": 2 * B * KH * (L - lo) * E * 2}
        rec = {"shape": f"{name} bf16 B{B} L{L} QH{QH} KH{KH} E{E}", "reps": args.reps, "iters": args.iters, "splits": splits,
               "bf16_over_fp8": round(med["bf16"] / med["fp8"], 3), "bf16_over_fp8_min": round(min(ratios), 3),
               "bf16_over_fp8_max": round(max(ratios), 3), "fp8_median_below_bf16_min": med["fp8"] < min(t["bf16"])}
        for n, v in t.items():
            rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1), "visible_kv_bytes": visible[n],
                      "tb_per_s": round(visible[n] / med[n] / 1e6, 3), "error_over_gate": round(gate[n], 4)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del c8, c16, deq
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
