"""Time decode attention over a paged FP8 KV cache (nnop_paged_attn_fp8, the fourteenth library) against the two calls it joins: the
dense FP8 call (nnop_decode_attn_fp8, the eleventh) on the same codes gathered into a dense cache -- what reading the pages where they
lie costs -- and the 16-bit paged call (nnop_paged_attn, the twelfth) on the same values in bf16 -- what keeping the pages in FP8 gains.
The gather a caller with an FP8 pool had to make per step before is not timed.

    python tools/perf_paged_attn_fp8.py [--out profiles/r12/paged_attn_fp8.jsonl] [--only llama]

The shapes are tools/perf_paged_attn.py's (128 MiB or more of visible K + V in bf16): bf16 queries; gpt-oss-120b (QH 64, KH 8, E 64,
sinks) and Llama-3-70B (QH 64, KH 8, E 128), dense; B = 1, 8, 64; every sequence as long as its table; a scale per KV head.  Arms:

    paged16    paged_decode_attention_fp8_into on a [P, 16, KH, E] pool of codes (the vLLM layout) with a shuffled table
    paged128   the same codes in pages of 128
    dense8     decode_attention_fp8_into on those codes gathered into [B, KH, L, E]; the same splits and workspace
    paged16b   paged_decode_attention_into on the dequantised values in bf16, pages of 16, the same table

The method is that tool's: the arms alternate in one process, per repeat `--iters` back-to-back calls between HIP events, `--reps` >= 10
repeats after `--warmup` untimed calls; each arm rotates over two copies of its cache so that L2 does not hold it.  Before timing the
dense8 arm is held against an fp64 softmax over the dequantised sequence 0 under the bf16 gate of tests/util.py, each FP8 paged arm
against the dense8 arm's bits and the bf16 arm against fp64 on the values its pool holds.  One JSON line per shape: microseconds
(median, min, max) of the arms, the visible K + V bytes over the median in TB/s, and the two ratios -- dense8 / paged (the cost of paging) and
paged16b / paged (the gain of FP8 pages) -- each with its spread over the paired repeats.
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
        if args.only not in name or window is not None or 2 * B * KH * L * E * 2 < MIN_VISIBLE or (L == 65536 and B > 8):
            continue
        torch.manual_seed(B + L)
        q = torch.randn(B, QH, 1, E, device=dev).to(dt)
        ks, vs = (torch.linspace(0.6, 1.7, KH, device=dev), torch.linspace(1.3, 0.4, KH, device=dev))
        dense = [tuple((torch.randn(B, KH, L, E, device=dev) / s[None, :, None, None]).to(torch.float8_e4m3fn) for s in (ks, vs)) for _ in range(2)]
        paged = {page: [] for page in (*PAGES, "16b")}
        for kv in dense:                                 # the same codes, every page somewhere else in a pool of exactly B L / page pages
            for page in PAGES:
                n = L // page
                table = torch.randperm(B * n, device=dev).to(torch.int32).view(B, n)
                pools = []
                for t in kv:
                    pool = torch.empty(B * n, page, KH, E, dtype=torch.uint8, device=dev)
                    pool[table.long()] = t.view(torch.uint8).view(B, KH, n, page, E).permute(0, 2, 3, 1, 4)
                    pools.append(pool.transpose(1, 2))
                paged[page].append((*pools, table))
            k8, v8, table = paged[16][-1]                # pages of 16 once more, dequantised to bf16: the twelfth library's pool
            paged["16b"].append(((k8.view(torch.float8_e4m3fn).float() * ks[None, :, None, None]).to(dt),
                                 (v8.view(torch.float8_e4m3fn).float() * vs[None, :, None, None]).to(dt), table))
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        sinks = torch.randn(QH, device=dev) if has_sink else None
        splits, nbytes = pkg.decode_attention_fp8_plan(q, *dense[0])
        assert all((splits, nbytes) == pkg.paged_decode_attention_fp8_plan(q, *paged[p][0]) for p in PAGES)
        assert (splits, nbytes) == pkg.paged_decode_attention_plan(q, *paged["16b"][0])
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        o, turn = torch.empty_like(q), {}

        def nxt(arm, caches, i):
            turn[arm] = turn.get(arm, 0) + (i is None)
            return caches[turn[arm] % 2 if i is None else i]

        def dense_arm(i=None):
            k, v = nxt("dense8", dense, i)
            return pkg.decode_attention_fp8_into(o, None, q, k, v, lens, k_scale=ks, v_scale=vs, sinks=sinks, workspace=ws)

        def paged_arm(page):
            def arm(i=None):
                k, v, table = nxt(page, paged[page], i)
                return pkg.paged_decode_attention_fp8_into(o, None, q, k, v, table, lens, k_scale=ks, v_scale=vs, sinks=sinks, workspace=ws)
            return arm

        def bf16_arm(i=None):
            k, v, table = nxt("16b", paged["16b"], i)
            return pkg.paged_decode_attention_into(o, None, q, k, v, table, lens, sinks=sinks, workspace=ws)

        arms = {"dense8": dense_arm, **{f"paged{p}": paged_arm(p) for p in PAGES}, "paged16b": bf16_arm}
        deq = tuple(c[:1].double() * s.double()[None, :, None, None] for c, s in zip(dense[0], (ks, vs)))
        want = dense_arm(0).clone()
        c16 = tuple((c[:1].float() * s[None, :, None, None]).to(dt) for c, s in zip(dense[0], (ks, vs)))     # the values the bf16 pool holds
        gate = {"dense8": inside_gate(want, q, *deq, 0, L, sinks), "paged16b": inside_gate(bf16_arm(0), q, *c16, 0, L, sinks)}
        assert max(gate.values()) <= 1.0, f"{name} B{B} L{L}: outside the gate: {gate}"
        for p in PAGES:
            assert torch.equal(arms[f"paged{p}"](0), want), f"{name} B{B} L{L}: page size {p} does not give the dense FP8 call's bits"
        t = time_arms(arms, args.warmup, args.iters, args.reps)
        med = {n: statistics.median(v) for n, v in t.items()}
        visible = {n: 2 * B * KH * L * E * (2 if n == "paged16b" else 1) for n in t}
        rec = {"shape": f"{name} bf16 B{B} L{L} QH{QH} KH{KH} E{E}", "reps": args.reps, "iters": args.iters, "splits": splits,
               "error_over_gate": {n: round(g, 4) for n, g in gate.items()}}
        for n, v in t.items():
            rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1), "visible_kv_bytes": visible[n],
                      "tb_per_s": round(visible[n] / med[n] / 1e6, 3)}
        for n in (f"paged{p}" for p in PAGES):           # the arms alternate: repeat r of one stands beside repeat r of the other
            for other, label in (("dense8", "dense8_over_paged"), ("paged16b", "bf16_over_fp8")):
                ratios = [x / y for x, y in zip(t[other], t[n])]
                rec[n].update({label: round(med[other] / med[n], 3), label + "_min": round(min(ratios), 3), label + "_max": round(max(ratios), 3)})
            rec[n]["median_below_bf16_min"] = med[n] < min(t["paged16b"])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del dense, paged, deq
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
