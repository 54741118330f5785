"""Time MLA decode attention over a paged latent cache (nnop_mla_decode, the eighteenth library) against the PyTorch composition it replaces
on the same pages: gather the visible latent rows through the table, softmax(scale q c^T) c[:, :512] in bf16 with torch.matmul.

    python tools/perf_mla_decode.py [--out profiles/r16/mla_decode.jsonl] [--only QH128]

bf16 queries, QL = 1, page size 64, every sequence as long as its table; QH 128 (DeepSeek-V3 at tensor-parallel degree 1) and 16 (degree
8); B = 1, 8, 64; 8K and 32K keys.  Arms:

    mla      mla_decode_attention_into with the automatic split count and a caller-owned workspace
    torch    pool[table] -> [B, L, 576]; matmul, softmax, matmul in bf16

The method is tools/perf_paged_attn.py's: the arms alternate in one process, per repeat `--iters` back-to-back calls between HIP events
(device-synchronised), `--reps` >= 10 repeats after `--warmup` untimed calls of every shape; each arm rotates over two copies of the
pool so that L2 does not hold it.  Before timing the call is held against an fp64 softmax over sequence 0 under the bf16 gate of
tests/util.py.  One JSON line per shape: microseconds (median, min, max) of the arms, torch / mla with the spread of that ratio over the
paired repeats, and for the call the achieved bytes/s of visible latent (B L 1152 bytes) and FLOP/s (2 B QH L (576 + 512)), both from
shapes, and which of the two lies nearer its ceiling -- 8 TB/s of HBM and 2.5 PFLOP/s of dense bf16 MFMA, the MI355X's data-sheet figures.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from perf_moe_gemm import time_arms  # noqa: E402
from util import ATOL_FRAC, RTOL  # noqa: E402

HEADS, BATCHES, LENGTHS, PAGE, W, V = (128, 16), (1, 8, 64), (8192, 32768), 64, 576, 512
HBM_BYTES_PER_S, MFMA_FLOP_PER_S = 8.0e12, 2.5e15
SCALE = 192 ** -0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the shape name")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev, dt = "cuda", torch.bfloat16
    lines = []
    for QH, L, B in ((h, n, b) for h in HEADS for n in LENGTHS for b in BATCHES):
        shape = f"mla bf16 QH{QH} B{B} L{L} page{PAGE}"
        if args.only not in shape:
            continue
        torch.manual_seed(B + L)
        n = L // PAGE
        q = torch.randn(B, QH, 1, W, device=dev).to(dt)
        caches = []
        for _ in range(2):                               # every page somewhere else in a pool of exactly B L / page pages
            table = torch.randperm(B * n, device=dev).to(torch.int32).view(B, n)
            caches.append((torch.randn(B * n, PAGE, W, device=dev).to(dt), table))
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        splits, nbytes = pkg.mla_decode_attention_plan(q, *caches[0])
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        o, turn = torch.empty(B, QH, 1, V, dtype=dt, device=dev), {}

        def nxt(arm, i):
            turn[arm] = turn.get(arm, 0) + (i is None)
            return caches[turn[arm] % 2 if i is None else i]

        def mla_arm(i=None):
            pool, table = nxt("mla", i)
            return pkg.mla_decode_attention_into(o, None, q, pool, table, lens, workspace=ws)

        def torch_arm(i=None):
            pool, table = nxt("torch", i)
            c = pool[table.long()].view(B, L, W)
            w = torch.softmax(torch.matmul(q[:, :, 0], c.transpose(1, 2)) * SCALE, -1)
            return torch.matmul(w, c[..., :V])

        got = mla_arm(0)[0, :, 0].double().cpu().numpy()
        c0 = caches[0][0][caches[0][1][0].long()].view(L, W).double()
        ref = (torch.softmax(q[0, :, 0].double() @ c0.t() * SCALE, -1) @ c0[:, :V]).cpu().numpy()
        gate = float((np.abs(got - ref) / (ATOL_FRAC["bf16"] * np.abs(ref).max() + RTOL["bf16"] * np.abs(ref))).max())
        assert gate <= 1.0, f"{shape}: the call is outside the gate: {gate}"
        t = time_arms({"mla": mla_arm, "torch": torch_arm}, args.warmup, args.iters, args.reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        visible, flop = B * L * W * 2, 2 * B * QH * L * (W + V)
        bps, fps = visible / med["mla"] * 1e6, flop / med["mla"] * 1e6
        ratios = [x / m for x, m in zip(t["torch"], t["mla"])]
        rec = {"shape": shape, "reps": args.reps, "iters": args.iters, "splits": splits, "visible_latent_bytes": visible, "flop": flop,
               "error_over_gate": round(gate, 4),
               **{k: {"us_median": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)} for k, v in t.items()},
               "torch_over_mla": round(med["torch"] / med["mla"], 2), "torch_over_mla_min": round(min(ratios), 2),
               "torch_over_mla_max": round(max(ratios), 2), "tb_per_s": round(bps / 1e12, 3), "tflop_per_s": round(fps / 1e12, 1),
               "nearer_ceiling": "bytes" if bps / HBM_BYTES_PER_S >= fps / MFMA_FLOP_PER_S else "flop"}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del caches
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
