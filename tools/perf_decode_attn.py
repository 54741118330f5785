"""Time decode attention over a KV cache (nnop_decode_attn, the tenth library) against the only way the other libraries offer for a
decode step: flash_attention with QL = 1 and a [B, KL] kpad_mask built every step (the mask carries the length and, where the layer has
one, the window: with one query a top-left window cannot stand at the end of the sequence).

    python tools/perf_decode_attn.py [--out profiles/r08/decode_attn.jsonl] [--only llama]

bf16; gpt-oss-120b (QH 64, KH 8, E 64, sinks) dense and with its window of 128, Llama-3-70B (QH 64, KH 8, E 128) dense; B = 1, 8, 64;
every sequence as long as its cache, 1024, 8192 and (up to B = 8) 65536 keys.  Arms:

    decode     decode_attention_into, automatic splits, caller-owned workspace
    flash      the mask from seqlens (three small torch kernels) and flash_attention
    sdpa       torch.nn.functional.scaled_dot_product_attention with the same mask, no sinks: for information only, 3 calls, not alternated

The method is that of tools/perf_moe_gemm.py: decode and flash alternate in one process, per repeat `--iters` back-to-back calls between
HIP events, `--reps` >= 10 repeats after `--warmup` untimed calls; each arm rotates over two copies of the cache so that L2 does not
hold it.  Before timing both arms are held against an fp64 softmax over the visible keys of sequence 0 under the bf16 gate of tests/util.py.
One JSON line per shape: microseconds (median, min, max), the visible K + V bytes, those bytes over the median in TB/s, flash / decode,
the resolved split count, and whether decode's median lies below flash's fastest repeat.
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

MODELS = (("gpt-oss-120b dense", 64, 8, 64, None, True), ("gpt-oss-120b window128", 64, 8, 64, 128, True),
          ("llama-3-70b dense", 64, 8, 128, None, False))
BATCHES, LENGTHS = (1, 8, 64), (1024, 8192, 65536)


def inside_gate(o, q, k, v, lo, n, sinks):
    """sequence 0 of o against fp64 on keys lo ... n - 1; worst error / gate"""
    G = q.shape[1] // k.shape[1]
    kk, vv = (t[0, :, lo:n].double().repeat_interleave(G, 0) for t in (k, v))
    x = torch.einsum("hqe,hje->hqj", q[0].double(), kk) / q.shape[-1] ** 0.5
    if sinks is not None:
        x = torch.cat([x, sinks.double()[:, None, None]], -1)
    ref = torch.einsum("hqj,hje->hqe", torch.softmax(x, -1)[..., :n - lo], vv)
    tol = ATOL_FRAC["bf16"] * ref.abs().max() + RTOL["bf16"] * ref.abs()
    return float(((o[0].double() - ref).abs() / tol).max())


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
        caches = [tuple(torch.randn(B, KH, L, E, device=dev).to(dt) for _ in range(2)) for _ in range(2)]
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        sinks = torch.randn(QH, device=dev) if has_sink else None
        lo = 0 if window is None else max(0, L - 1 - window)
        splits, nbytes = pkg.decode_attention_plan(q, *caches[0], window_left=window)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        o, ar, turn = torch.empty_like(q), torch.arange(L, device=dev)[None, :], {"n": 0}

        def nxt(i):
            turn["n"] += i is None
            return caches[turn["n"] % 2 if i is None else i]

        def mask():
            m = ar < lens[:, None]
            return m if window is None else m & (ar >= (lens[:, None] - 1 - window))

        def decode(i=None):
            k, v = nxt(i)
            return pkg.decode_attention_into(o, None, q, k, v, lens, window_left=window, sinks=sinks, workspace=ws)

        def flash(i=None):
            k, v = nxt(i)
            return pkg.flash_attention(q, k, v, causal=False, kpad_mask=mask(), sinks=sinks)

        def sdpa(i=None):
            k, v = nxt(i)
            return torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask()[:, None, None, :], enable_gqa=True)

        gate = {n: inside_gate(f(0), q, *caches[0], lo, L, sinks) for n, f in (("decode", decode), ("flash", flash))}
        assert max(gate.values()) <= 1.0, f"{name} B{B} L{L}: outside the gate: {gate}"
        t = time_arms({"decode": decode, "flash": flash}, args.warmup, args.iters, args.reps)
        try:
            t["sdpa"] = time_arms({"sdpa": sdpa}, 1, 1, 3)["sdpa"]
        except Exception as e:  # information only: some builds have no kernel for this call
            print(f"sdpa skipped: {type(e).__name__}", file=sys.stderr)
        med = {n: statistics.median(v) for n, v in t.items()}
        visible = 2 * B * KH * (L - lo) * E * 2
        rec = {"shape": f"{name} bf16 B{B} L{L} QH{QH} KH{KH} E{E}", "reps": args.reps, "iters": args.iters, "splits": splits,
               "visible_kv_bytes": visible, "decode_tb_per_s": round(visible / med["decode"] / 1e6, 3),
               "flash_over_decode": round(med["flash"] / med["decode"], 2), "decode_median_below_flash_min": med["decode"] < min(t["flash"])}
        for n, v in t.items():
            rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
            if n in gate:
                rec[n]["error_over_gate"] = round(gate[n], 4)
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
