"""Time the weight-streaming forward on MXFP4 expert weights (nnop_moe_mx_decode_linear, the eighth library) against the 128 x 128 tile
forward on the same weights (nnop_moe_mx_linear, the seventh) at decode sizes.

    python tools/perf_moe_mx_decode.py [--out profiles/r06/moe_mx_decode.jsonl] [--only down] [--tokens 64]

bf16 rows, the two projections of gpt-oss-120b (E = 128, k = 4: 2880 -> 5760 and 2880 -> 2880) at T = 1, 4, 16, 64 and 256 tokens
(S = 4 ... 1024 slot rows), rows routed uniformly at random, random codes with scale bytes 118 ... 126, a bias.  The method is that of
tools/perf_moe_mx.py: the two arms are timed interleaved in one process, per repeat `--iters` back-to-back calls of each arm between
HIP events, `--reps` >= 10 repeats after `--warmup` untimed calls; every arm rotates over `--copies` copies of its weights, so a call
never finds the weights it reads where the previous call left them.  One JSON line per shape with the median / min / max microseconds
per arm, the weight bytes a call reads (those of the experts that have rows), the rate that is, and the ratio tile / decode.

Before timing, both results are held against the fp64 formula on the dequantised weights under the gate of tests/moe_linear_ref.py,
u |ref| + (K + 3) 2^-23 (A + |bias|) + floor, which depends on no summation order: the two kernels add in different orders and are not
bit-equal.  Recorded, not gated.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from perf_moe_gemm import routing, time_arms  # noqa: E402

# (shape name, E, k, K, N)
SHAPES = [("gpt-oss-120b gate_up", 128, 4, 2880, 5760), ("gpt-oss-120b down", 128, 4, 2880, 2880)]
TOKENS = (1, 4, 16, 64, 256)
U_BF16, FLOOR_BF16, EPS_MM = 2.0 ** -8, 2.0 ** -134, 2.0 ** -23  # unit roundoff, half the subnormal spacing, an fp32 operation


def worst_ratio(pkg, ys, xs, blocks, scales, bias, off_host, K):
    """max |ys - ref| / gate over the rows of the experts that have them, ref in fp64 on the dequantised weights of one expert at a time"""
    worst = 0.0
    for e in range(off_host.numel() - 1):
        lo, hi = int(off_host[e]), int(off_host[e + 1])
        if hi <= lo:
            continue
        w = pkg.mxfp4_dequantize(blocks[e], scales[e], xs.dtype).double()
        x, b = xs[lo:hi].double(), bias[e].double()
        ref, A = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()
        gate = U_BF16 * ref.abs() + (K + 3) * EPS_MM * A + FLOOR_BF16
        worst = max(worst, float(((ys[lo:hi].double() - ref).abs() / gate).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the shape name")
    ap.add_argument("--tokens", type=int, default=0, help="one token count instead of 1, 4, 16, 64 and 256")
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10 or args.only, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    M, D = pkg._lib_moe_mx, pkg._lib_moe_mx_decode
    mx, dec = M.load(), D.load()
    vp = C.c_void_p
    P = lambda t: vp(t.data_ptr())
    dt, code = torch.bfloat16, pkg._common._DTYPES
    lines = []
    for name, E, k, K, N in SHAPES:
        if args.only not in name:
            continue
        torch.manual_seed(0)
        packed = [(torch.randint(0, 256, (E, N, K // 32, 16), dtype=torch.uint8, device="cuda"),
                   torch.randint(118, 127, (E, N, K // 32), dtype=torch.uint8, device="cuda")) for _ in range(args.copies)]
        bias = torch.randn(E, N, device="cuda").to(dt)
        bytes_mx = E * N * (K // 2 + K // 32)
        for tokens in ((args.tokens,) if args.tokens else TOKENS):
            S = tokens * k
            off_host = routing(S, E, False)
            counts = off_host[1:] - off_host[:-1]
            off, live = off_host.cuda(), int((counts > 0).sum())
            xs = torch.randn(S, K, device="cuda").to(dt)
            ys = torch.empty(S, N, device="cuda", dtype=dt)
            fields = dict(dtype=code[dt], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=K, ld_y=N, ld_b=N, ld_q=K // 2, ld_s=K // 32, flags=0)
            md, dd = M.MoeMxDesc(**fields), D.MoeMxDecodeDesc(**fields)
            s = vp(torch.cuda.current_stream().cuda_stream)
            ok = lambda st: st == 0 or sys.exit(f"status {st}")
            turn = {"n": 0}

            def nxt():
                turn["n"] += 1
                return turn["n"] % args.copies

            def tile(i=None):
                b, sc = packed[nxt() if i is None else i]
                ok(mx.nnop_moe_mx_linear(C.byref(md), P(ys), P(xs), P(b), P(sc), P(bias), P(off), s))

            def decode(i=None):
                b, sc = packed[nxt() if i is None else i]
                ok(dec.nnop_moe_mx_decode_linear(C.byref(dd), P(ys), P(xs), P(b), P(sc), P(bias), P(off), s))

            # faster and wrong is not faster: both inside the gate first
            gate = {}
            for arm, fn in (("tile", tile), ("decode", decode)):
                ys.fill_(float("nan"))
                fn(0)
                torch.cuda.synchronize()
                gate[arm] = worst_ratio(pkg, ys, xs, packed[0][0], packed[0][1], bias, off_host, K)
                assert gate[arm] <= 1.0, f"{name} S{S}: {arm} misses the gate: error / gate = {gate[arm]}"
            t = time_arms({"tile": tile, "decode": decode}, args.warmup, args.iters, args.reps)
            med = {n: statistics.median(v) for n, v in t.items()}
            nbytes = bytes_mx * live // E
            rec = {"shape": f"{name} bf16 S{S} E{E} {K}->{N}", "group": "fwd", "reps": args.reps, "iters": args.iters, "copies": args.copies,
                   "experts_with_rows": live, "max_rows_per_expert": int(counts.max()), "weight_MB_per_call": round(nbytes / 1e6, 1)}
            for n, v in t.items():
                rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                          "weight_TBps": round(nbytes / med[n] / 1e6, 2), "error_over_gate": round(gate[n], 4)}
            rec["tile_over_decode"] = round(med["tile"] / med["decode"], 3)
            rec["faster_beyond_spread"] = max(t["decode"]) < min(t["tile"])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del xs, ys
        del packed
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
