"""Time the expert linear layers on MXFP4 weights against the same layers on the pre-expanded bf16 weights (what a caller did before).

    python tools/perf_moe_mx.py [--out profiles/r05/moe_mx.jsonl] [--only down] [--tokens 64]

bf16 rows, the two projections of gpt-oss-120b (E = 128, k = 4: 2880 -> 5760 and 2880 -> 2880) at T = 8192 tokens (S = 32768 slot rows:
prefill, training) and T = 64 and 256 (S = 256 and 1024: decode), rows routed uniformly at random, random codes with scale bytes
118 ... 126.  The method is that of tools/perf_moe_gemm.py: the arms of one group are timed interleaved in one process, per repeat
`--iters` back-to-back calls of each arm between HIP events, `--reps` >= 10 repeats after `--warmup` untimed calls.  Every arm rotates
over `--copies` copies of its weights, so a call never finds the weights it reads where the previous call left them (one copy of the
smallest operand, 0.56 GB, is already twice the last-level cache).  One JSON line per (shape, group) with the median / min / max
microseconds per arm, the weight bytes an arm reads per call (those of the experts that have rows), and mxfp4's ratio to dense.  Groups:
  fwd     dense (nnop_moe_linear, [E, N, K] bf16 weights, bias) | mxfp4 (nnop_moe_mx_linear, the same weights packed, bias)
  bwd_x   dense (nnop_moe_linear_bwd_x) | mxfp4 (nnop_moe_mx_linear_bwd_x)
Before timing, each mxfp4 result is compared with the dense one bit for bit.  Recorded, not gated.
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
TOKENS = (8192, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the shape name")
    ap.add_argument("--tokens", type=int, default=0, help="one token count instead of 8192, 64 and 256")
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10 or args.only, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    L, M = pkg._lib_moe_linear, pkg._lib_moe_mx
    lin, mx = L.load(), M.load()
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
        dense = [pkg.mxfp4_dequantize(b, s, dt) for b, s in packed]
        bias = torch.randn(E, N, device="cuda").to(dt)
        bytes_dense, bytes_mx = E * N * K * 2, E * N * (K // 2 + K // 32)
        for tokens in ((args.tokens,) if args.tokens else TOKENS):
            S = tokens * k
            off_host = routing(S, E, False)
            off, live = off_host.cuda(), int((off_host[1:] > off_host[:-1]).sum())
            xs, dys = torch.randn(S, K, device="cuda").to(dt), torch.randn(S, N, device="cuda").to(dt)
            ys, dxs = torch.empty_like(dys), torch.empty_like(xs)
            ld = L.MoeLinearDesc(dtype=code[dt], grad_dtype=code[dt], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=K, ld_y=N, ld_w=K, ld_dw=K,
                                 ld_b=N, ld_db=N, flags=0)
            md = M.MoeMxDesc(dtype=code[dt], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=K, ld_y=N, ld_b=N, ld_q=K // 2, ld_s=K // 32, flags=0)
            s = vp(torch.cuda.current_stream().cuda_stream)
            ok = lambda st: st == 0 or sys.exit(f"status {st}")
            turn = {"n": 0}

            def nxt():
                turn["n"] += 1
                return turn["n"] % args.copies

            def fwd_dense(i=None):
                w = dense[nxt() if i is None else i]
                ok(lin.nnop_moe_linear(C.byref(ld), P(ys), P(xs), P(w), P(bias), P(off), s))

            def fwd_mx(i=None):
                b, sc = packed[nxt() if i is None else i]
                ok(mx.nnop_moe_mx_linear(C.byref(md), P(ys), P(xs), P(b), P(sc), P(bias), P(off), s))

            def bwd_dense(i=None):
                w = dense[nxt() if i is None else i]
                ok(lin.nnop_moe_linear_bwd_x(C.byref(ld), P(dxs), P(dys), P(w), P(off), s))

            def bwd_mx(i=None):
                b, sc = packed[nxt() if i is None else i]
                ok(mx.nnop_moe_mx_linear_bwd_x(C.byref(md), P(dxs), P(dys), P(b), P(sc), P(off), s))

            # faster and different is not faster: the same bits first
            for out, a, b in ((ys, fwd_dense, fwd_mx), (dxs, bwd_dense, bwd_mx)):
                a(0)
                want = out.clone()
                out.zero_()
                b(0)
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int16), want.view(torch.int16)), f"{name} S{S}: mxfp4 differs from dense"
            for group, arms in (("fwd", {"dense": fwd_dense, "mxfp4": fwd_mx}), ("bwd_x", {"dense": bwd_dense, "mxfp4": bwd_mx})):
                t = time_arms(arms, args.warmup, args.iters, args.reps)
                med = {n: statistics.median(v) for n, v in t.items()}
                rec = {"shape": f"{name} bf16 S{S} E{E} {K}->{N}", "group": group, "reps": args.reps, "iters": args.iters, "copies": args.copies,
                       "experts_with_rows": live}
                for n, v in t.items():
                    nbytes = (bytes_dense if n == "dense" else bytes_mx) * live // E
                    rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                              "weight_MB_per_call": round(nbytes / 1e6, 1), "weight_TBps": round(nbytes / med[n] / 1e6, 2),
                              "TFLOPs": round(2.0 * S * K * N / med[n] / 1e6, 1)}
                rec["mxfp4_over_dense"] = round(med["mxfp4"] / med["dense"], 3)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del xs, dys, ys, dxs
        del packed, dense
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
