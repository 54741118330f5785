"""Time the expert linear layers (bias, [E, K, N] weights, accumulating gradients) against the grouped GEMM and what a caller does without them.

    python tools/perf_moe_linear.py [--out profiles/moe_linear/perf.jsonl] [--only gpt-oss]

bf16, T = 8192 tokens, rows routed uniformly at random, random operands: the two projections of gpt-oss-120b (S = 32768, E = 128,
2880 -> 5760 and 2880 -> 2880) and the down projection of Mixtral (S = 16384, E = 8, 14336 -> 4096).  The method is that of
tools/perf_moe_gemm.py: the arms of one group are timed interleaved in one process, per repeat `--iters` back-to-back calls of each arm
between HIP events, `--reps` >= 10 repeats after `--warmup` untimed calls; one JSON line per (shape, group) with the median / min / max
microseconds per arm and each arm's ratio to the group's first arm.  Library calls go through ctypes into preallocated buffers.  Groups:
  fwd        gemm (nnop_moe_gemm, the grouped GEMM alone) | linear_nk_bias | gemm + ys += bias[expert_of_row] (the gather a caller adds; the
             row -> expert index is precomputed) | linear_nk (no bias) | linear_kn | linear_kn_bias
  bwd_x      gemm_bwd_x | linear_nk | linear_kn
  bwd_b      linear_bwd_b (with TB/s on the S N elements it reads) | a loop of dys[lo:hi].sum(0) with offsets already on the host |
             torch.segment_reduce where this torch has it for this type
  bwd_w      gemm_bwd_w (bf16 dw) | linear_kn (bf16 dw) | linear_acc_f32 (added into an fp32 main gradient in the epilogue) |
             gemm_bwd_w + main_grad.add_(dw.float())
Recorded, not gated.
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

from perf_moe_gemm import T, routing, time_arms  # noqa: E402

# (shape name, E, k, K, N)
SHAPES = [("gpt-oss-120b gate_up", 128, 4, 2880, 5760), ("gpt-oss-120b down", 128, 4, 2880, 2880), ("Mixtral down", 8, 2, 14336, 4096)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the shape name")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10 or args.only, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    G, L = pkg._lib_moe_gemm, pkg._lib_moe_linear
    gemm, lin = G.load(), L.load()
    vp = C.c_void_p
    P = lambda t: vp(t.data_ptr())
    dt, code = torch.bfloat16, pkg._common._DTYPES
    lines = []
    for name, E, k, K, N in SHAPES:
        if args.only not in name:
            continue
        S = T * k
        torch.manual_seed(0)
        off_host = routing(S, E, False)
        off, ends = off_host.cuda(), off_host.tolist()
        e_of = torch.repeat_interleave(torch.arange(E), off_host[1:] - off_host[:-1]).cuda()
        xs, dys = torch.randn(S, K, device="cuda").to(dt), torch.randn(S, N, device="cuda").to(dt)
        w = (torch.randn(E, N, K, device="cuda") / K ** 0.5).to(dt)
        wk = w.transpose(1, 2).contiguous()
        bias = torch.randn(E, N, device="cuda").to(dt)
        ys, dxs, dw, db = torch.empty_like(dys), torch.empty_like(xs), torch.empty_like(w), torch.empty_like(bias)
        main = torch.zeros(E, N, K, dtype=torch.float32, device="cuda")
        gd = G.MoeGemmDesc(dtype=code[dt], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=K, ld_y=N, ld_w=K)
        desc = lambda kn=False, f32=False, acc=False: L.MoeLinearDesc(
            dtype=code[dt], grad_dtype=code[torch.float32 if f32 else dt], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=K, ld_y=N,
            ld_w=N if kn else K, ld_dw=N if kn else K, ld_b=N, ld_db=N, flags=(L.KN if kn else 0) | (L.ACCUMULATE if acc else 0))
        nk, kn, acc = desc(), desc(kn=True), desc(f32=True, acc=True)
        s = vp(torch.cuda.current_stream().cuda_stream)
        null = vp(0)
        ok = lambda st: st == 0 or sys.exit(f"status {st}")
        groups = {
            "fwd": {"gemm": lambda: ok(gemm.nnop_moe_gemm(C.byref(gd), P(ys), P(xs), P(w), P(off), s)),
                    "linear_nk_bias": lambda: ok(lin.nnop_moe_linear(C.byref(nk), P(ys), P(xs), P(w), P(bias), P(off), s)),
                    "gemm_then_gather_add": lambda: (ok(gemm.nnop_moe_gemm(C.byref(gd), P(ys), P(xs), P(w), P(off), s)), ys.add_(bias[e_of])),
                    "linear_nk": lambda: ok(lin.nnop_moe_linear(C.byref(nk), P(ys), P(xs), P(w), null, P(off), s)),
                    "linear_kn": lambda: ok(lin.nnop_moe_linear(C.byref(kn), P(ys), P(xs), P(wk), null, P(off), s)),
                    "linear_kn_bias": lambda: ok(lin.nnop_moe_linear(C.byref(kn), P(ys), P(xs), P(wk), P(bias), P(off), s))},
            "bwd_x": {"gemm_bwd_x": lambda: ok(gemm.nnop_moe_gemm_bwd_x(C.byref(gd), P(dxs), P(dys), P(w), P(off), s)),
                      "linear_nk": lambda: ok(lin.nnop_moe_linear_bwd_x(C.byref(nk), P(dxs), P(dys), P(w), P(off), s)),
                      "linear_kn": lambda: ok(lin.nnop_moe_linear_bwd_x(C.byref(kn), P(dxs), P(dys), P(wk), P(off), s))},
            "bwd_b": {"linear_bwd_b": lambda: ok(lin.nnop_moe_linear_bwd_b(C.byref(nk), P(db), P(dys), P(off), s)),
                      "loop_sum": lambda: torch.stack([dys[ends[e]:ends[e + 1]].sum(0) for e in range(E)])},
            "bwd_w": {"gemm_bwd_w": lambda: ok(gemm.nnop_moe_gemm_bwd_w(C.byref(gd), P(dw), P(dys), P(xs), P(off), s)),
                      "linear_kn": lambda: ok(lin.nnop_moe_linear_bwd_w(C.byref(kn), P(dw), P(dys), P(xs), P(off), s)),
                      "linear_acc_f32": lambda: ok(lin.nnop_moe_linear_bwd_w(C.byref(acc), P(main), P(dys), P(xs), P(off), s)),
                      "gemm_bwd_w_then_add": lambda: (ok(gemm.nnop_moe_gemm_bwd_w(C.byref(gd), P(dw), P(dys), P(xs), P(off), s)),
                                                      main.add_(dw.float()))},
        }
        if hasattr(torch, "segment_reduce"):
            lengths = (off[1:] - off[:-1]).long()
            try:
                torch.segment_reduce(dys, "sum", lengths=lengths, axis=0)
                torch.cuda.synchronize()
                groups["bwd_b"]["segment_reduce"] = lambda: torch.segment_reduce(dys, "sum", lengths=lengths, axis=0)
            except Exception as e:                          # recorded, not hidden
                print(json.dumps({"shape": name, "torch.segment_reduce": f"unavailable: {type(e).__name__}: {str(e)[:120]}"}), flush=True)
        for group, arms in groups.items():
            t = time_arms(arms, args.warmup, args.iters, args.reps)
            med = {n: statistics.median(v) for n, v in t.items()}
            first = next(iter(arms))
            rec = {"shape": f"{name} bf16 S{S} E{E} {K}->{N}", "group": group, "reps": args.reps, "iters": args.iters}
            for n, v in t.items():
                rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                          "ratio_to_" + first: round(med[n] / med[first], 3)}
            if group == "bwd_b":
                rec["linear_bwd_b"]["TBps_read"] = round(S * N * 2 / med["linear_bwd_b"] / 1e6, 2)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del groups, xs, dys, w, wk, ys, dxs, dw, main
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
