"""Time the grouped expert GEMM (forward, both pullbacks) against the loop of vendor GEMMs it replaces.

    python tools/perf_moe_gemm.py [--out profiles/moe_gemm/perf.jsonl] [--only gpt-oss]

bf16, T = 8192 tokens, the expert MLP's two projections at the widths of three models.  Rows are routed uniformly at random; the bwd_w
pass is measured once more under a skewed routing in which one expert owns a quarter of the rows (one workgroup per (expert, tile) walks
all of an expert's rows, so the largest expert bounds that pass).  Operands are random, not zeros.  The arms of one (shape, pass) are
timed interleaved in one process: per repeat, `--iters` back-to-back calls of each arm between HIP events, `--reps` >= 10 repeats after
`--warmup` untimed calls; one JSON line per (shape, routing, pass) with the median / min / max microseconds per arm, TFLOP/s on
2 S_valid K N and the fraction of the 2.52 PFLOP/s nominal bf16 peak.
  fused     one library call into a preallocated buffer (ctypes, no allocation, no autograd); offsets stay on the device
  loop      torch.matmul over the experts' slices with offsets ALREADY on the host (INTEGRATION.md's earlier recipe; the device-to-host
            sync it needs in a real layer is not charged to it); the pullbacks are its autograd (torch.autograd.grad, retain_graph)
  grouped   torch._grouped_mm, forward only, where this torch has it and it runs on this device
Recorded, not gated: where the loop of vendor GEMMs is faster the line says so (ratio > 1).
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

PEAK_BF16 = 2.52e15
T = 8192
# (model, E, k, H, I): hidden and expert-intermediate widths
MODELS = [("gpt-oss-120b", 128, 4, 2880, 2880), ("Mixtral", 8, 2, 4096, 14336), ("Qwen3-MoE", 128, 8, 2048, 768)]


def routing(S, E, skewed, seed=0):
    """offsets [E+1] of S rows sent to E experts uniformly at random; skewed: expert 0 owns a quarter, the rest is uniform over the others"""
    g = torch.Generator().manual_seed(seed)
    if skewed:
        n0 = S // 4
        counts = torch.bincount(torch.randint(1, E, (S - n0,), generator=g), minlength=E)
        counts[0] = n0
    else:
        counts = torch.bincount(torch.randint(0, E, (S,), generator=g), minlength=E)
    return torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32)


def time_arms(arms, warmup, iters, reps):
    """{name: [us per call] * reps}, the arms alternating inside every repeat"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in arms}
    for _ in range(reps):
        for n, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[n].append(a.elapsed_time(b) * 1000.0 / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="a substring of the model name")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10 or args.only, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    M = pkg._lib_moe_gemm
    lib = M.load()
    vp = C.c_void_p
    P = lambda t: vp(t.data_ptr())
    dt = torch.bfloat16
    lines = []
    for model, E, k, H, I in MODELS:
        if args.only not in model:
            continue
        S = T * k
        for K, N in ((H, 2 * I), (I, H)):
            for skewed in (False, True):
                torch.manual_seed(0)
                off_host = routing(S, E, skewed)
                off = off_host.cuda()
                ends = off_host.tolist()
                xs = torch.randn(S, K, device="cuda").to(dt)
                dys = torch.randn(S, N, device="cuda").to(dt)
                w = (torch.randn(E, N, K, device="cuda") / K ** 0.5).to(dt)
                ys, dxs, dw = torch.empty_like(dys), torch.empty_like(xs), torch.empty_like(w)
                d = M.MoeGemmDesc(dtype=pkg.attention._DTYPES[dt], rows=S, experts=E, in_dim=K, out_dim=N, ld_x=K, ld_y=N, ld_w=K)
                s = vp(torch.cuda.current_stream().cuda_stream)
                fused = dict(fwd=lambda: lib.nnop_moe_gemm(C.byref(d), P(ys), P(xs), P(w), P(off), s),
                             bwd_x=lambda: lib.nnop_moe_gemm_bwd_x(C.byref(d), P(dxs), P(dys), P(w), P(off), s),
                             bwd_w=lambda: lib.nnop_moe_gemm_bwd_w(C.byref(d), P(dw), P(dys), P(xs), P(off), s))
                loop_fwd = lambda a, b: torch.cat([a[ends[e]:ends[e + 1]] @ b[e].t() for e in range(E)])
                xs_leaf, w_leaf = xs.clone().requires_grad_(True), w.clone().requires_grad_(True)
                graph = loop_fwd(xs_leaf, w_leaf)
                loop = dict(fwd=lambda: loop_fwd(xs, w),
                            bwd_x=lambda: torch.autograd.grad(graph, xs_leaf, dys, retain_graph=True),
                            bwd_w=lambda: torch.autograd.grad(graph, w_leaf, dys, retain_graph=True))
                grouped = None
                if hasattr(torch, "_grouped_mm"):
                    wt, offs = w.transpose(1, 2), off[1:].contiguous()
                    try:
                        torch._grouped_mm(xs, wt, offs=offs)
                        torch.cuda.synchronize()
                        grouped = lambda: torch._grouped_mm(xs, wt, offs=offs)
                    except Exception as e:                      # recorded, not hidden
                        print(json.dumps({"shape": f"{model} {K}->{N}", "torch._grouped_mm": f"unavailable: {type(e).__name__}: {str(e)[:120]}"}),
                              flush=True)
                flop = 2.0 * S * K * N
                for pas in (("bwd_w",) if skewed else ("fwd", "bwd_x", "bwd_w")):
                    assert fused[pas]() == 0
                    arms = {"fused": fused[pas], "loop": loop[pas]}
                    if pas == "fwd" and grouped is not None:
                        arms["grouped"] = grouped
                    t = time_arms(arms, args.warmup, args.iters, args.reps)
                    med = {n: statistics.median(v) for n, v in t.items()}
                    rec = {"shape": f"{model} bf16 S{S} E{E} {K}->{N}", "routing": "skewed" if skewed else "uniform",
                           "largest_expert": int((off_host[1:] - off_host[:-1]).max()), "pass": pas, "reps": args.reps, "iters": args.iters}
                    for n, v in t.items():
                        rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                                  "tflops": round(flop / med[n] / 1e6, 1), "of_peak": round(flop / med[n] / 1e-6 / PEAK_BF16, 4)}
                    rec["ratio_to_loop"] = round(med["fused"] / med["loop"], 3)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del graph, xs_leaf, w_leaf, loop, fused, xs, dys, w, ys, dxs, dw
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
