"""Time the mixture-of-experts gate (forward, pullback) and the dispatch plan against the PyTorch compositions they replace.

    python tools/perf_moe.py [--out profiles/moe/perf.jsonl]

The method of tools/perf_window.py: HIP events, `--warmup` untimed launches, then `--reps` timed repeats of `--iters` back-to-back calls
each; one JSON line per (shape, pass) with the median / min / max microseconds of the fused call and of the composition, timed in the same
process on the same GPU, and their ratio.  The fused calls are single library calls into preallocated buffers (ctypes, no allocation, no
autograd).  The compositions are what a caller writes today:
  fwd   softmax(float32) -> topk -> (norm="topk": renormalise) plus logsumexp where the fused call's lse is used (it always is computed)
  bwd   the autograd backward of that forward for a given dw (retain_graph; includes autograd's own dispatch)
  plan  argsort(stable) of the flat expert ids -> bincount -> cumsum -> the inverse permutation by a scatter
Recorded, not gated: if the fused path is not faster at a shape the line says so (ratio >= 1).
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

# (name, dtype, T, E, k, norm)
SHAPES = [
    ("gpt-oss-120b bf16 T8192 E128 k4", torch.bfloat16, 8192, 128, 4, "topk"),
    ("gpt-oss-20b bf16 T8192 E32 k4", torch.bfloat16, 8192, 32, 4, "topk"),
    ("Qwen3-MoE bf16 T8192 E128 k8", torch.bfloat16, 8192, 128, 8, "topk"),
    ("bf16 T8192 E256 k8", torch.bfloat16, 8192, 256, 8, "topk"),
]


def _time(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import __graft_entry__ as ge
    pkg = ge.load_package()
    M = pkg._lib_moe
    lib = M.load()
    vp = C.c_void_p
    P = lambda t: vp(t.data_ptr())
    lines = []
    for name, dt, T, E, k, norm in SHAPES:
        torch.manual_seed(0)
        x = (3.0 * torch.randn(T, E, device="cuda")).to(dt)
        w, idx, lse = pkg._moe_router(x, k, norm=norm)
        dw = torch.randn(T, k, device="cuda")
        dx = torch.empty_like(x)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
        counts, offsets, perm, slot = i32(E), i32(E + 1), i32(T * k), i32(T, k)
        rd = M.MoeRouterDesc(dtype=pkg.attention._DTYPES[dt], tokens=T, experts=E, topk=k, ld=E, norm=M.NORMS[norm])
        pd = M.MoePlanDesc(tokens=T, topk=k, experts=E)
        ws = torch.empty(int(lib.nnop_moe_plan_workspace_bytes(C.byref(pd))), dtype=torch.uint8, device="cuda")
        s = vp(torch.cuda.current_stream().cuda_stream)
        fused = dict(
            fwd=lambda: lib.nnop_moe_router(C.byref(rd), P(idx), P(w), P(lse), P(x), s),
            bwd=lambda: lib.nnop_moe_router_bwd(C.byref(rd), P(dx), P(dw), vp(0), P(w), P(idx), P(lse), P(x), s),
            plan=lambda: lib.nnop_moe_plan(C.byref(pd), P(counts), P(offsets), P(perm), P(slot), P(idx), P(ws), C.c_size_t(ws.numel()), s))

        def torch_fwd(src=x):
            p = torch.softmax(src.float(), dim=-1)
            tw, ti = torch.topk(p, k, dim=-1)
            if norm == "topk":
                tw = tw / tw.sum(dim=-1, keepdim=True)
            return tw, ti, torch.logsumexp(src.float(), dim=-1)

        leaf = x.clone().requires_grad_(True)
        tw_graph = torch_fwd(leaf)[0]

        def torch_bwd():
            return torch.autograd.grad(tw_graph, leaf, dw, retain_graph=True)[0]

        flat = idx.view(-1).long()

        def torch_plan():
            order = torch.argsort(flat, stable=True)
            c = torch.bincount(flat, minlength=E)
            off = torch.cumsum(c, 0)
            inv = torch.empty_like(order)
            inv[order] = torch.arange(order.numel(), device=order.device)
            return c, off, order, inv

        torch_ = dict(fwd=torch_fwd, bwd=torch_bwd, plan=torch_plan)
        for pas in ("fwd", "bwd", "plan"):
            assert fused[pas]() == 0
            tf = _time(fused[pas], args.warmup, args.iters, args.reps)
            tt = _time(torch_[pas], args.warmup, args.iters, args.reps)
            mf, mt = statistics.median(tf), statistics.median(tt)
            rec = {"shape": name, "pass": pas, "us_median": round(mf, 2), "us_min": round(min(tf), 2), "us_max": round(max(tf), 2),
                   "torch_us_median": round(mt, 2), "torch_us_min": round(min(tt), 2), "torch_us_max": round(max(tt), 2),
                   "ratio": round(mf / mt, 3), "reps": args.reps, "iters": args.iters}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
