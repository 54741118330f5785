"""Time the mixture-of-experts token permute and weighted combine (forward, pullback) against the PyTorch composition they replace.

    python tools/perf_moe_data.py [--out profiles/moe_data/perf.jsonl]

The method of tools/perf_moe.py: HIP events, `--warmup` untimed launches, then `--reps` timed repeats of `--iters` back-to-back calls
each; one JSON line per (shape, pass) with the median / min / max microseconds of the fused call and of the composition, timed in the same
process on the same GPU, their ratio, and the fused call's achieved bytes/s against the minimal traffic: the slot-order array once plus the
token-order array once (combine_bwd: ys, dys and dy once each).  The fused calls are single library calls into preallocated buffers
(ctypes, no allocation, no autograd).  The compositions are what a caller wrote before (INTEGRATION.md's earlier recipe):
  permute       x[(perm // k).long()]                                   (the index is precomputed outside the timed region)
  permute_bwd   the autograd backward of that gather for a given dxs    (retain_graph; includes autograd's own dispatch)
  combine       (ys[slot.long()] * w[..., None]).sum(1).to(dtype)       (materialises [T, k, D] in fp32)
  combine_bwd   the autograd backward of that expression for a given dy, in ys and w
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

# (name, dtype, T, D, E, k)
SHAPES = [
    ("gpt-oss-120b bf16 T8192 D2880 E128 k4", torch.bfloat16, 8192, 2880, 128, 4),
    ("Qwen3-MoE bf16 T8192 D2048 E128 k8", torch.bfloat16, 8192, 2048, 128, 8),
    ("Mixtral bf16 T8192 D4096 E8 k2", torch.bfloat16, 8192, 4096, 8, 2),
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
    M = pkg._lib_moe_data
    lib = M.load()
    vp = C.c_void_p
    P = lambda t: vp(t.data_ptr())
    lines = []
    for name, dt, T, D, E, k in SHAPES:
        torch.manual_seed(0)
        S, es = T * k, torch.empty(0, dtype=dt).element_size()
        x, dy = torch.randn(T, D, device="cuda").to(dt), torch.randn(T, D, device="cuda").to(dt)
        ys, dxs = torch.randn(S, D, device="cuda").to(dt), torch.randn(S, D, device="cuda").to(dt)
        w, idx, _ = pkg._moe_router((3.0 * torch.randn(T, E, device="cuda")).to(dt), k)
        _, _, perm, slot = pkg.moe_dispatch_plan(idx, E)
        xs, dys, y, dx, dw = torch.empty_like(ys), torch.empty_like(ys), torch.empty_like(x), torch.empty_like(x), torch.empty_like(w)
        d = M.MoeRowsDesc(dtype=pkg.attention._DTYPES[dt], tokens=T, topk=k, dim=D, ld_tok=D, ld_slot=D)
        s = vp(torch.cuda.current_stream().cuda_stream)
        fused = dict(
            permute=lambda: lib.nnop_moe_permute(C.byref(d), P(xs), P(x), P(perm), s),
            permute_bwd=lambda: lib.nnop_moe_permute_bwd(C.byref(d), P(dx), P(dxs), P(slot), s),
            combine=lambda: lib.nnop_moe_combine(C.byref(d), P(y), P(ys), P(w), P(slot), s),
            combine_bwd=lambda: lib.nnop_moe_combine_bwd(C.byref(d), P(dys), P(dw), P(dy), P(ys), P(w), P(perm), P(slot), s))
        nbytes = dict(permute=(S + T) * D * es, permute_bwd=(S + T) * D * es, combine=(S + T) * D * es, combine_bwd=(2 * S + T) * D * es)

        tok, slotl = (perm // k).long(), slot.long()
        x_leaf, ys_leaf, w_leaf = x.clone().requires_grad_(True), ys.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xs_graph = x_leaf[tok]
        y_graph = (ys_leaf[slotl] * w_leaf[..., None]).sum(1).to(dt)
        torch_ = dict(
            permute=lambda: x[tok],
            permute_bwd=lambda: torch.autograd.grad(xs_graph, x_leaf, dxs, retain_graph=True),
            combine=lambda: (ys[slotl] * w[..., None]).sum(1).to(dt),
            combine_bwd=lambda: torch.autograd.grad(y_graph, (ys_leaf, w_leaf), dy, retain_graph=True))
        for pas in ("permute", "permute_bwd", "combine", "combine_bwd"):
            assert fused[pas]() == 0
            tf = _time(fused[pas], args.warmup, args.iters, args.reps)
            tt = _time(torch_[pas], args.warmup, args.iters, args.reps)
            mf, mt = statistics.median(tf), statistics.median(tt)
            rec = {"shape": name, "pass": pas, "us_median": round(mf, 2), "us_min": round(min(tf), 2), "us_max": round(max(tf), 2),
                   "torch_us_median": round(mt, 2), "torch_us_min": round(min(tt), 2), "torch_us_max": round(max(tt), 2),
                   "ratio": round(mf / mt, 3), "min_bytes": nbytes[pas], "tb_per_s": round(nbytes[pas] / mf / 1e6, 3),
                   "reps": args.reps, "iters": args.iters}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del xs_graph, y_graph
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
