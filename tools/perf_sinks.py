"""Time the forward and backward with learned attention sinks against the same call without them (HIP events, warm-up,
interleaved repeats).

    python tools/perf_sinks.py [--out profiles/r05/sinks.jsonl] [--only c2]

One JSON line per (shape, pass, sinks): median / min / max microseconds over `--reps` timed repeats of `--iters` back-to-back
launches each, after `--warmup` untimed launches.  The repeats of the call with and without sinks alternate, so that both see the
same clock and thermal state.  Every timed call is one library call into preallocated buffers (the ctypes entry points: the call
without sinks is nnop_fa_fwd_ex / nnop_fa_bwd_ex, the call with them nnop_fa_fwd_sinks / nnop_fa_bwd_sinks; no allocation, no
autograd).  A last line per (shape, pass) gives the ratio of the medians.
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

# (key, name, dtype, E, L, QH, KH, B, causal, window)
SHAPES = [
    ("c2", "C2 bf16 E64 L4096 H4 B4", torch.bfloat16, 64, 4096, 4, 4, 4, False, None),
    ("c3", "C3 bf16 E128 L8192 H16 B16 causal", torch.bfloat16, 128, 8192, 16, 16, 16, True, None),
    ("gptoss", "gpt-oss prefill bf16 E64 QH64 KH8 L4096 B2 causal", torch.bfloat16, 64, 4096, 64, 8, 2, True, None),
    ("gptoss-win", "gpt-oss prefill bf16 E64 QH64 KH8 L4096 B2 causal window (127, 0)", torch.bfloat16, 64, 4096, 64, 8, 2, True,
     (127, 0)),
    ("f32", "fp32 E64 L4096 H4 B4 causal", torch.float32, 64, 4096, 4, 4, 4, True, None),
]
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _time_interleaved(fns, warmup, iters, reps):
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) * 1000.0 / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape keys: " + ", ".join(s[0] for s in SHAPES))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import __graft_entry__ as ge
    pkg = ge.load_package()
    L = pkg._lib
    lib = L.load()
    vp = C.c_void_p
    only = set(args.only.split(",")) if args.only else None
    lines = []
    for key, name, dt, E, Lq, QH, KH, B, causal, window in SHAPES:
        if only and key not in only:
            continue
        torch.manual_seed(0)
        q = torch.randn(B, QH, Lq, E, device="cuda").to(dt)
        k, v = (torch.randn(B, KH, Lq, E, device="cuda").to(dt) for _ in range(2))
        do = torch.randn_like(q)
        o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ms, ls = (torch.empty(B, QH, Lq, device="cuda", dtype=dt) for _ in range(2))
        sinks = torch.randn(QH, device="cuda", dtype=torch.float32)
        dsinks = torch.empty_like(sinks)
        d = L.FaDesc(dtype=_DT[dt], emb=E, ql=Lq, kl=Lq, qh=QH, kh=KH, batch=B, causal=int(causal))
        opts = L.fa_opts(window, d)
        op = C.byref(opts) if opts is not None else None
        ws = torch.empty(int(lib.nnop_fa_bwd_workspace_bytes(C.byref(d))), dtype=torch.uint8, device="cuda")
        s = vp(torch.cuda.current_stream().cuda_stream)
        P = lambda t: vp(t.data_ptr())
        fwd = lambda: lib.nnop_fa_fwd_ex(C.byref(d), op, P(o), P(ms), P(ls), P(q), P(k), P(v), vp(0), vp(0), s)
        fwd_s = lambda: lib.nnop_fa_fwd_sinks(C.byref(d), op, P(sinks), P(o), P(ms), P(ls), P(q), P(k), P(v), vp(0), vp(0), s)
        bwd = lambda: lib.nnop_fa_bwd_ex(C.byref(d), op, P(dq), P(dk), P(dv), vp(0), P(do), P(o), P(ms), P(ls), P(q), P(k), P(v),
                                         vp(0), vp(0), P(ws), C.c_size_t(ws.numel()), s)
        bwd_s = lambda: lib.nnop_fa_bwd_sinks(C.byref(d), op, P(sinks), P(dsinks), P(dq), P(dk), P(dv), vp(0), P(do), P(o), P(ms),
                                              P(ls), P(q), P(k), P(v), vp(0), vp(0), P(ws), C.c_size_t(ws.numel()), s)
        assert fwd_s() == 0 and bwd_s() == 0 and fwd() == 0 and bwd() == 0
        for pas, pair in (("fwd", (fwd, fwd_s)), ("bwd", (bwd, bwd_s))):
            t0, t1 = _time_interleaved(pair, args.warmup, args.iters, args.reps)
            meds = []
            for with_sinks, t in ((False, t0), (True, t1)):
                rec = {"shape": name, "pass": pas, "sinks": with_sinks, "us_median": round(statistics.median(t), 2),
                       "us_min": round(min(t), 2), "us_max": round(max(t), 2), "reps": args.reps, "iters": args.iters,
                       "fwd_form": L.fwd_form(d, window=window)}
                meds.append(statistics.median(t))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            rec = {"shape": name, "pass": pas, "ratio_sinks_over_plain": round(meds[1] / meds[0], 4),
                   "delta_us": round(meds[1] - meds[0], 2)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del q, k, v, do, o, dq, dk, dv, ms, ls, ws
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
