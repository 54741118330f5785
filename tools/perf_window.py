"""Time the sliding-window forward and backward against the unwindowed causal call (HIP events, warm-up, repeats).

    python tools/perf_window.py [--out profiles/r05/window.jsonl] [--lib path/to/libnnop_hip.so] [--only masked]

One JSON line per (shape, window, pass): median / min / max microseconds over `--reps` timed repeats of `--iters` back-to-back
launches each, after `--warmup` untimed launches.  Every timed call is one library call into preallocated buffers (the
ctypes entry points, no allocation, no autograd).  `--lib` times another build of the library through the calls both ABI
versions share (nnop_fa_fwd / nnop_fa_bwd, no window): the masked-mode check of existing launches, run interleaved with the
current library in separate processes.
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

# (name, dtype, E, L, H, B, causal, windows): `None` = the unwindowed call
WINDOWED = [
    ("bf16 E128 L16384 H8 B1 causal", torch.bfloat16, 128, 16384, 8, 1, True, [None, (1023, 0)]),
    ("bf16 E128 L32768 H8 B1 causal", torch.bfloat16, 128, 32768, 8, 1, True, [None, (1023, 0)]),
    ("bf16 E64 L16384 H8 B1 causal", torch.bfloat16, 64, 16384, 8, 1, True, [None, (1023, 0), (255, 0)]),
]
MASKED = [("fp32 E64 L4096 H4 B4 causal", torch.float32, 64, 4096, 4, 4, True, [None])]
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


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
    ap.add_argument("--lib", default=None, help="another libnnop_hip.so (unwindowed calls only)")
    ap.add_argument("--only", choices=["windowed", "masked"], default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import __graft_entry__ as ge
    pkg = ge.load_package()
    L = pkg._lib
    lib = L.load() if args.lib is None else C.CDLL(args.lib)
    tag = "current" if args.lib is None else os.path.basename(os.path.dirname(os.path.abspath(args.lib)))
    vp = C.c_void_p
    lib.nnop_fa_fwd.restype = lib.nnop_fa_bwd.restype = C.c_int
    lib.nnop_fa_bwd_workspace_bytes.restype = C.c_size_t
    lib.nnop_fa_bwd_workspace_bytes.argtypes = [C.POINTER(L.FaDesc)]

    cfgs = (WINDOWED if args.only != "masked" else []) + (MASKED if args.only != "windowed" else [])
    lines = []
    for name, dt, E, Lq, H, B, causal, windows in cfgs:
        torch.manual_seed(0)
        mk = lambda: torch.randn(B, H, Lq, E, device="cuda").to(dt)
        q, k, v, do = mk(), mk(), mk(), mk()
        o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ms, ls = (torch.empty(B, H, Lq, device="cuda", dtype=dt) for _ in range(2))
        d = L.FaDesc(dtype=_DT[dt], emb=E, ql=Lq, kl=Lq, qh=H, kh=H, batch=B, causal=int(causal))
        ws = torch.empty(int(lib.nnop_fa_bwd_workspace_bytes(C.byref(d))), dtype=torch.uint8, device="cuda")
        s = vp(torch.cuda.current_stream().cuda_stream)
        P = lambda t: vp(t.data_ptr())
        for w in windows:
            if w is not None and args.lib is not None:
                continue
            opts = L.fa_opts(w)
            if opts is None:
                fwd = lambda: lib.nnop_fa_fwd(C.byref(d), P(o), P(ms), P(ls), P(q), P(k), P(v), vp(0), vp(0), s)
                bwd = lambda: lib.nnop_fa_bwd(C.byref(d), P(dq), P(dk), P(dv), vp(0), P(do), P(o), P(ms), P(ls), P(q), P(k),
                                              P(v), vp(0), vp(0), P(ws), C.c_size_t(ws.numel()), s)
            else:
                fwd = lambda: lib.nnop_fa_fwd_ex(C.byref(d), C.byref(opts), P(o), P(ms), P(ls), P(q), P(k), P(v), vp(0), vp(0), s)
                bwd = lambda: lib.nnop_fa_bwd_ex(C.byref(d), C.byref(opts), P(dq), P(dk), P(dv), vp(0), P(do), P(o), P(ms), P(ls),
                                                 P(q), P(k), P(v), vp(0), vp(0), P(ws), C.c_size_t(ws.numel()), s)
            assert fwd() == 0
            assert bwd() == 0
            for pas, fn in (("fwd", fwd), ("bwd", bwd)):
                t = _time(fn, args.warmup, args.iters, args.reps)
                rec = dict(shape=name, window=w, pass_=pas, lib=tag, us_median=round(statistics.median(t), 2),
                           us_min=round(min(t), 2), us_max=round(max(t), 2), reps=args.reps, iters=args.iters,
                           fwd_form=L.fwd_form(d, window=w) if args.lib is None else None)
                rec["pass"] = rec.pop("pass_")
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
