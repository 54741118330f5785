"""Time logit soft-capping: the capped call, the same call uncapped on the same 32-row kernels, and the default uncapped call
(HIP events, warm-up, repeats).

    python tools/perf_softcap.py [--out profiles/r05/softcap.jsonl] [--lib path/to/libnnop_hip.so] [--cap 30]

Per shape and pass (forward, backward) three variants:
    (a) capped     nnop_fa_fwd_softcap / nnop_fa_bwd_softcap with the cap
    (b) row32      no cap, forced onto the kernels the cap runs on by a window that removes almost nothing, (QL - 2, -1)
    (c) default    no cap, no window: whatever forms the launcher picks (duo / w64 / split where they apply)
(a) / (b) is what the tanh costs; (a) / (c) is what a capped call pays for not being on the fast forms.  One JSON line per (shape,
variant, pass): median / min / max microseconds over `--reps` timed repeats of `--iters` back-to-back launches each, after `--warmup`
untimed launches.  Every timed call is one library call into preallocated buffers (ctypes, no allocation, no autograd); a backward
is everything nnop_fa_bwd launches (preprocess, dK/dV, dQ).  `--lib` times variant (c) alone with another build of the library (the
check that existing launches did not move), through nnop_fa_fwd / nnop_fa_bwd, which every build has.
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

# (name, dtype, E, L, H, B, causal)
SHAPES = [
    ("bf16 E64 L4096 H4 B4", torch.bfloat16, 64, 4096, 4, 4, False),
    ("fp32 E64 L4096 H4 B4", torch.float32, 64, 4096, 4, 4, False),
    ("bf16 E128 L8192 H8 B2 causal", torch.bfloat16, 128, 8192, 8, 2, True),
]
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
    ap.add_argument("--lib", default=None, help="another libnnop_hip.so (the default uncapped call only)")
    ap.add_argument("--cap", type=float, default=30.0)
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

    lines = []
    for name, dt, E, Lq, H, B, causal in SHAPES:
        torch.manual_seed(0)
        mk = lambda: torch.randn(B, H, Lq, E, device="cuda").to(dt)
        q, k, v, do = mk(), mk(), mk(), mk()
        o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ms, ls = (torch.empty(B, H, Lq, device="cuda", dtype=dt) for _ in range(2))
        d = L.FaDesc(dtype=_DT[dt], emb=E, ql=Lq, kl=Lq, qh=H, kh=H, batch=B, causal=int(causal))
        ws = torch.empty(int(lib.nnop_fa_bwd_workspace_bytes(C.byref(d))), dtype=torch.uint8, device="cuda")
        s = vp(torch.cuda.current_stream().cuda_stream)
        P = lambda t: vp(t.data_ptr())
        wide = (Lq - 2, -1)                                    # removes one key of the last row only: stays a window, costs nothing
        variants = [("default", None, 0.0)] if args.lib is not None else \
            [("capped", None, args.cap), ("row32", wide, 0.0), ("default", None, 0.0)]
        for vname, w, cap in variants:
            opts = L.fa_opts(w)
            op = C.byref(opts) if opts is not None else None
            if vname == "default":
                fwd = lambda: lib.nnop_fa_fwd(C.byref(d), P(o), P(ms), P(ls), P(q), P(k), P(v), vp(0), vp(0), s)
                bwd = lambda: lib.nnop_fa_bwd(C.byref(d), P(dq), P(dk), P(dv), vp(0), P(do), P(o), P(ms), P(ls), P(q), P(k),
                                              P(v), vp(0), vp(0), P(ws), C.c_size_t(ws.numel()), s)
            else:
                cf = C.c_float(cap)
                fwd = lambda: lib.nnop_fa_fwd_softcap(C.byref(d), op, vp(0), cf, P(o), P(ms), P(ls), P(q), P(k), P(v), vp(0), vp(0), s)
                bwd = lambda: lib.nnop_fa_bwd_softcap(C.byref(d), op, vp(0), vp(0), cf, P(dq), P(dk), P(dv), vp(0), P(do), P(o), P(ms),
                                                      P(ls), P(q), P(k), P(v), vp(0), vp(0), P(ws), C.c_size_t(ws.numel()), s)
            assert fwd() == 0               # (the backward below reads this variant's own o, ms, ls)
            assert bwd() == 0
            for pas, fn in (("fwd", fwd), ("bwd", bwd)):
                t = _time(fn, args.warmup, args.iters, args.reps)
                rec = dict(shape=name, variant=vname, softcap=cap, window=w, lib=tag, us_median=round(statistics.median(t), 2),
                           us_min=round(min(t), 2), us_max=round(max(t), 2), reps=args.reps, iters=args.iters,
                           fwd_form=L.fwd_form(d, window=w, softcap=cap) if args.lib is None else None,
                           bwd_kernels=L.bwd_kernels(d, window=w, softcap=cap) if args.lib is None else None)
                rec["pass"] = pas
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
