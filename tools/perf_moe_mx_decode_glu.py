"""Time the decode expert forward with the gated activation in its epilogue and the token gather in front (nnop_moe_mx_decode_glu, the
ninth library) against the launches it replaces: nnop_moe_permute -> nnop_moe_mx_decode_linear -> nnop_glu.

    python tools/perf_moe_mx_decode_glu.py [--out profiles/r07/moe_mx_decode_glu.jsonl] [--tokens 16]

bf16 rows, the gate-up projection of gpt-oss-120b (E = 128, k = 4, K = 2880, I = 2880: 5760 weight rows per expert, interleaved), a bias,
swiglu_oai, at T = 1, 4, 16, 64 and 256 tokens (S = 4 ... 1024 slot rows); every token picks k distinct experts uniformly at random and
the plan is moe_dispatch_plan's.  Random codes with scale bytes 118 ... 126; x is scaled by a power of two so that the pre-activations have
a standard deviation near 5 (at unit scale every swiglu_oai element saturates).  Four arms, all through the C ABI:

    fused+perm      nnop_moe_mx_decode_glu with perm                                     1 launch
    permute+2       nnop_moe_permute, nnop_moe_mx_decode_linear, nnop_glu                3 launches
    fused           nnop_moe_mx_decode_glu on rows already in slot order                 1 launch
    2 calls         nnop_moe_mx_decode_linear, nnop_glu                                  2 launches

The method is that of tools/perf_moe_mx_decode.py: the arms are timed interleaved in one process, per repeat `--iters` back-to-back calls
of each arm between HIP events, `--reps` >= 10 repeats after `--warmup` untimed calls; every arm rotates over `--copies` copies of its
weights.  One JSON line per S with the median / min / max microseconds per arm and the two ratios composition / fused; a fused arm counts
as not slower when its median is not above the composition's maximum and its minimum not above the composition's median.

Before timing, every arm is held against the fp64 formula on the dequantised weights under the gate of tests/moe_mx_glu_ref.py,
    2 u |ref| + 2e-6 max|ref| + L (|upside| + du) dg + (|a| + L dg) du + floor,   d = (K + 3) 2^-23 (A + |bias|),  L = 1.13,
which depends on no summation order; the root-mean-square errors of the fused and the composed result are recorded beside it.
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

from perf_moe_gemm import time_arms  # noqa: E402

E, TOPK, K, I = 128, 4, 2880, 2880
TOKENS = (1, 4, 16, 64, 256)
ALPHA, LIMIT, L_ACT = 1.702, 7.0, 1.13
U_BF16, TINY_BF16, EPS_MM = 2.0 ** -8, 2.0 ** -133, 2.0 ** -23


def judge(pkg, h, xs, blocks, scales, bias, off_host):
    """(max |h - ref| / gate, root-mean-square error) over the rows of the experts that have them, ref in fp64, one expert at a time"""
    parts, sq, n, hmax = [], 0.0, 0, 0.0
    for e in range(off_host.numel() - 1):
        lo, hi = int(off_host[e]), int(off_host[e + 1])
        if hi <= lo:
            continue
        w = pkg.mxfp4_dequantize(blocks[e], scales[e], xs.dtype).double()
        x, b = xs[lo:hi].double(), bias[e].double()
        p, d = x @ w.t() + b, (K + 3) * EPS_MM * (x.abs() @ w.abs().t() + b.abs())
        gate, up, dg, du = p[:, 0::2], p[:, 1::2], d[:, 0::2], d[:, 1::2]
        gp = gate.clamp(max=LIMIT)
        a, upside = gp * torch.sigmoid(ALPHA * gp), up.clamp(-LIMIT, LIMIT) + 1
        ref = a * upside
        err = (h[lo:hi].double() - ref).abs()
        parts.append((err, ref.abs(), L_ACT * (upside.abs() + du) * dg + (a.abs() + L_ACT * dg) * du))
        sq, n, hmax = sq + float((err * err).sum()), n + err.numel(), max(hmax, float(ref.abs().max()))
    worst = max(float((err / (2 * U_BF16 * r + 2e-6 * hmax + t + TINY_BF16)).max()) for err, r, t in parts)
    return worst, (sq / n) ** 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", type=int, default=0, help="one token count instead of 1, 4, 16, 64 and 256")
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    L, R, D, G = pkg._lib, pkg._lib_moe_data, pkg._lib_moe_mx_decode, pkg._lib_moe_mx_decode_glu
    main_lib, rows_lib, dec, fused_lib = L.load(), R.load(), D.load(), G.load()
    vp = C.c_void_p
    P = lambda t: vp(t.data_ptr())
    dt, code, N = torch.bfloat16, pkg._common._DTYPES, 2 * I
    torch.manual_seed(0)
    packed = [(torch.randint(0, 256, (E, N, K // 32, 16), dtype=torch.uint8, device="cuda"),
               torch.randint(118, 127, (E, N, K // 32), dtype=torch.uint8, device="cuda")) for _ in range(args.copies)]
    bias = torch.randn(E, N, device="cuda").to(dt)
    w0 = pkg.mxfp4_dequantize(packed[0][0][0], packed[0][1][0], dt).double()
    sd = float((torch.randn(64, K, device="cuda").to(dt).double() @ w0.t()).std())
    x_scale = 2.0 ** round(torch.log2(torch.tensor(5.0 / sd)).item())
    del w0
    lines = []
    for tokens in ((args.tokens,) if args.tokens else TOKENS):
        S = tokens * TOPK
        g = torch.Generator(device="cuda").manual_seed(tokens)
        idx = torch.rand(tokens, E, generator=g, device="cuda").topk(TOPK, dim=1).indices.to(torch.int32)
        counts, off, perm, _ = pkg.moe_dispatch_plan(idx, E)
        off_host, live = off.cpu(), int((counts > 0).sum())
        x = (torch.randn(tokens, K, generator=g, device="cuda") * x_scale).to(dt)
        xs, gu = torch.empty(S, K, device="cuda", dtype=dt), torch.empty(S, N, device="cuda", dtype=dt)
        h = torch.empty(S, I, device="cuda", dtype=dt)
        common = dict(dtype=code[dt], rows=S, experts=E, in_dim=K, ld_x=K, ld_b=N, ld_q=K // 2, ld_s=K // 32, flags=0)
        dd = D.MoeMxDecodeDesc(out_dim=N, ld_y=N, **common)
        glu = dict(inter_dim=I, ld_h=I, act=L.GLU_ACTS["swiglu_oai"], layout=G.LAYOUTS["interleaved"], alpha=ALPHA, limit=LIMIT, **common)
        fd, fpd = G.MoeMxDecodeGluDesc(tokens=0, topk=0, **glu), G.MoeMxDecodeGluDesc(tokens=tokens, topk=TOPK, **glu)
        pd = R.MoeRowsDesc(dtype=code[dt], tokens=tokens, topk=TOPK, dim=K, ld_tok=K, ld_slot=K)
        gd = L.GluDesc(dtype=code[dt], act=L.GLU_ACTS["swiglu_oai"], layout=L.GLU_INTERLEAVED, reserved=0, rows=S, n=I, ld=N, alpha=ALPHA,
                       limit=LIMIT)
        s = vp(torch.cuda.current_stream().cuda_stream)
        ok = lambda st: st == 0 or sys.exit(f"status {st}")
        turn = {"n": 0}

        def nxt(i):
            if i is not None:
                return packed[i]
            turn["n"] += 1
            return packed[turn["n"] % args.copies]

        def two_calls(i=None):
            b, sc = nxt(i)
            ok(dec.nnop_moe_mx_decode_linear(C.byref(dd), P(gu), P(xs), P(b), P(sc), P(bias), P(off), s))
            ok(main_lib.nnop_glu(C.byref(gd), P(h), P(gu), None, s))

        def permute_two_calls(i=None):
            ok(rows_lib.nnop_moe_permute(C.byref(pd), P(xs), P(x), P(perm), s))
            two_calls(i)

        def fused(i=None):
            b, sc = nxt(i)
            ok(fused_lib.nnop_moe_mx_decode_glu(C.byref(fd), P(h), P(xs), P(b), P(sc), P(bias), P(off), None, s))

        def fused_perm(i=None):
            b, sc = nxt(i)
            ok(fused_lib.nnop_moe_mx_decode_glu(C.byref(fpd), P(h), P(x), P(b), P(sc), P(bias), P(off), P(perm), s))

        arms = {"fused+perm": fused_perm, "permute+2": permute_two_calls, "fused": fused, "2 calls": two_calls}
        # faster and wrong is not faster: every arm inside the gate first (permute+2 runs first and leaves xs for the arms without perm)
        gate, rms = {}, {}
        for arm in ("permute+2", "fused+perm", "fused", "2 calls"):
            h.fill_(float("nan"))
            arms[arm](0)
            torch.cuda.synchronize()
            gate[arm], rms[arm] = judge(pkg, h, xs, packed[0][0], packed[0][1], bias, off_host)
            assert gate[arm] <= 1.0, f"S{S}: {arm} misses the gate: error / gate = {gate[arm]}"
        t = time_arms(arms, args.warmup, args.iters, args.reps)
        med = {n: statistics.median(v) for n, v in t.items()}
        rec = {"shape": f"gpt-oss-120b gate_up + swiglu_oai bf16 S{S} T{tokens} E{E} k{TOPK} {K}->2x{I}", "group": "fwd", "reps": args.reps,
               "iters": args.iters, "copies": args.copies, "experts_with_rows": live, "max_rows_per_expert": int(counts.max()), "x_scale": x_scale}
        for n, v in t.items():
            rec[n] = {"us_median": round(med[n], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                      "error_over_gate": round(gate[n], 4), "rms_error": float(f"{rms[n]:.4e}")}
        for f, c, key in (("fused+perm", "permute+2", "with_perm"), ("fused", "2 calls", "without_perm")):
            rec[f"composition_over_fused_{key}"] = round(med[c] / med[f], 3)
            rec[f"not_slower_{key}"] = med[f] <= max(t[c]) and min(t[f]) <= med[c]
            rec[f"faster_beyond_spread_{key}"] = max(t[f]) < min(t[c])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
