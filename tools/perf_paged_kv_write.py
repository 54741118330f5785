"""Time the paged KV-cache write (nnop_paged_kv_write, the seventeenth library) against the PyTorch composition it replaces, on the same
inputs: the device-side slot arithmetic -- a search over cu_seqlens_q, each token's position, page and row -- and `index_put_` into the
pool, with the divide, clamp and cast in front for an E4M3 pool.  That composition is given every advantage a caller has: the token
indices are made once outside the timed region, nothing syncs, and it writes through the same strided views.

    python tools/perf_paged_kv_write.py [--out profiles/r15/paged_kv_write.jsonl] [--only decode] [--lib DIR/libnnop_hip_paged_kv_write.so ...]

bf16 sources as the K and V slices of a fused QKV projection [T, (64 + 2 * 8) E], KH 8, E 64 and 128, pages of 16 in the vLLM layout
[P, 16, KH, E] with a shuffled table, a 16-bit pool and an E4M3 pool with scales that are no powers of two.  Shapes:

    decode  T = B = 64 and 256, one new token behind 2047 keys each
    chunk   2048 new tokens behind 8192 keys, B = 1
    prompt  8192 new tokens, B = 1

Arms: `torch`, the composition; `hip`, paged_kv_cache_write with all its host checks; `hip_raw`, the library's entry point on a
descriptor made once, which is what a C caller pays per call; and one arm per `--lib`, that raw call on another build of the library
(a build with another NNOP_PAGED_KV_WRITE_BLOCK_TOKENS), named by its directory.  The method is tools/perf_paged_prefill.py's: the arms
alternate in one process, per repeat `--iters` back-to-back calls between HIP events, `--reps` >= 10 repeats after `--warmup` untimed
calls.  These are eager calls: at the decode shapes the interval is the host's launch rate, not the kernel.  Before timing, every arm's
pools are held against the `torch` arm's: bit for bit for a 16-bit pool, and for E4M3 the count of unlike codes is recorded (the tests hold
the library to the CPU's result of the rule's expression, bit for bit; this tool does not judge the GPU's).  One JSON line per shape: microseconds (median, min, max) of the arms, their bytes
per second against the minimal traffic 2 T KH E (2 + bytes of a pool element), and torch / arm with the spread of that ratio over the
paired repeats.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from perf_moe_gemm import time_arms  # noqa: E402

QH, KH, PAGE = 64, 8, 16
SHAPES = (("decode", 64, 1, 2047), ("decode", 256, 1, 2047), ("chunk", 1, 2048, 8192), ("prompt", 1, 8192, 0))   # (kind, B, new, prefix)
F8 = torch.float8_e4m3fn


def torch_write(k, v, kp, vp, table, cu, seqlens, tok, scales):
    """the composition: kp, vp the [P, KH, page, E] views, tok = arange(T)"""
    b = torch.searchsorted(cu[1:], tok, right=True)
    pos = seqlens[b] - (cu[b + 1] - cu[b]) + (tok - cu[b])
    page, row = table[b, pos // PAGE].long(), pos % PAGE
    for pool, x, s in ((kp, k, scales[0]), (vp, v, scales[1])):
        if pool.dtype == torch.uint8:
            x = (x.float() / s[:, None]).clamp(-448, 448).to(F8).view(torch.uint8)
        pool[page, :, row] = x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="decode, chunk or prompt; all by default")
    ap.add_argument("--lib", action="append", default=[], help="another build of libnnop_hip_paged_kv_write.so: one more arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 10, "n >= 10 repeats"

    import __graft_entry__ as ge
    pkg = ge.load_package()
    W, B_ = pkg.paged_kv_write, pkg._lib_paged_kv_write
    dev, dt, lines = "cuda", torch.bfloat16, []
    others = {"hip_raw": B_.load()}
    for path in args.lib:
        lib = C.CDLL(os.path.abspath(path))
        lib.nnop_paged_kv_write.restype, lib.nnop_paged_kv_write.argtypes = B_.PROTOTYPES["nnop_paged_kv_write"]
        others[os.path.basename(os.path.dirname(os.path.abspath(path)))] = lib
    for (kind, B, n, c), E, fmt in ((s, e, f) for s in SHAPES for e in (64, 128) for f in ("16bit", "e4m3")):
        if args.only not in kind:
            continue
        T, pages = B * n, -(-(c + n) // PAGE)
        torch.manual_seed(T + E)
        qkv = torch.randn(T, QH + 2 * KH, E, device=dev).to(dt)
        k, v = qkv[:, QH:QH + KH], qkv[:, QH + KH:]
        table = torch.randperm(B * pages, device=dev).to(torch.int32).view(B, pages)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
        seqlens = torch.full((B,), c + n, dtype=torch.int32, device=dev)
        tok = torch.arange(T, dtype=torch.int32, device=dev)
        scales = [torch.tensor([0.011 * 1.9 ** h for h in range(KH)], device=dev) * f for f in (1.0, 1.3)] if fmt == "e4m3" else [None, None]
        pdt = torch.uint8 if fmt == "e4m3" else dt
        pools = {a: [torch.zeros(B * pages, PAGE, KH, E, dtype=pdt, device=dev).transpose(1, 2) for _ in range(2)] for a in ("torch", "hip", *others)}
        kw = {} if fmt == "16bit" else dict(k_scale=scales[0], v_scale=scales[1])
        arms = {"torch": lambda: torch_write(k, v, *pools["torch"], table, cu, seqlens, tok, scales),
                "hip": lambda: pkg.paged_kv_cache_write(k, v, *pools["hip"], table, cu, seqlens, **kw)}
        d = W._desc(k, v, *pools["hip"], table, scales=fmt == "e4m3")
        for a, lib in others.items():
            arms[a] = lambda a=a, lib=lib: W._raise(lib.nnop_paged_kv_write(
                C.byref(d), *(W._ptr(t) for t in (*pools[a], k, v, *scales, table, cu, seqlens)), W._stream(k)))
        differ = {}
        for a, f in arms.items():
            f()
            differ[a] = sum(int((x != y).sum()) for x, y in zip(pools[a], pools["torch"]))
            assert pools[a][0].any() and differ[a] == (0 if fmt == "16bit" else differ[a]) <= 1e-4 * 2 * T * KH * E, f"{kind} T{T} E{E} {fmt}: arm {a} differs"
        t = time_arms(arms, args.warmup, args.iters, args.reps)
        med = {a: statistics.median(x) for a, x in t.items()}
        nbytes = 2 * T * KH * E * (2 + (1 if fmt == "e4m3" else 2))
        rec = {"shape": f"{kind} bf16->{fmt} B{B} new{n} prefix{c} KH{KH} E{E} page{PAGE}", "reps": args.reps, "iters": args.iters,
               "baseline": "searchsorted + slot arithmetic + index_put_ (+ divide, clamp, cast for e4m3), eager", "min_bytes": nbytes,
               "block_tokens": B_.BLOCK_TOKENS, "elements_unlike_torch": differ,
               **{a: {"us_median": round(med[a], 2), "us_min": round(min(x), 2), "us_max": round(max(x), 2),
                      "gb_per_s": round(nbytes / med[a] / 1e3, 1)} for a, x in t.items()}}
        for a in arms:
            if a != "torch":
                ratios = [b / s for b, s in zip(t["torch"], t[a])]
                rec[f"torch_over_{a}"] = [round(med["torch"] / med[a], 2), round(min(ratios), 2), round(max(ratios), 2)]   # of medians, min, max
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del qkv, pools
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
