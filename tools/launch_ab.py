#!/usr/bin/env python3
"""A/B of the attention launch path (csrc/fa_fwd_inst.hpp, fa_bwd_inst.hpp, fa_launch.hpp, nnop_capi.cpp) against another build of
libnnop_hip.so -- for changes to HOST code that must leave every launch as it was.

    python tools/launch_ab.py --forms   [--out-dir D]      CPU: sweep the six nnop_debug_*_form* hooks, dumps must be byte-identical
    python tools/launch_ab.py --run     [--out-dir D]      GPU: forward + backward of every launcher branch, output hashes must be equal
    python tools/launch_ab.py --time    [--out-dir D]      GPU: timings, libraries alternated (parent, this, parent, this)
    python tools/launch_ab.py --trace A.csv B.csv          compare two rocprofv3 --kernel-trace CSVs of `--child run` runs

A process binds one library (NNOP_LIB_PATH), so each mode starts one fresh child per library (`--child MODE --out FILE`, which can
also be started by hand, e.g. under rocprofv3) and compares what the children wrote.  `--parent` / `--this` name the two libraries
(default nnop.jl_amd/lib_prev/ and nnop.jl_amd/lib/).  Exit status 1 when anything differs.

What the modes do not see: `causal_alt` and `persist_hx` only reorder blocks (same hashes, same grids) -- `--time` times the cases
that use them.  The records of `--run` name the launcher branch each case is meant for (`branch`, from _cases()).
"""
import argparse
import csv
import filecmp
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ---------------------------------------------------------------- form sweep (CPU) -------------------------------------------------
EMBS = (4, 8, 16, 32, 64, 128, 256, 512)
LENS = (1, 63, 128, 129, 256, 512, 1024, 2048, 4096, 16384, 70000)
HEADS = ((1, 1), (4, 4), (8, 2), (32, 8))
BATCHES = (1, 4, 16, 64)
WINDOWS = (None, (70000, 70000), (64, 0), (-1, 7))          # the second one removes no key of any shape here: normalises away
CAPS = (0.0, 30.0)
# every knob at each value its comment in csrc/tuning.hpp / fa_fwd_inst.hpp lists; (None, -1) = all automatic
KNOBS = [(None, -1)] + [(k, v) for k, vals in (("fwd_split", (0, 1)), ("fwd_w64", (0, 1)), ("fwd_duo", (0, 1, 2, 3)),
                                               ("fwd_exact_scale", (0, 1)), ("bwd_w64", (0, 1, 2, 3, 4)), ("bwd_narrow", (0, 1)))
                        for v in vals]
# all automatic: the full cross of (QL, KL); under a forced knob: QL = KL and a few pairs off the diagonal (every length still occurs)
LEN_PAIRS_KNOB = [(n, n) for n in LENS] + [(1, 4096), (4096, 1), (63, 129), (128, 2048), (2048, 129), (70000, 512), (512, 70000),
                                           (16384, 256), (256, 16384), (1024, 63)]


def forms_child(out):
    import ctypes as C
    import __graft_entry__ as ge
    L = ge.load_package()._lib
    lib = L.load()
    f0, b0, f1, b1, f2, b2 = (getattr(lib, "nnop_debug_" + n) for n in ("fwd_form", "bwd_form", "fwd_form_ex", "bwd_form_ex",
                                                                        "fwd_form_cap", "bwd_form_cap"))
    opts = [C.byref(L.FaOpts(window_left=w[0], window_right=w[1])) if w else None for w in WINDOWS]
    caps = [C.c_float(c) for c in CAPS]
    n_cases = 0
    with open(out, "w") as f:
        for knob, val in KNOBS:
            if knob:
                L.debug_set(knob, val)
            pairs = [(a, b) for a in LENS for b in LENS] if knob is None else LEN_PAIRS_KNOB
            for dtype in (0, 1, 2):
                for emb in EMBS:
                    for ql, kl in pairs:
                        for qh, kh in HEADS:
                            for batch in BATCHES:
                                ans = []
                                for flags in range(8):                       # bit 0 causal, bit 1 pair, bit 2 key-padding mask
                                    d = L.FaDesc(dtype=dtype, emb=emb, ql=ql, kl=kl, qh=qh, kh=kh, batch=batch, causal=flags & 1)
                                    dp, hp, hm = C.byref(d), (flags >> 1) & 1, flags >> 2
                                    ans += [f0(dp, hp, hm), b0(dp, hp, hm)]
                                    for o in opts:
                                        ans += [f1(dp, o, hp, hm), b1(dp, o, hp, hm)]
                                        for c in caps:
                                            ans += [f2(dp, o, c, hp, hm), b2(dp, o, c, hp, hm)]
                                n_cases += 8 * len(opts) * len(caps)
                                f.write(f"{knob}={val} dt{dtype} E{emb} QL{ql} KL{kl} H{qh}/{kh} B{batch}: {' '.join(map(str, ans))}\n")
            if knob:
                L.debug_set(knob, -1)
        f.write(f"cases {n_cases}\n")


# ---------------------------------------------------------------- bitwise run (GPU) ------------------------------------------------
S = dict(B=2, QH=4, KH=2, QL=300, KL=256)                       # the small shape; ragged cases: KL 260
BIG = dict(B=8, QH=8, KH=8, QL=2048, KL=2048)                   # the persistent list divides: 64 columns x 8 blocks = 2 steps
ALT = dict(B=4, QH=4, KH=4, QL=4096, KL=4096)                   # causal_alt_run: 16 columns x 32 blocks of 128 rows
ROW32 = dict(fwd_split=0, fwd_w64=0, fwd_duo=0)                 # 16-bit types onto the 32-row forward
MODES = ("plain", "causal", "kpad")


def _cases():
    """(name, branch, dict(dt, E, shape, mode, pair, window, cap, sinks, knobs, ws)) -- ws: 'staged' = the pair workspace"""
    out = []

    def add(name, branch, dt, E, modes=MODES, shape=S, **kw):
        for m in modes:
            out.append((f"{name} {dt} E{E} {m}", branch, dict(dt=dt, E=E, shape=shape, mode=m, **kw)))

    for dt in ("f32", "bf16"):
        for E in (16, 32, 64, 128):
            for nw in (None, 8):
                kn = dict(ROW32, **({"fwd_nw": nw} if nw else {}))
                tag = f"nw{nw or 'auto'}"
                add(f"row32 {tag}", f"launch_fwd_cfg NW={nw or 4}, modes 0 / 1; launch_bwd_cfg default shapes", dt, E, knobs=kn)
                add(f"row32 {tag} pair", f"launch_fwd_cfg NW={nw or 4} mode 2; launch_bwd_cfg MODE 3 (staged workspace)", dt, E,
                    knobs=kn, pair=True, ws="staged")
        add("E256", "fp32: launch_fwd_cfg E 256 + tiled backward; bf16: launch_fwd_w64 E 256 (auto) + launch_bwd_w64 E 256", dt, 256)
        add("E256 pair", "launch_fwd_cfg E 256 mode 2; backward fp32: launch_bwd_generic, bf16: launch_bwd_cfg MODE 3", dt, 256,
            pair=True, ws="staged")
        add("pair small ws", "launch_bwd_cfg MODE 2 (direct pair path)", dt, 64, pair=True)
        for E in (64, 8):
            gen = "launch_fwd_generic / launch_bwd_generic" if E == 8 else "launch_fwd_cfg WIN / CAP; launch_bwd_cfg WIN / kBwdCap"
            add("window", gen, dt, E, window=(64, 0))
            add("cap", gen, dt, E, cap=30.0)
            add("sinks", "launch_fwd_generic / launch_bwd_generic (sink kernels); launch_bwd_sinks" if E == 8 else
                "the sink kernels of the launcher's form (fp32: launch_fwd_cfg, bf16: launch_fwd_duo NZ = 1); launch_bwd_sinks", dt, E, sinks=True)
            add("cap+window+sinks+pair", gen, dt, E, window=(64, 0), cap=30.0, sinks=True, pair=True)
    add("split", "launch_fwd_split", "bf16", 16, modes=("plain",))
    for E in (64, 128):
        add("w64", "launch_fwd_w64 PRE = false", "bf16", E, knobs=dict(fwd_w64=1))
        add("w64 folded scale", "launch_fwd_w64 PRE = true", "bf16", E, knobs=dict(fwd_w64=1, fwd_exact_scale=0))
    add("duo auto", "launch_fwd_duo NZ = 1 (fwd_duo_nz at a small grid)", "bf16", 64)
    add("duo nz2", "launch_fwd_duo NZ = 2", "bf16", 64, knobs=dict(fwd_duo=2))
    add("duo", "launch_fwd_duo E 128 (NZ = 1)", "bf16", 128, knobs=dict(fwd_duo=1))
    add("duo", "launch_fwd_duo E 32 (NZ = 2)", "bf16", 32, knobs=dict(fwd_duo=1))
    for E in (64, 128):
        add("persist", "persist_list: fwd_persist_plan (duo E 64 / w64 E 128) and launch_bwd_w64, both passes", "bf16", E,
            modes=("causal",), shape=BIG)
        add("persist hx", "persist_list hx branch: forward and the dQ pass (per-batch key lengths, no causal mask)", "bf16", E,
            modes=("kpad",), shape=BIG)
    add("causal alt", "causal_alt_run in launch_fwd_cfg, launch_dkdv, launch_dq", "f32", 64, modes=("causal",), shape=ALT)
    add("bwd nw8", "launch_bwd_cfg kWide8", "bf16", 64, knobs=dict(bwd_w64=0, bwd_nw=8))
    add("bwd big7", "launch_bwd_cfg kBig7", "bf16", 128, knobs=dict(bwd_w64=0, bwd_big7=0))
    for E in (64, 128):
        for w64 in (None, 2, 3, 4):
            for narrow in (0, 1):
                kn = dict(bwd_narrow=narrow, **({"bwd_w64": w64} if w64 else {}))
                add(f"bwd_w64={w64 or 'auto'} narrow={narrow}", "launch_bwd_w64 (bwd_w64_forms, fused / separate preprocess)", "bf16", E,
                    knobs=kn)
    return out


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _run_case(pkg, torch, name, c):
    """zero-filled outputs -> forward -> backward; {tensor name: sha256 of its bytes}"""
    A, L = pkg.attention, pkg._lib
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[c["dt"]]
    sh, E, mode = c["shape"], c["E"], c["mode"]
    B, QH, KH, QL = sh["B"], sh["QH"], sh["KH"], sh["QL"]
    KL = sh["KL"] + (4 if (mode == "kpad" and sh is S) else 0)                       # ragged key axis for the padded small cases
    g = torch.Generator(device="cuda").manual_seed(_seed(name))
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dt)
    q, k, v, do = rnd(B, QH, QL, E), rnd(B, KH, KL, E), rnd(B, KH, KL, E), rnd(B, QH, QL, E)
    pair = rnd(B, KL, QL, QH) if c.get("pair") else None
    sinks = torch.randn(QH, device="cuda", generator=g) if c.get("sinks") else None
    kpad = None
    if mode == "kpad":                                                             # per-batch key lengths, at least half the keys
        lens = torch.tensor([KL - (b * 37) % (KL // 2) for b in range(B)], device="cuda")
        kpad = torch.arange(KL, device="cuda")[None, :] < lens[:, None]
    kw = dict(causal=mode == "causal", kpad_mask=kpad, window=c.get("window"), sinks=sinks, softcap=c.get("cap"))
    z = torch.zeros_like
    o, dq, dk, dv = z(q), z(q), z(k), z(v)
    ms, ls = (torch.zeros(B, QH, QL, device="cuda", dtype=dt) for _ in range(2))
    dpair = z(pair) if pair is not None else None
    dsinks = z(sinks) if sinks is not None else None
    ws = torch.zeros(A.bwd_workspace_bytes(q, k, v, causal=kw["causal"], pair=c.get("ws") == "staged"), dtype=torch.uint8, device="cuda")
    for key, val in c.get("knobs", {}).items():
        L.debug_set(key, val)
    try:
        A.fa_fwd_into(o, ms, ls, q, k, v, pair, **kw)
        A.fa_bwd_into(dq, dk, dv, dpair, ws, do, o, ms, ls, q, k, v, pair, dsinks=dsinks, **kw)
        torch.cuda.synchronize()
    finally:
        for key in c.get("knobs", {}):
            L.debug_set(key, -1)
    outs = dict(o=o, ms=ms, ls=ls, dq=dq, dk=dk, dv=dv, dpair=dpair, dsinks=dsinks)
    return {n: hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
            for n, t in outs.items() if t is not None}


def run_child(out):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    res = {}
    for name, branch, c in _cases():
        res[name] = dict(branch=branch, hashes=_run_case(pkg, torch, name, c))
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)


# ---------------------------------------------------------------- timings (GPU) ----------------------------------------------------
def time_child(out):
    """median microseconds per call: the block-order cases (forward, backward), and the host cost per enqueue of a launch-bound call"""
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    A = pkg.attention
    res = {}

    def bufs(dt, E, sh, mode):
        g = torch.Generator(device="cuda").manual_seed(0)
        B, QH, KH, QL, KL = sh["B"], sh["QH"], sh["KH"], sh["QL"], sh["KL"]
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dt)
        q, k, v, do = rnd(B, QH, QL, E), rnd(B, KH, KL, E), rnd(B, KH, KL, E), rnd(B, QH, QL, E)
        kpad = None
        if mode == "kpad":
            lens = torch.tensor([KL - (b * 37) % (KL // 2) for b in range(B)], device="cuda")
            kpad = torch.arange(KL, device="cuda")[None, :] < lens[:, None]
        e = torch.empty_like
        o, dq, dk, dv = e(q), e(q), e(k), e(v)
        ms, ls = (torch.empty(B, QH, QL, device="cuda", dtype=dt) for _ in range(2))
        ws = torch.empty(A.bwd_workspace_bytes(q, k, v, causal=mode == "causal"), dtype=torch.uint8, device="cuda")
        kw = dict(causal=mode == "causal", kpad_mask=kpad)
        fwd = lambda: A.fa_fwd_into(o, ms, ls, q, k, v, **kw)
        bwd = lambda: A.fa_bwd_into(dq, dk, dv, None, ws, do, o, ms, ls, q, k, v, **kw)
        return fwd, bwd

    def gpu_us(fn, warmup=30, iters=50, reps=15):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1000.0 / iters)
        return round(statistics.median(ts), 2)

    for name, dt, E, sh, mode in (("persist bf16 E64 causal", torch.bfloat16, 64, BIG, "causal"),
                                  ("persist bf16 E128 causal", torch.bfloat16, 128, BIG, "causal"),
                                  ("persist hx bf16 E64 kpad", torch.bfloat16, 64, BIG, "kpad"),
                                  ("persist hx bf16 E128 kpad", torch.bfloat16, 128, BIG, "kpad"),
                                  ("causal alt f32 E64", torch.float32, 64, ALT, "causal")):
        fwd, bwd = bufs(dt, E, sh, mode)
        res[name + " fwd us"] = gpu_us(fwd)
        res[name + " bwd us"] = gpu_us(bwd)
    # launch-bound: host microseconds per enqueue, a few thousand calls ending in one synchronise
    fwd, _ = bufs(torch.bfloat16, 64, dict(B=1, QH=4, KH=4, QL=128, KL=128), "plain")
    for _ in range(200):
        fwd()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(4000):
            fwd()
        t1 = time.perf_counter()                                 # enqueue cost only: the synchronise is outside
        torch.cuda.synchronize()
        ts.append((t1 - t0) * 1e6 / 4000)
    res["launch-bound bf16 E64 (1,4,4,128,128) host us per enqueue"] = round(statistics.median(ts), 3)
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)


# ---------------------------------------------------------------- trace comparison -------------------------------------------------
def trace_rows(path):
    """(kernel name, grid, workgroup size, LDS bytes) of the library's kernels in dispatch order, from a rocprofv3 kernel-trace CSV"""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["LDS_Block_Size"])
            for r in rows if "nnop" in r["Kernel_Name"]]


def trace_compare(a, b):
    ra, rb = trace_rows(a), trace_rows(b)
    bad = [i for i, (x, y) in enumerate(zip(ra, rb)) if x != y]
    print(f"kernel trace: {len(ra)} vs {len(rb)} launches of the library's kernels, {len(set(ra))} distinct (name, grid, workgroup, LDS), "
          f"{len(bad)} differ")
    for i in bad[:10]:
        print(f"  #{i}\n    parent {ra[i]}\n    this   {rb[i]}")
    return 0 if (not bad and len(ra) == len(rb) and ra) else 1


# ---------------------------------------------------------------- drivers ----------------------------------------------------------
def child(mode, lib, out):
    env = dict(os.environ, NNOP_LIB_PATH=os.path.abspath(lib), NNOP_DEBUG_HOOKS="1")
    # (a child that fails or hangs ends the comparison: nothing else is started after it)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--out", out], env=env, check=True, timeout=900)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--trace", nargs=2, metavar=("PARENT_CSV", "THIS_CSV"))
    ap.add_argument("--child", choices=("forms", "run", "time"))
    ap.add_argument("--out", help="with --child: the file to write")
    ap.add_argument("--parent", default=os.path.join(ROOT, "nnop.jl_amd", "lib_prev", "libnnop_hip.so"))
    ap.add_argument("--this", default=os.path.join(ROOT, "nnop.jl_amd", "lib", "libnnop_hip.so"))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r06"))
    a = ap.parse_args()
    if a.child:
        {"forms": forms_child, "run": run_child, "time": time_child}[a.child](a.out)
        return 0
    if a.trace:
        return trace_compare(*a.trace)
    os.makedirs(a.out_dir, exist_ok=True)
    path = lambda n: os.path.join(a.out_dir, n)
    rc = 0
    if a.forms:
        child("forms", a.parent, path("forms_parent.txt"))
        child("forms", a.this, path("forms_this.txt"))
        same = filecmp.cmp(path("forms_parent.txt"), path("forms_this.txt"), shallow=False)
        with open(path("forms_this.txt"), "rb") as f:
            data = f.read()
        rec = dict(identical=same, cases=int(data.splitlines()[-1].split()[1]), lines=len(data.splitlines()) - 1,
                   bytes=len(data), sha256=hashlib.sha256(data).hexdigest())
        with open(path("forms.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print("form sweep:", json.dumps(rec))
        rc |= 0 if same else 1
    if a.run:
        child("run", a.parent, path("run_parent.json"))
        child("run", a.this, path("run_this.json"))
        old, new = json.load(open(path("run_parent.json"))), json.load(open(path("run_this.json")))
        bad = sorted(n for n in set(old) | set(new) if old.get(n) != new.get(n))
        print(f"bitwise run: {len(new)} cases, {sum(len(r['hashes']) for r in new.values())} tensors, {len(bad)} cases differ")
        for n in bad:
            print("  DIFFERS", n, old.get(n, {}).get("hashes"), new.get(n, {}).get("hashes"))
        rc |= 1 if (bad or not new) else 0
    if a.time:
        runs = []
        for tag, lib in (("parent", a.parent), ("this", a.this), ("parent", a.parent), ("this", a.this)):
            child("time", lib, path("time_tmp.json"))
            runs.append((tag, json.load(open(path("time_tmp.json")))))
        os.remove(path("time_tmp.json"))
        # the margin of a figure is the spread between the parent's two runs: this build must lie no further than that from them
        lines = ["figure: parent run 1, run 2 (spread) | this run 1, run 2 (spread) | within the parent's margin?"]
        for key in sorted(runs[0][1]):
            p = [r[key] for t, r in runs if t == "parent"]
            n = [r[key] for t, r in runs if t == "this"]
            m = max(p) - min(p)
            ok = all(min(p) - m <= x <= max(p) + m for x in n)
            rc |= 0 if ok else 1
            lines.append(f"{key}: {p[0]}, {p[1]} ({m:.3f}) | {n[0]}, {n[1]} ({max(n) - min(n):.3f}) | {'yes' if ok else 'NO'}")
        with open(path("launch_ab.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main())
